"""MultiDiffusion views (arXiv 2302.08113; diffusers' ``StableDiffusionPanoramaPipeline``): a latent larger than the one the
networks were trained on is covered by overlapping windows of the training size, every window is denoised as an ordinary
sample, and after every sampler step the windows are averaged where they overlap.

This module holds the geometry and the DEFINITION of the blend in torch (``blend_views_reference``); the HIP kernel
(``csrc/multidiff.hip``, ``ops.view_blend``) computes the same bits in one in-place launch.  Restated from the paper and from
diffusers' pipeline; parity with diffusers is unpinned (its package is not a dependency of this one).

Not here (each is refused or documented where it can be asked for): circular padding (panoramas that wrap), different prompts or
weights per view, non-square windows, training.
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import torch

MAX_COVER = 64  # covering views per pixel the blend supports: diffusers' default window 64 with stride 8 (8 x 8)


class ViewGeometry(NamedTuple):
    """``rows x cols`` windows of ``wh x ww`` latent pixels, window (r, c) starting at ``(r * sy, c * sx)``, over a latent of
    ``H x W`` = ``((rows - 1) * sy + wh) x ((cols - 1) * sx + ww)``.  View index ``v = r * cols + c`` (row-major)."""
    rows: int
    cols: int
    wh: int
    ww: int
    sy: int
    sx: int

    @property
    def num_views(self) -> int:
        return self.rows * self.cols

    @property
    def height(self) -> int:
        return (self.rows - 1) * self.sy + self.wh

    @property
    def width(self) -> int:
        return (self.cols - 1) * self.sx + self.ww

    @property
    def max_cover(self) -> int:
        """The largest number of views that cover one pixel: per axis min(windows, ceil(window / stride))."""
        return min(self.rows, -(-self.wh // self.sy)) * min(self.cols, -(-self.ww // self.sx))

    @property
    def views(self) -> List[Tuple[int, int, int, int]]:
        """``(h_start, h_end, w_start, w_end)`` per view, row-major: diffusers' ``get_views``."""
        return [(r * self.sy, r * self.sy + self.wh, c * self.sx, c * self.sx + self.ww)
                for r in range(self.rows) for c in range(self.cols)]


def _axis(name: str, length: int, window: int, stride: int) -> Tuple[int, int]:
    """(number of windows, window length) along one axis."""
    if length <= window:
        return 1, length
    if (length - window) % stride:
        lo = window + (length - window) // stride * stride
        raise ValueError(f"MultiDiffusion: a latent {name} of {length} is not window + k * stride (window {window}, stride "
                         f"{stride}): the last {length - lo} pixels would be covered by no view.  The nearest sizes that fit "
                         f"are {lo} and {lo + stride}")
    return (length - window) // stride + 1, window


def view_geometry(latent_h: int, latent_w: int, window_size: int = 64, stride: int = 8) -> ViewGeometry:
    """The windows of a ``latent_h x latent_w`` latent (sizes in latent pixels).  ``ValueError`` for a size the windows do not
    tile exactly (diffusers leaves those border pixels uncovered and divides by zero); ``NotImplementedError`` for more than
    ``MAX_COVER`` covering views per pixel and for a stride above the window (pixels between two windows)."""
    latent_h, latent_w, window_size, stride = int(latent_h), int(latent_w), int(window_size), int(stride)
    if latent_h < 1 or latent_w < 1 or window_size < 1 or stride < 1:
        raise ValueError("MultiDiffusion: latent sizes, window_size and stride are positive integers")
    rows, wh = _axis("height", latent_h, window_size, stride)
    cols, ww = _axis("width", latent_w, window_size, stride)
    geo = ViewGeometry(rows, cols, wh, ww, stride, stride)
    if (rows > 1 or cols > 1) and stride > window_size:
        raise NotImplementedError(f"MultiDiffusion: stride {stride} above the window {window_size} leaves pixels uncovered")
    if geo.max_cover > MAX_COVER:
        raise NotImplementedError(f"MultiDiffusion: window {window_size} with stride {stride} covers a pixel with "
                                  f"{geo.max_cover} views; at most {MAX_COVER} are supported (window 64 with stride 8)")
    return geo


def get_views(latent_h: int, latent_w: int, window_size: int = 64, stride: int = 8) -> List[Tuple[int, int, int, int]]:
    """diffusers' ``get_views``: ``(h_start, h_end, w_start, w_end)`` of ``(L - window) // stride + 1`` windows per axis with
    starts ``k * stride``, listed row-major; an axis not longer than the window has one window of its own length."""
    return view_geometry(latent_h, latent_w, window_size, stride).views


def _geometry_of(views_or_geometry) -> ViewGeometry:
    if isinstance(views_or_geometry, ViewGeometry):
        return views_or_geometry
    return ViewGeometry(*(int(v) for v in views_or_geometry))


def gather_views(x: torch.Tensor, views) -> torch.Tensor:
    """``[N, C, H, W]`` -> ``[N * V, C, wh, ww]``; sample ``n``'s view ``v`` lands at index ``n * V + v``.  ``views``: a
    ``ViewGeometry`` or a list of ``(h_start, h_end, w_start, w_end)``."""
    vs = views.views if isinstance(views, ViewGeometry) else list(views)
    if x.dim() != 4:
        raise ValueError("gather_views: x is [N, C, H, W]")
    cut = torch.stack([x[:, :, h0:h1, w0:w1] for (h0, h1, w0, w1) in vs], dim=1)  # [N, V, C, wh, ww]
    return cut.reshape(x.shape[0] * len(vs), x.shape[1], cut.shape[-2], cut.shape[-1])


def cover_count(geometry, device=None) -> torch.Tensor:
    """fp32 ``[H, W]``: the number of views that cover each pixel (exact: small integers)."""
    geo = _geometry_of(geometry)
    count = torch.zeros(geo.height, geo.width, dtype=torch.float32, device=device)
    for (h0, h1, w0, w1) in geo.views:
        count[h0:h1, w0:w1] += 1.0
    return count


def blend_views_global(views_tensor: torch.Tensor, geometry) -> torch.Tensor:
    """The global fp32 ``[N, C, H, W]`` of the blend below."""
    geo = _geometry_of(geometry)
    V = geo.num_views
    if views_tensor.dim() != 4 or views_tensor.shape[0] % V or tuple(views_tensor.shape[-2:]) != (geo.wh, geo.ww):
        raise ValueError(f"blend_views: expected [N * {V}, C, {geo.wh}, {geo.ww}], got {tuple(views_tensor.shape)}")
    N, Cc = views_tensor.shape[0] // V, views_tensor.shape[1]
    m = views_tensor.to(torch.float32).reshape(N, V, Cc, geo.wh, geo.ww)
    value = torch.zeros(N, Cc, geo.height, geo.width, dtype=torch.float32, device=views_tensor.device)
    for v, (h0, h1, w0, w1) in enumerate(geo.views):  # ascending view index: ((m0 + m1) + m2) + ...
        value[:, :, h0:h1, w0:w1] += m[:, v]
    return value / cover_count(geo, views_tensor.device)  # IEEE division, not a multiply by the reciprocal


def blend_views_reference(views_tensor: torch.Tensor, geometry, return_global: bool = False):
    """THE definition of the blend, in torch, on any device: ``value = 0``; for ``v`` ascending ``value[window_v] += view_v``;
    ``global = value / count``; the views regathered from ``global``.  fp32 arithmetic; returns fp32 ``[N * V, C, wh, ww]``
    (and the global ``[N, C, H, W]`` with ``return_global``).  CPU pipelines use this function; ``ops.view_blend`` is the
    kernel with the same bits."""
    geo = _geometry_of(geometry)
    glob = blend_views_global(views_tensor, geo)
    out = gather_views(glob, geo)
    return (out, glob) if return_global else out
