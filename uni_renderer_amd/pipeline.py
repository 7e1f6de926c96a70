"""L3 sampling pipeline (mirror of the reference's ``models/pipeline.py`` ``UniRendererPipeline``, 124-4290).

The reference class has no ``__call__``; its live entry points are kept with their names,
keyword blocks and return conventions:

  ``real_image2mask_3mod_albedo`` (ref 2391-2808)  inverse rendering of a real image   enc + unet + dec per step
  ``image2mask_3mod_albedo``      (ref 1990-2390)  same, tensor inputs in [0, 1]
  ``mask2image_3mod_albedo``      (ref 1368-1697)  rendering from attributes             enc + unet per step

Per step the three networks run through ``graph.GraphedDualStreamStep`` (one hipGraph replay) when shapes are
static, otherwise eagerly; both only enqueue HIP kernels.  The frozen side models (VAE, CLIP text encoder --
SURVEY.md S2) are duck-typed objects supplied by the caller exactly as in ``eval/test_real.py:470-495`` and are
out of scope here; ``prompt_embeds=`` / tensor latents let the loop run without them.  Schedulers follow the
diffusers protocol (``scheduler_img`` ... ``scheduler_env`` attributes, test_real.py:485-492); a built-in x0
DDIM (schedulers.py) is attached by default.  The 11 legacy 12/16-channel methods of the reference
 are not reproduced.
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from typing import Any, Dict, List, Optional, Tuple, Union

import torch

from .controlnet import AttributeDecoderModel, AttributeEncoderModel, UNet2DConditionModel
from . import ops
from .ip_adapter import read_ip_adapter_file
from .multidiffusion import ViewGeometry, gather_views, view_geometry
from .lora import read_lora_file, scale_of
from .graph import GraphedDualStreamStep, GraphedHoistedStep, dual_stream_step
from .schedulers import DDIMScheduler, device_plan, retrieve_timesteps
from .unet_2d_blocks import freeu_state

SCHEDULER_NAMES = ("img", "attr", "material", "albedo", "normal", "spec_light", "diff_light", "env")
ATTR_GROUPS = ("material", "normal", "albedo", "spec_light", "diff_light", "env")  # after the mask group


class _SamplerState:
    """The device state one captured sampling loop carries between its replays, for a ``schedulers.DevicePlan`` kind: the step
    counter, the plan's table and timesteps, the fp32 master copy of the evolving latent and what the kind's update kernel
    keeps besides -- UniPC: the corrected sample L and the two previous predictions (``ur_unipc_update``); ``sde-*``: the
    previous prediction and the noise key (``ur_sde_update``).  The graph knows the buffers, ``reset`` writes their values."""

    def __init__(self, kind: str, nsteps: int, width: int):
        self.kind, self.n, self.width = kind, nsteps, width

    def allocate(self, mshape, dev, round_master: bool):
        z = lambda *lead: torch.zeros(lead + tuple(mshape), dtype=torch.float32, device=dev)
        self.round_master = round_master
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.coef, self.tvals, self.master = torch.zeros(self.n, self.width, device=dev), torch.zeros(self.n, device=dev), z()
        if self.kind == "unipc":
            self.last, self.hist = z(), z(2)
        elif self.kind != "ddim":
            self.hist, self.seed = z(), torch.zeros(1, dtype=torch.int64, device=dev)

    def reset(self, x0, seed: Optional[int], plan):
        """Step 0 of a call: ``plan``'s table (same kind and length; its values may differ from the last call's), the initial
        sample ``x0``, the call's noise key."""
        self.step.zero_()
        self.coef.copy_(plan.coef)
        self.tvals.copy_(plan.tvals)
        self.master.copy_(x0)
        if self.kind == "unipc":
            self.last.copy_(self.master)  # L_0 = the initial sample
            self.hist.zero_()
        elif self.kind != "ddim":
            self.hist.zero_()
            self.seed.fill_(0 if seed is None else seed)

    def update(self, pred_nhwc, c0: int, lat, guidance: Optional[float], cfg_channels: int):
        """The kind's update kernel: prediction -> next input ``lat``, at the device-side step."""
        kw = dict(round_master=self.round_master, guidance=guidance, cfg_channels=cfg_channels)
        if self.kind == "ddim":
            ops.ddim_update(pred_nhwc, c0, lat, self.coef, self.step, self.n, master=self.master, **kw)
        elif self.kind == "unipc":
            ops.unipc_update(pred_nhwc, c0, lat, self.coef, self.step, self.n, self.last, self.master, self.hist, **kw)
        else:
            ops.sde_update(pred_nhwc, c0, lat, self.coef, self.step, self.n, self.seed, self.master, self.hist, **kw)


class UniRendererPipeline:
    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet: UNet2DConditionModel = None,
                 controlnet: AttributeEncoderModel = None, controldec: AttributeDecoderModel = None, scheduler=None,
                 safety_checker=None, feature_extractor=None, image_encoder=None, requires_safety_checker: bool = False):
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.unet, self.controlnet, self.controldec = unet, controlnet, controldec
        self.safety_checker, self.feature_extractor, self.image_encoder = safety_checker, feature_extractor, image_encoder
        for n in SCHEDULER_NAMES:  # test_real.py:485-492 overwrites these with UniPC instances
            setattr(self, f"scheduler_{n}", scheduler if (scheduler is not None and n == "img") else DDIMScheduler())
        self.vae_scale_factor = 8
        self.use_hip_graph = True
        self.use_fused_sampler = True  # whole sampling loop on the device when the configuration allows (_fusable)
        # The loops' invariant half once per call instead of once per step (hoist.py): inverse direction = UNet conv_in + down +
        # mid and the decoder's exchange convs once, UNet up / conv_out and the encoder's exchange convs never (their results
        # are dropped, ref 2670: ``_, ..., _ =``); rendering direction = the whole encoder once.  UR_HOIST=0 / False: every
        # network on every step (the grouped enc || unet, unet || dec executor of fused.py).
        self.hoist_invariants = os.environ.get("UR_HOIST", "1") != "0"
        self.rerun_invariants = False  # tests: the hoisted executor with its prologue replayed before EVERY step
        # hoisted on-device loops: time embedding + every resnet's time projection for ALL steps once per call (hoist.time_tables)
        self.precompute_time_tables = True
        self._sample_graphs: Dict[Any, Any] = {}
        self._graphs: Dict[Tuple, GraphedDualStreamStep] = {}
        self._progress_kwargs: Dict[str, Any] = {}
        self._guidance_scale = 0.0
        self._num_timesteps = 0
        self._multidiffusion: Optional[Dict[str, Any]] = None  # enable_multidiffusion: window_size, stride, view_batch_size

    # ---- construction / placement ---------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=None, **components):
        """Components given as keywords are used as-is (test_real.py:470-482); unet / controlnet / controldec
        missing from the keywords are loaded from the diffusers-layout subfolders of the path."""
        for name, klass in (("unet", UNet2DConditionModel), ("controlnet", AttributeEncoderModel),
                            ("controldec", AttributeDecoderModel)):
            if components.get(name) is None and os.path.isdir(os.path.join(pretrained_model_name_or_path, name)):
                components[name] = klass.from_pretrained(pretrained_model_name_or_path, subfolder=name,
                                                         torch_dtype=torch_dtype)
        known = ("vae", "text_encoder", "tokenizer", "unet", "controlnet", "controldec", "scheduler", "safety_checker",
                 "feature_extractor", "image_encoder", "requires_safety_checker")
        return cls(**{k: v for k, v in components.items() if k in known})

    def to(self, *args, **kwargs):
        for n in ("vae", "text_encoder", "unet", "controlnet", "controldec"):
            m = getattr(self, n)
            if m is not None and hasattr(m, "to"):
                setattr(self, n, m.to(*args, **kwargs))
        self.invalidate_graphs()
        return self

    def invalidate_graphs(self):
        """Drop every captured step / sampling graph.  A captured graph is bound to the static input buffers of its
        ``GraphedDualStreamStep`` and to the PACKED copies of the weights it was captured with, so it must not outlive a
        device move or a weight update.  ``to()`` calls this; weight updates (optimizer steps, ``load_state_dict``) are
        detected per sampling call through ``_weights_signature``."""
        self._graphs.clear()
        self._sample_graphs.clear()

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (arXiv 2309.11497; ref 739-759) on the image stream's UNet: ``s1`` / ``s2`` attenuate the lowest frequencies of
        the skips of up-block stage 1 / 2, ``b1`` / ``b2`` amplify the first half of their backbone channels.  The factors are
        kernel arguments of the captured step, so they are part of the graph key (``_graph_for``): graphs captured in
        another FreeU state are never replayed."""
        if getattr(self, "unet", None) is None:
            raise ValueError("The pipeline must have `unet` for using FreeU.")
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        """ref 762-764."""
        self.unet.disable_freeu()

    # ---- MultiDiffusion views for latents larger than the training size ------------------------------------------
    def enable_multidiffusion(self, window_size: int = 64, stride: int = 8, view_batch_size: Optional[int] = None):
        """MultiDiffusion (arXiv 2302.08113; diffusers' ``StableDiffusionPanoramaPipeline``; restated from both, parity with
        diffusers unpinned) for ``real_image2mask_3mod_albedo``, ``image2mask_3mod_albedo`` and ``mask2image_3mod_albedo``: a
        latent larger than ``window_size`` (on either axis; sizes in LATENT pixels, 64 = the 512 x 512 images the networks
        were trained on) is covered by overlapping square windows at every ``stride`` pixels, every window ("view") is
        denoised as an ordinary sample of the batch, and after every sampler step the views are averaged where they overlap
        (``ops.view_blend``, one launch inside the captured loop).  The inputs are encoded and the noise drawn at full size;
        ``latents=`` / ``image_latents=`` / ``mask_latents=`` / ``attr_latents=`` are global tensors, cut into views once per
        call; the prompt and image-prompt embeddings are repeated per view; the results are global.

        Every view is its own batch element, so it has its own multistep history (UniPC's corrected sample, the previous
        predictions) -- what diffusers does when it saves and restores the scheduler state per view.  A sampler with a noise
        term keeps its ONE stream over the ``[N * V, ...]`` view batch: overlapping views get independent noise, as in diffusers.

        The latent must be ``window_size + k * stride`` long on every axis longer than the window (``ValueError`` names the
        nearest sizes), and at most 64 views may cover a pixel (window 64 with stride 8; ``NotImplementedError`` beyond).
        ``view_batch_size``: the step-by-step loop runs the networks over at most that many views at a time (memory); the
        on-device loop always takes all views as one batch.  A latent not larger than the window, or ``disable_multidiffusion``,
        is today's path bit for bit: no launch, no graph key changes.

        Not supported: circular padding (panoramas that wrap), different prompts or weights per view, non-square windows,
        folding the blend into the update kernels, training."""
        window_size, stride = int(window_size), int(stride)
        if window_size < 1 or stride < 1:
            raise ValueError("enable_multidiffusion: window_size and stride are positive numbers of latent pixels")
        if view_batch_size is not None and int(view_batch_size) < 1:
            raise ValueError("enable_multidiffusion: view_batch_size is None or >= 1")
        self._multidiffusion = dict(window_size=window_size, stride=stride,
                                    view_batch_size=None if view_batch_size is None else int(view_batch_size))

    def disable_multidiffusion(self):
        self._multidiffusion = None

    def _view_geometry(self, h8: int, w8: int) -> Optional[ViewGeometry]:
        """The views of an ``h8 x w8`` latent, or None when the call is not a MultiDiffusion call (switch off, or the latent
        not larger than the window)."""
        md = self._multidiffusion
        if md is None or (h8 <= md["window_size"] and w8 <= md["window_size"]):
            return None
        return view_geometry(h8, w8, md["window_size"], md["stride"])

    def _view_chunks(self, nv: int, cfg: bool, device):
        """Batch-row index tensors of the step-by-step loop's network calls under ``view_batch_size`` (both halves of a
        guided batch together), or None for one call over all views."""
        vb = self._multidiffusion["view_batch_size"]
        if vb is None or vb >= nv:
            return None
        chunks = [torch.arange(s, min(s + vb, nv), device=device) for s in range(0, nv, vb)]
        return [torch.cat([i, i + nv]) for i in chunks] if cfg else chunks

    @staticmethod
    def _blend_views(parts, geo: ViewGeometry):
        """The per-step blend of the step-by-step loops: the latent groups ``parts`` ([N * V, c, wh, ww] each, one dtype) as ONE
        latent through ``ops.view_blend`` -- what the on-device loop does to its master copy.  Returns (the blended
        groups, the global fp32 [N, C, H, W])."""
        cat = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
        master = cat.float().contiguous()
        if master is cat or master.data_ptr() == cat.data_ptr():
            master = cat.clone()
        out = torch.empty(cat.shape, dtype=cat.dtype, device=cat.device)
        glob = torch.empty(cat.shape[0] // geo.num_views, cat.shape[1], geo.height, geo.width, dtype=torch.float32, device=cat.device)
        ops.view_blend(master, out, glob, geo, halves=1, round_master=cat.dtype != torch.float32)
        return list(out.split([p_.shape[1] for p_ in parts], dim=1)), glob

    # ---- IP-Adapter image prompts (the reference's IPAdapterMixin, ref 11,125) ------------------------------
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder: Optional[str] = None,
                        weight_name: Optional[str] = None, **kwargs):
        """Loads an IP-Adapter (arXiv 2308.06721) into the UNet: a state dict in the original layout (``image_proj.*``,
        ``ip_adapter.{id}.to_{k,v}_ip.weight``; flat or nested), a local ``.safetensors`` / ``.bin`` file, or a directory holding
        ``[subfolder/]weight_name``.  Nothing is loaded from a hub.  Every sampling call then needs ``ip_adapter_image=`` and the
        pipeline an ``image_encoder`` (a CLIP vision tower with projection, supplied by the caller like the text encoder).  Only
        the UNet is adapted; the attribute encoder / decoder keep their prompt-only attention."""
        if getattr(self, "unet", None) is None:
            raise ValueError("The pipeline must have `unet` for using an IP-Adapter.")
        self.unet._load_ip_adapter_weights(read_ip_adapter_file(pretrained_model_name_or_path_or_dict, subfolder, weight_name))

    def set_ip_adapter_scale(self, scale: float):
        """The image prompt's weight in every cross-attention of the UNet.  A kernel argument of the captured step, so it is
        part of the graph key: graphs captured at another scale are never replayed."""
        self.unet.set_ip_adapter_scale(scale)

    def unload_ip_adapter(self):
        """Drops the adapter; the pipeline behaves exactly as before ``load_ip_adapter``."""
        self.unet.unload_ip_adapter()

    def encode_image(self, image, device, num_images_per_prompt):
        """ref 433-444: PIL / array through ``feature_extractor`` (a pixel tensor as it is), the CLIP image embedding of
        ``image_encoder``, repeated per prompt; returns ``(image_embeds, zeros_like)``."""
        dtype = next(self.image_encoder.parameters()).dtype
        if not isinstance(image, torch.Tensor):
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=dtype)
        image_embeds = self.image_encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return image_embeds, torch.zeros_like(image_embeds)

    def _prepare_ip_adapter(self, ip_adapter_image, device, total: int, num_images_per_prompt: int, views: int = 1):
        """Puts the image prompt of a sampling call into the UNet's static embedding buffer: ``total`` rows, under
        classifier-free guidance ``[zeros ; embeds]`` in the order of ``_batch_prompt``.  ``views`` > 1 (MultiDiffusion): every
        row repeated for its sample's views."""
        loaded = self.unet.ip_adapter_state() is not None
        if ip_adapter_image is None:
            if loaded:
                raise ValueError("an IP-Adapter is loaded: pass ip_adapter_image=, or unload_ip_adapter() first")
            return
        if not loaded:
            raise ValueError("ip_adapter_image was passed but no IP-Adapter is loaded (load_ip_adapter first)")
        if self.image_encoder is None:
            raise ValueError("ip_adapter_image needs an image_encoder (the CLIP vision tower is not part of this package: pass "
                             "image_encoder= to the pipeline)")
        if not isinstance(ip_adapter_image, torch.Tensor) and self.feature_extractor is None:
            raise ValueError("ip_adapter_image as a PIL image / array needs a feature_extractor; pass a pixel tensor otherwise")
        embeds, uncond = self.encode_image(ip_adapter_image, device, num_images_per_prompt)
        if embeds.shape[0] != total:
            if total % embeds.shape[0]:
                raise ValueError(f"{embeds.shape[0]} image embeddings for a batch of {total}")
            embeds = embeds.repeat(total // embeds.shape[0], 1)
            uncond = torch.zeros_like(embeds)
        if views > 1:
            embeds = embeds.repeat_interleave(views, dim=0)
            uncond = torch.zeros_like(embeds)
        if self.do_classifier_free_guidance:
            embeds = torch.cat([uncond, embeds])
        self.unet.set_ip_adapter_image_embeds(embeds)

    # ---- VAE slicing / tiling (ref 185-215): the VAE's own switches ---------------------------------------
    def enable_vae_slicing(self):
        """The VAE encodes / decodes a batch one sample at a time (ref 185-190)."""
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        """ref 193-198."""
        self.vae.disable_slicing()

    def enable_vae_tiling(self):
        """The VAE processes inputs larger than its tile size as overlapping tiles, stitched by one fused launch
        (``AutoencoderKL.enable_tiling``; ref 201-207).  Tiling changes the images, as in the reference: every tile has its
        own GroupNorm statistics and attention."""
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        """ref 210-215."""
        self.vae.disable_tiling()

    # ---- LoRA (the reference's LoraLoaderMixin, UNet part) ----------------------------------------------
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name=None, adapter_name: str = "default", **kwargs):
        """Loads a LoRA file (a state dict, a ``.safetensors`` file or a directory holding ``weight_name``; local files only)
        into the UNet.  ``unet.``-prefixed and unprefixed keys go to ``unet.load_attn_procs``; ``.alpha`` entries are the
        network alphas.  The text encoder is not part of this package: ``text_encoder.`` keys raise ``NotImplementedError``."""
        sd = read_lora_file(pretrained_model_name_or_path_or_dict, weight_name)
        te = [k for k in sd if k.startswith(("text_encoder.", "text_encoder_2."))]
        if te:
            raise NotImplementedError(f"LoRA key {te[0]!r}: adapters for the text encoder are not supported (the text "
                                      "encoder is not run by this package)")
        self.unet.load_attn_procs(sd, adapter_name=adapter_name)

    def unload_lora_weights(self):
        self.unet.unload_lora()

    def fuse_lora(self, lora_scale: float = 1.0, **kwargs):
        self.unet.fuse_lora(lora_scale)

    def unfuse_lora(self, **kwargs):
        self.unet.unfuse_lora()

    def _weights_signature(self):
        """(device, (data_ptr, version) of every parameter) of the three networks: in-place updates bump ``_version``,
        re-assignments change ``data_ptr``.  ~1.7 k parameters: evaluated once per sampling call, not per step."""
        nets = [m for m in (self.unet, self.controlnet, self.controldec) if m is not None]
        # ... and the identity and scale of the UNet's IP-Adapter, whose tensors are no parameters
        return (str(self.device), self.unet.ip_adapter_state()) + tuple((p_.data_ptr(), p_._version) for m in nets for p_ in m.parameters())

    @property
    def device(self):
        return self.unet.device

    _execution_device = device

    def set_progress_bar_config(self, **kwargs):
        self._progress_kwargs = kwargs

    @contextmanager
    def progress_bar(self, total=None):
        try:
            from tqdm.auto import tqdm

            bar = tqdm(total=total, **self._progress_kwargs)
        except Exception:  # pragma: no cover
            bar = None
        try:
            yield bar if bar is not None else _NullBar()
        finally:
            if bar is not None:
                bar.close()

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale != 0  # ref 806-808

    # ---- helpers (ref 251-431, 674-719) --------------------------------------------------------------
    def encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                      prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
        if prompt_embeds is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("pass prompt_embeds= or attach tokenizer + text_encoder (CLIP is out of scope here)")
            prompts = [prompt] if isinstance(prompt, str) else list(prompt)
            ids = self.tokenizer(prompts, padding="max_length", max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors="pt").input_ids
            prompt_embeds = self.text_encoder(ids.to(device))[0]
        bs = prompt_embeds.shape[0]
        prompt_embeds = prompt_embeds.to(device=device).repeat(1, num_images_per_prompt, 1).view(
            bs * num_images_per_prompt, prompt_embeds.shape[1], -1)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            if self.text_encoder is not None and self.tokenizer is not None:
                neg = [""] * bs if negative_prompt is None else ([negative_prompt] * bs if isinstance(negative_prompt, str) else list(negative_prompt))
                ids = self.tokenizer(neg, padding="max_length", max_length=prompt_embeds.shape[1], truncation=True,
                                     return_tensors="pt").input_ids
                negative_prompt_embeds = self.text_encoder(ids.to(device))[0]
            else:
                negative_prompt_embeds = torch.zeros_like(prompt_embeds[:bs])
        if do_classifier_free_guidance:
            negative_prompt_embeds = negative_prompt_embeds.to(device=device, dtype=prompt_embeds.dtype).repeat(
                1, num_images_per_prompt, 1).view(bs * num_images_per_prompt, prompt_embeds.shape[1], -1)
        return prompt_embeds, negative_prompt_embeds

    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt, device, dtype,
                      do_classifier_free_guidance=False, guess_mode=False):
        """PIL / ndarray / tensor -> [B,3,H,W] in [-1, 1] (VaeImageProcessor.preprocess semantics)."""
        if not torch.is_tensor(image):
            import numpy as np

            imgs = image if isinstance(image, (list, tuple)) else [image]
            arr = []
            for im in imgs:
                if hasattr(im, "resize"):  # PIL
                    im = np.asarray(im.convert("RGB").resize((width, height)), dtype=np.float32) / 255.0
                arr.append(torch.from_numpy(np.asarray(im, dtype=np.float32)).permute(2, 0, 1))
            image = torch.stack(arr) * 2.0 - 1.0
        if image.shape[0] == 1 and batch_size > 1:
            image = image.repeat(batch_size, 1, 1, 1)
        return image.to(device=device, dtype=dtype)

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        shape = (batch_size, num_channels_latents, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            latents = torch.randn(shape, generator=generator, device=device, dtype=dtype)
        else:
            latents = latents.to(device)
        return latents * self.scheduler_img.init_noise_sigma  # ref 719

    def _batch_prompt(self, prompt_embeds, negative_prompt_embeds, batch_size):
        """Broadcast a single prompt to the image batch (ref 2504-2507), then stack [uncond, cond] for CFG."""
        def fit(e):
            if e.shape[0] != batch_size:
                if batch_size % e.shape[0]:
                    raise ValueError(f"{e.shape[0]} prompt embeddings for a batch of {batch_size}")
                e = e.repeat(batch_size // e.shape[0], 1, 1)
            return e

        prompt_embeds = fit(prompt_embeds)
        if self.do_classifier_free_guidance:
            prompt_embeds = torch.cat([fit(negative_prompt_embeds), prompt_embeds])
        return prompt_embeds

    def _vae_encode(self, image):
        w = getattr(self.vae, "dtype", image.dtype)
        return self.vae.encode(image.to(dtype=w)).latent_dist.sample() * self.vae.config.scaling_factor

    def _vae_decode(self, latents, generator=None):
        return self.vae.decode(latents / self.vae.config.scaling_factor, return_dict=False)[0]

    @staticmethod
    def _postprocess(image: torch.Tensor, output_type: str):
        image = (image.float() / 2 + 0.5).clamp(0, 1)
        if output_type == "pt":
            return image
        arr = image.cpu().permute(0, 2, 3, 1).numpy()
        if output_type == "np":
            return arr
        from PIL import Image

        return [Image.fromarray((a * 255).round().astype("uint8")) for a in arr]

    # ---- one denoise step of the three networks ----------------------------------------------------------
    # ---- on-device sampling loop -------------------------------------------------------------
    def _fusable(self, scheds, device, cond_scale, callback, eta: float = 0.0) -> bool:
        """The fused loop covers what eval needs: a scheduler with a device plan (``schedulers.device_plan``: this package's
        DDIM with any eta, UniPC, DDPM, DPM-Solver++; x0 prediction) on every latent group with one common schedule and
        configuration, with or without classifier-free guidance, no per-step callback, HIP graph on.  Anything else takes the
        step-by-step loop (identical results: tests/test_pipeline_gpu.py)."""
        if not (self.use_fused_sampler and self.use_hip_graph and torch.device(device).type == "cuda"):
            return False
        if callback is not None:
            return False
        s0, p0 = scheds[0], device_plan(scheds[0], eta)
        if p0 is None:
            return False
        own_final = hasattr(s0, "final_alpha_cumprod")  # DDIM: the schedule is its tensors; the others': their configuration
        for s in scheds:
            plan = device_plan(s, eta)
            if plan is None or plan.kind != p0.kind or s.prediction_type != "sample":
                return False
            if s.num_inference_steps != s0.num_inference_steps or not torch.equal(s.timesteps.cpu(), s0.timesteps.cpu()):
                return False
            if not torch.equal(s.alphas_cumprod, s0.alphas_cumprod):
                return False
            if own_final and float(s.final_alpha_cumprod) != float(s0.final_alpha_cumprod):
                return False
            if not own_final and s.config != s0.config:
                return False
        return True

    # ---- stochastic samplers (DDIM with eta, DDPM, SDE-DPM-Solver++) --------------------------------------------------
    def _draw_seed(self, scheds, eta: float, generator) -> Optional[int]:
        """ONE int64 per sampling call that keys the noise of every step (``ur_sde_update``, ``ops.sampler_noise``,
        ``schedulers.philox_normal``), drawn from ``generator`` (the global generator if None) -- the package's own stream, not
        ``torch.randn``'s: the same ``manual_seed`` gives the same images, a second call on the same generator object other
        ones.  None, and nothing drawn, when no scheduler of the call has a noise term (a foreign scheduler has none here)."""
        plans = [device_plan(s, eta) for s in scheds]
        if not any(p is not None and p.noisy for p in plans):
            return None
        if isinstance(generator, (list, tuple)):
            generator = generator[0]
        return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, dtype=torch.int64,
                                 device=generator.device if generator is not None else "cpu"))

    @staticmethod
    def _step_noise(seed: Optional[int], seed_dev, i: int, shape, device):
        """The noise of step ``i`` of the step-by-step loops for the whole evolving latent of ``shape`` (what the fused loop's
        kernel draws for the same elements), or None for a call without a noise term."""
        if seed is None:
            return None
        if torch.device(device).type == "cuda":
            return ops.sampler_noise(seed_dev, i, shape)
        from .schedulers import philox_normal

        return philox_normal(seed, i, shape).to(device)

    def _graph_key(self, x_img, ehs, run_decoder, cond_scale: float = 1.0):
        """Everything a captured step bakes in besides the weights: shapes, dtype, executor, conditioning scale, the
        UNet's FreeU factors (kernel arguments of ``ur_freeu``) and its IP-Adapter (identity, token count, scale: launches and
        kernel arguments of ``ur_ip_attention_add``)."""
        B, _, h, w = x_img.shape
        return (str(x_img.device), B, h, w, ehs.shape[1], ehs.shape[2], run_decoder, self.unet.dtype, float(cond_scale),
                self.hoist_invariants, self.rerun_invariants, freeu_state(self.unet), self.unet.ip_adapter_state())

    def _graph_for(self, x_img, cond28, ehs, run_decoder, cond_scale: float = 1.0, sig=None):
        """The captured step for these shapes / this conditioning scale, re-captured when the weights it baked in have
        changed since (``sig`` = a ``_weights_signature()`` the caller took once for its whole sampling call)."""
        B, _, h, w = x_img.shape
        dt = self.unet.dtype
        key = self._graph_key(x_img, ehs, run_decoder, cond_scale)
        sig = sig if sig is not None else self._weights_signature()
        g = self._graphs.get(key)
        if g is not None and g.weights_sig != sig:  # stale packed weights: drop it and every sampling graph built on it
            del self._graphs[key]
            for k in [k for k in self._sample_graphs if k[:len(key)] == key]:
                del self._sample_graphs[k]
            g = None
        if g is None:
            kw = dict(dtype=dt, device=x_img.device, run_decoder=run_decoder, cond_channels=cond28.shape[1],
                      img_channels=x_img.shape[1], ctx_len=ehs.shape[1], conditioning_scale=cond_scale)
            if self.hoist_invariants:
                g = GraphedHoistedStep(self.unet, self.controlnet, self.controldec, B, (h, w), ehs.shape[2],
                                       hoist=not self.rerun_invariants, **kw)
            else:
                g = GraphedDualStreamStep(self.unet, self.controlnet, self.controldec, B, (h, w), ehs.shape[2], **kw)
            g.load_inputs(x_img, cond28, ehs, 0, 0)
            g.capture()
            g.weights_sig = sig
            self._graphs[key] = g
        return key, g

    def _fused_loop(self, x_img, cond28, ehs, timesteps, sched, run_decoder: bool, lat_dtype=torch.float32,
                    guidance: Optional[float] = None, cond_scale: float = 1.0, eta: float = 0.0, seed: Optional[int] = None,
                    views: Optional[ViewGeometry] = None):
        """All denoise steps as replays of ONE graph = step + ur_ddim_update (prediction -> next input, in the
        graph's static input buffer) + ur_sampler_advance (step counter, next timestep).  UniPC: ur_unipc_update.  DDIM
        with eta != 0, DDPM, (SDE-)DPM-Solver++: ur_sde_update, whose noise is keyed by ``seed``, written into a device
        buffer before the replays (the graph knows the buffer, not the value).  Inverse direction: the 24
        attribute channels of ``cond`` evolve at t_attr, the image latent is clean (t_img = 0); rendering direction:
        the 4 image channels of ``x_t`` evolve at t_img, the attributes are clean.  ``guidance``: classifier-free
        guidance -- the inputs hold cond + uncond halves (2B samples); the inverse direction guides the material group
        only (pipeline.py:2695-2721), the rendering direction the whole image prediction (1642-1644).
        ``views`` (MultiDiffusion): the batch is N * V views; ``ops.view_blend`` follows the update inside the graph, whose key
        then holds the geometry (the launch bakes it in), and the result is the GLOBAL latent [N, C, H, W]."""
        n = len(timesteps)
        cfg = guidance is not None
        nb = x_img.shape[0] // 2 if cfg else x_img.shape[0]  # distinct latents
        key, g = self._graph_for(x_img, cond28, ehs, run_decoder, cond_scale)
        t0 = float(timesteps[0])
        g.load_inputs(x_img, cond28, ehs, 0.0 if run_decoder else t0, t0 if run_decoder else 0.0)
        plan = device_plan(sched, eta)
        skey = key + (() if views is None else (("views",) + tuple(views),)) + (n, lat_dtype, guidance, self.precompute_time_tables, plan.kind)
        st = self._sample_graphs.get(skey)
        if st is None:
            dev = x_img.device
            evolving = g.cond[:, 4:] if run_decoder else g.x_t
            mshape = (nb,) + tuple(evolving.shape[1:])
            sampler = _SamplerState(plan.kind, n, plan.coef.shape[1])
            sampler.allocate(mshape, dev, round_master=lat_dtype != torch.float32)
            st = dict(sampler=sampler)
            if views is not None:  # the blended global latent (ur_view_blend writes it on every step)
                st["global"] = torch.zeros((nb // views.num_views, mshape[1], views.height, views.width), dtype=torch.float32, device=dev)

            def update(pred_nhwc, c0, lat, cfg_channels):
                sampler.update(pred_nhwc, c0, lat, guidance, cfg_channels)
                if views is not None:  # every view <- the mean of the views that cover each of its pixels
                    ops.view_blend(sampler.master, lat, st["global"], views, halves=2 if cfg else 1, round_master=sampler.round_master)

            def post(out):
                if run_decoder:  # the material group is channels 4..7 of the 28
                    update(out["attr_pred"].permute(0, 2, 3, 1), 4, g.cond[:, 4:], 4)
                    ops.sampler_advance(sampler.step, sampler.tvals, n, g.t_attr)
                else:
                    update(out["img_pred"].permute(0, 2, 3, 1), 0, g.x_t, g.x_t.shape[1])
                    ops.sampler_advance(sampler.step, sampler.tvals, n, g.t_img)

            if isinstance(g, GraphedHoistedStep) and self.precompute_time_tables:
                # the time projections of all n steps once per call (they depend on the timestep only); the step graph picks
                # its rows with the device-side step counter
                st["tgraph"], (tab1, tab3) = g.capture_time_tables(sampler.tvals)
                st["graph"], st["out"] = g.capture_with(post, tables=(tab1, tab3, sampler.step))
            else:
                st["graph"], st["out"] = g.capture_with(post)
            self._sample_graphs[skey] = st
            g.load_inputs(x_img, cond28, ehs, 0.0 if run_decoder else t0, t0 if run_decoder else 0.0)  # capture ran no kernel, but be explicit
        sampler = st["sampler"]
        sampler.reset((cond28[:nb, 4:] if run_decoder else x_img[:nb]), seed, plan)  # the caller's latents at their own precision
        hoisted = isinstance(g, GraphedHoistedStep)
        if st.get("tgraph") is not None:
            st["tgraph"].replay()  # time projections of every step of this call (the reset above wrote its timesteps)
        if hoisted:
            g.begin()  # the loop-invariant half, once per call
        for _ in range(n):
            if hoisted and not g.hoist:
                g.pro.replay()
            st["graph"].replay()
        # a COPY: ``master`` is this sampling graph's static buffer and the next call with the same shapes overwrites it
        return (sampler.master if views is None else st["global"]).to(lat_dtype, copy=True)

    def _step(self, x_img, cond28, ehs, t_img, t_attr, run_decoder: bool, cond_scale: float = 1.0, sig=None, first: bool = True):
        """One step of a sampling loop.  ``first``: the first step of a loop (the hoisted executor runs its prologue on the
        loop-invariant inputs then and only reloads the evolving latent afterwards).  The inverse loops' ``img_pred`` is not
        computed by the hoisted executor (the reference drops it, 2670)."""
        dt = self.unet.dtype
        if self.use_hip_graph and x_img.is_cuda:
            _, g = self._graph_for(x_img, cond28, ehs, run_decoder, cond_scale, sig=sig)
            if isinstance(g, GraphedHoistedStep):
                return g.step(x_img, cond28, ehs, t_img, t_attr, first=first)
            return g.step(x_img, cond28, ehs, t_img, t_attr)
        tb = lambda t: torch.as_tensor(t, device=x_img.device).float().reshape(-1)
        return dual_stream_step(self.unet, self.controlnet, self.controldec, x_img.to(dt), cond28.to(dt), ehs.to(dt),
                                tb(t_img), tb(t_attr), run_decoder, conditioning_scale=cond_scale)

    def _step_chunked(self, chunks, fixed, x_img, cond28, ehs, t_img, t_attr, run_decoder: bool, **kw):
        """``_step`` over the batch rows ``chunks[k]`` in turn (``view_batch_size``); the prediction the loop reads, assembled
        for the whole batch.  ``fixed``: a dict the loop keeps for its call -- every chunk's fixed inputs are cut ONCE, so that the
        hoisted executor sees one object per chunk (a chunk's prologue still re-runs when the previous call was another chunk's)."""
        name = "attr_pred" if run_decoder else "img_pred"
        full = None
        for k, idx in enumerate(chunks):
            if k not in fixed:
                fixed[k] = ((x_img if run_decoder else cond28)[idx], ehs[idx])
            if run_decoder:
                (xi, e), ci = fixed[k], cond28[idx]
            else:
                (ci, e), xi = fixed[k], x_img[idx]
            o = self._step(xi, ci, e, t_img, t_attr, run_decoder, **kw)[name]
            if full is None:
                full = torch.empty((x_img.shape[0],) + tuple(o.shape[1:]), dtype=o.dtype, device=o.device)
            full[idx] = o  # the executor's output buffer is static: copy before the next chunk runs
        return {name: full}

    def _sample(self, *, fixed, lat, scheds, guided, input_sched, run_decoder: bool, timesteps, num_inference_steps,
                prompt_embeds, geo, cond_scale: float, eta: float, generator, callback=None):
        """The sampling loop of both directions.  ``fixed``: the clean inputs as global tensors -- inverse (``run_decoder``): the
        image and mask latents, whose timestep is the constant 0; rendering: the 28 attribute channels.  ``lat``: the evolving
        latent groups (global, initial noise), ``scheds`` their schedulers, ``guided`` which of them classifier-free guidance
        combines (the others keep the cond half; inverse: ``material`` only, ref 2697-2721; rendering: the image, ref
        1642-1644).  ``input_sched`` scales the evolving input of every step; the on-device loop needs it and ``scheds`` on one
        common schedule.  Returns the final groups (global under MultiDiffusion ``geo``)."""
        device, cfg = prompt_embeds.device, self.do_classifier_free_guidance
        widths = [t.shape[1] for t in lat]
        cat = lambda parts: torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
        glob = None
        if geo is not None:  # the global tensors are cut into views ONCE per call; view v of sample n is batch row n * V + v
            glob = cat(lat).float()
            fixed, lat = [gather_views(t, geo) for t in fixed], [gather_views(t, geo) for t in lat]
            prompt_embeds = prompt_embeds.repeat_interleave(geo.num_views, dim=0)
        dup = (lambda t: torch.cat([t, t])) if cfg else (lambda t: t)
        fixed = [dup(self.scheduler_img.scale_model_input(t, 0)) for t in fixed]

        def inputs(x):  # (x_img, cond28) of a step: inverse = mask latent first, 4 + 6*4 = 28 channels
            return (fixed[0], torch.cat((fixed[1].to(x.dtype), x), dim=1)) if run_decoder else (x, fixed[0])

        seed = self._draw_seed(scheds, eta, generator)  # after the initial latents, in both loops: same generator state
        with self.progress_bar(total=num_inference_steps) as bar:
            if self._fusable([input_sched] + scheds, device, cond_scale, callback, eta):
                x = cat([dup(t) for t in lat])
                fin = self._fused_loop(*inputs(x), prompt_embeds, timesteps, scheds[0], run_decoder=run_decoder, lat_dtype=x.dtype,
                                       guidance=(float(self.guidance_scale) if cfg else None), cond_scale=cond_scale, eta=eta,
                                       seed=seed, views=geo)
                return [f.to(t.dtype) for f, t in zip(fin.split(widths, dim=1), lat)]  # ``fin`` is the global latent already
            sig = self._weights_signature()  # once per call, not per step
            seed_dev = torch.tensor([seed], dtype=torch.int64, device=device) if seed is not None else None
            chunks, chunk_fixed = (self._view_chunks(lat[0].shape[0], cfg, device) if geo is not None else None), {}
            plans = [device_plan(s, eta) for s in scheds]
            # the clean side's timestep is the constant 0 (ref 2476 / 1455): hand the hoisted executor the SAME tensor object on
            # every step -- it re-runs its prologue when a fixed input changes identity (graph.GraphedHoistedStep.step)
            t_zero = torch.zeros_like(timesteps)[0] if len(timesteps) else None
            for i, t in enumerate(timesteps):
                x_img, cond28 = inputs(input_sched.scale_model_input(cat([dup(v) for v in lat]), t))
                t_img, t_attr = (t_zero, t) if run_decoder else (t, t_zero)
                if chunks is None:
                    out = self._step(x_img, cond28, prompt_embeds, t_img, t_attr, run_decoder=run_decoder, cond_scale=cond_scale,
                                     sig=sig, first=(i == 0))
                else:
                    out = self._step_chunked(chunks, chunk_fixed, x_img, cond28, prompt_embeds, t_img, t_attr,
                                             run_decoder=run_decoder, cond_scale=cond_scale, sig=sig, first=(i == 0))
                preds = (out["attr_pred"][:, 4:] if run_decoder else out["img_pred"]).split(widths, dim=1)  # drop the mask group (ref 2691)
                # the groups are ONE latent to the noise stream, as in the fused loop (MultiDiffusion: over the [N * V, ...] view
                # batch, so overlapping views draw independent noise)
                noise = self._step_noise(seed, seed_dev, i, (lat[0].shape[0], sum(widths)) + tuple(lat[0].shape[2:]), device)
                noises = [None] * len(lat) if noise is None else noise.split(widths, dim=1)
                for k, (pred, sch, plan) in enumerate(zip(preds, scheds, plans)):
                    if cfg:
                        p_cond, p_uncond = pred.chunk(2)  # chunk order exactly as the reference reads it
                        pred = p_uncond + self.guidance_scale * (p_cond - p_uncond) if guided[k] else p_cond
                    kw_step = plan.step_kwargs(eta, noises[k]) if plan is not None else {}
                    lat[k] = sch.step(pred, t, lat[k], return_dict=False, **kw_step)[0]
                if geo is not None:  # where the fused loop's graph has ur_view_blend
                    lat, glob = self._blend_views(lat, geo)
                if callback is not None:
                    callback(self, i, t, {"latents": lat[0]})
                bar.update()
        if glob is not None:  # the step-by-step MultiDiffusion loop: the results are the global latents
            lat = [g_.to(t.dtype) for g_, t in zip(glob.split(widths, dim=1), lat)]
        return lat

    # =====================================================================================================
    @torch.no_grad()
    def real_image2mask_3mod_albedo(
        self, prompt: Union[str, List[str]] = None, image=None, masks=None, height: Optional[int] = None,
        width: Optional[int] = None, num_inference_steps: int = 50, timesteps: List[int] = None,
        guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0,
        generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None, ip_adapter_image=None,
        output_type: Optional[str] = "pil", return_dict: bool = True, cross_attention_kwargs=None,
        controlnet_conditioning_scale: Union[float, List[float]] = 1.0, guess_mode: bool = False,
        control_guidance_start=0.0, control_guidance_end=1.0, clip_skip=None, callback_on_step_end=None,
        callback_on_step_end_tensor_inputs: List[str] = ["latents"], image_latents=None, mask_latents=None, **kwargs,
    ):
        """Inverse rendering: image (+ mask) -> material / normal / albedo / specular / diffuse / environment.
        Returns ``(material_latents, normal, albedo, spec_light, diff_light, env)`` like the reference (2808).
        ``image_latents`` / ``mask_latents`` (already VAE-encoded, scaled) bypass the VAE; ``output_type="latent"``
        returns the six latents instead of decoded images.  ``eta`` is DDIM's (other schedulers ignore it, as in the
        reference's ``prepare_extra_step_kwargs``).  A sampler with a noise term (DDIM with eta != 0, DDPM, SDE-DPM-Solver++)
        draws ONE int64 from ``generator`` per call and takes all its noise from the package's own counter-based stream
        keyed by it (``_draw_seed``) -- reproducible under ``manual_seed``, not ``torch.randn``'s numbers.
        ``ip_adapter_image`` (PIL / array through ``feature_extractor``, or a pixel tensor): the image prompt of a loaded
        IP-Adapter (``load_ip_adapter``), encoded by ``image_encoder`` and folded with ``num_images_per_prompt``; it goes to
        the UNet only, under classifier-free guidance as ``[zeros ; embeds]``."""
        self._guidance_scale = guidance_scale
        self.unet._lora_apply(scale_of(cross_attention_kwargs))  # before any _weights_signature(): graphs see merged weights
        device = self._execution_device
        batch_size = 1 if isinstance(prompt, str) else (len(prompt) if prompt is not None else prompt_embeds.shape[0])
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, num_images_per_prompt, self.do_classifier_free_guidance, negative_prompt,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
        timesteps_attr, num_inference_steps = retrieve_timesteps(self.scheduler_attr, num_inference_steps, device)
        for n in ATTR_GROUPS:
            retrieve_timesteps(getattr(self, f"scheduler_{n}"), num_inference_steps, device)
        self._num_timesteps = len(timesteps_attr)  # the image latent is clean: t_img = 0 (ref 2476)

        if image_latents is None:
            if not torch.is_tensor(image):
                image = self.prepare_image(image, width, height, batch_size * num_images_per_prompt, num_images_per_prompt,
                                           device, self.controlnet.dtype)
                masks = self.prepare_image(masks, width, height, batch_size * num_images_per_prompt, num_images_per_prompt,
                                           device, self.controlnet.dtype)
            else:  # ref 2504-2507
                batch_size = image.shape[0]
            image_latents, mask_latents = self._vae_encode(image), self._vae_encode(masks)
        else:
            batch_size = image_latents.shape[0]
        # Repeat folding: eval/test_real.py:547-564 calls this method ``compute_times`` = 5 times on the
        # same image and averages; ``num_images_per_prompt=5`` is the same protocol as ONE batch of 5 (the reference's
        # prepare_image repeats the image batch_size * num_images_per_prompt times, ref 2504-2523, and every attribute
        # group draws batch_size * num_images_per_prompt noise latents, 2540-2609): 5x fewer loop launches.
        total = batch_size * num_images_per_prompt
        if image_latents.shape[0] != total:
            if image_latents.shape[0] * num_images_per_prompt != total:
                raise ValueError("image batch does not match batch_size * num_images_per_prompt")
            image_latents = image_latents.repeat_interleave(num_images_per_prompt, dim=0)
            mask_latents = mask_latents.repeat_interleave(num_images_per_prompt, dim=0)
        prompt_embeds = self._batch_prompt(prompt_embeds, negative_prompt_embeds, total)
        h8, w8 = image_latents.shape[-2:]
        geo = self._view_geometry(h8, w8)  # MultiDiffusion: None unless enabled and the latent is larger than the window
        self._prepare_ip_adapter(ip_adapter_image, device, total, num_images_per_prompt, views=geo.num_views if geo else 1)
        height, width = height or h8 * self.vae_scale_factor, width or w8 * self.vae_scale_factor
        nlat = self.unet.config.in_channels
        lat = {n: self.prepare_latents(total, nlat, height, width, prompt_embeds.dtype,
                                       device, generator, latents) for n in ATTR_GROUPS}
        fin = self._sample(fixed=[image_latents, mask_latents], lat=[lat[n] for n in ATTR_GROUPS],
                           scheds=[getattr(self, f"scheduler_{n}") for n in ATTR_GROUPS],
                           guided=[n == "material" for n in ATTR_GROUPS], input_sched=self.scheduler_attr, run_decoder=True,
                           timesteps=timesteps_attr, num_inference_steps=num_inference_steps, prompt_embeds=prompt_embeds, geo=geo,
                           cond_scale=float(controlnet_conditioning_scale), eta=float(eta), generator=generator,
                           callback=callback_on_step_end)
        lat = dict(zip(ATTR_GROUPS, fin))
        if output_type == "latent":
            return tuple(lat[n] for n in ATTR_GROUPS)
        # the five image groups (ref 2755-2769: five vae.decode calls) decoded as ONE batch
        dec = self._vae_decode(torch.cat([lat[n] for n in ATTR_GROUPS[1:]], dim=0), generator).chunk(len(ATTR_GROUPS) - 1, dim=0)
        imgs = [self._postprocess(d, output_type) for d in dec]
        return (lat["material"], *imgs)

    @torch.no_grad()
    def image2mask_3mod_albedo(self, prompt=None, image: torch.Tensor = None, masks: torch.Tensor = None, **kwargs):
        """Dataset-evaluation variant (ref 1990-2390): tensor inputs in [0, 1] are normalised to [-1, 1] first."""
        if image is not None:
            image = image * 2.0 - 1.0
        if masks is not None:
            masks = masks * 2.0 - 1.0
        return self.real_image2mask_3mod_albedo(prompt=prompt, image=image, masks=masks, **kwargs)

    @torch.no_grad()
    def mask2image_3mod_albedo(
        self, prompt=None, masks_image=None, material_num=None, normal_image=None, albedo_image=None,
        spec_light_image=None, diff_light_image=None, env_image=None, height: Optional[int] = None,
        width: Optional[int] = None, num_inference_steps: int = 50, timesteps=None, guidance_scale: float = 7.5,
        negative_prompt=None, num_images_per_prompt: Optional[int] = 1, eta: float = 0.0, generator=None, latents=None,
        prompt_embeds=None, negative_prompt_embeds=None, output_type: Optional[str] = "pil", return_dict: bool = True,
        cross_attention_kwargs=None, controlnet_conditioning_scale: float = 1.0, guess_mode: bool = False,
        attr_latents: Optional[torch.Tensor] = None, ip_adapter_image=None, **kwargs,
    ):
        """Rendering: attributes -> image (enc + unet per step; the decoder is not run, ref 1631-1639).
        ``attr_latents`` ([B,28,h,w], mask first) bypasses the VAE encodes of the seven attribute images.  ``eta`` /
        ``generator`` / ``ip_adapter_image``: as in ``real_image2mask_3mod_albedo``."""
        self._guidance_scale = guidance_scale
        self.unet._lora_apply(scale_of(cross_attention_kwargs))  # before any _weights_signature(): graphs see merged weights
        device = self._execution_device
        batch_size = 1 if isinstance(prompt, str) else (len(prompt) if prompt is not None else prompt_embeds.shape[0])
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, num_images_per_prompt, self.do_classifier_free_guidance, negative_prompt,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds)
        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler_img, num_inference_steps, device)
        self._num_timesteps = len(timesteps)  # the attributes are clean: t_attr = 0 (ref 1455)
        if attr_latents is None:
            bs = batch_size * num_images_per_prompt
            prep = lambda im: self.prepare_image(im, width, height, bs, num_images_per_prompt, device, self.controlnet.dtype)
            l_normal = self._vae_encode(prep(normal_image))
            m = torch.as_tensor(material_num, device=l_normal.device, dtype=l_normal.dtype)
            metallic = torch.zeros_like(l_normal[:, :2]) + m[0]
            rough = torch.zeros_like(l_normal[:, :2]) + m[1]
            l_material = torch.cat((metallic, rough), dim=1) * 2 - 1.0  # constant 2+2 channels (ref 1534-1541)
            parts = [self._vae_encode(prep(masks_image)), l_material, l_normal, self._vae_encode(prep(albedo_image)),
                     self._vae_encode(prep(spec_light_image)), self._vae_encode(prep(diff_light_image)),
                     self._vae_encode(prep(env_image))]
            attr_latents = torch.cat(parts, dim=1)
        batch_size = attr_latents.shape[0]
        prompt_embeds = self._batch_prompt(prompt_embeds, negative_prompt_embeds, batch_size)
        h8, w8 = attr_latents.shape[-2:]
        geo = self._view_geometry(h8, w8)  # MultiDiffusion (see real_image2mask_3mod_albedo)
        self._prepare_ip_adapter(ip_adapter_image, device, batch_size, num_images_per_prompt, views=geo.num_views if geo else 1)
        height, width = height or h8 * self.vae_scale_factor, width or w8 * self.vae_scale_factor
        latents_img = self.prepare_latents(batch_size, 4, height, width, prompt_embeds.dtype, device, generator, latents)
        (latents_img,) = self._sample(fixed=[attr_latents], lat=[latents_img], scheds=[self.scheduler_img], guided=[True],
                                      input_sched=self.scheduler_img, run_decoder=False, timesteps=timesteps,
                                      num_inference_steps=num_inference_steps, prompt_embeds=prompt_embeds, geo=geo,
                                      cond_scale=float(controlnet_conditioning_scale), eta=float(eta), generator=generator)
        if output_type == "latent":
            return latents_img
        return self._postprocess(self._vae_decode(latents_img, generator), output_type)


class _NullBar:
    def update(self, *_):
        return None
