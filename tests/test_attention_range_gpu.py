"""csrc/attention.hip and csrc/attention_bwd.hip against float64, per (batch, head, row), on the data the kernels'
hand-built numerics exist for.  The other suites assert one rel-L2 over the whole output against an fp32 SDPA on N(0, 1)
operands: a flat softmax, in which the lazy rescale (a wave-uniform decision for 32 queries), the reference slot of the
d = 40 kernel, the row sums taken from the MFMA, a sink on the last valid key of a ragged tile or one wrong row of 1024
never show.  Here every case is built by util_attention.make_case (families: see FAMILIES there), evaluated in float64 on
exactly the stored operands, and every row is held to the element-wise bounds derived in util_attention's docstring
(|o - ref| <= 3 u A; lse within 2 u + 2^-22 |ref|; dv / dq / dk within their 4 u / 5 u + 2 u forms) plus the suites'
rel-L2 tolerances per row.  test_attention_bounds_cpu.py shows that correct arithmetic meets these bounds with room and that
they reject the single-row errors the old assertion accepts.

All shapes are inside what ur_attention accepts; nothing here is meant to make a launch fail.
"""
import pytest
import torch

import util_attention as ua

pytestmark = pytest.mark.gpu

DTYPES = ua.DTYPES
B, H = 2, 3  # H odd: head offsets are not powers of two
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None

# (id, head dim, pre-scaled): every instantiation launch_attn_d reaches
KERNELS = [("a32_d32_scaled", 32, False), ("a32_d40_scaled", 40, False), ("a32_d64_scaled", 64, False),
           ("a32_d32_prescaled", 32, True), ("a32_d64_prescaled", 64, True), ("slot_d40_prescaled", 40, True),
           ("a16_d80_scaled", 80, False), ("a16_d80_prescaled", 80, True), ("a16_d128_scaled", 128, False),
           ("a16_d128_prescaled", 128, True), ("a16_d160_scaled", 160, False), ("a16_d160_prescaled", 160, True)]
KID = [k[0] for k in KERNELS]
THREE = [KERNELS[5], KERNELS[0], KERNELS[6]]  # the slot kernel, the 32x32 kernel without slot, one attention_kernel head dim


def _tok(x):
    """[B, H, T, d] -> token matrix [B, T, H*d]."""
    b, h, t, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, t, h * d)


def _vt(v, dtype, dev, wide=False):
    """V^T [B, H*d, Tk_pad] with zero columns >= Tk (the contract of ops.vt_proj); ``wide``: rows C .. 2C of a
    [B, 3C, Tk_pad] projection whose other rows hold NaN (vt_bstride = 3 samples' worth)."""
    b, h, tk, d = v.shape
    C, tp = h * d, (tk + 63) // 64 * 64
    big = torch.full((b, 3 * C if wide else C, tp), float("nan") if wide else 0.0, dtype=torch.float64)
    r0 = C if wide else 0
    big[:, r0:r0 + C] = 0.0
    big[:, r0:r0 + C, :tk] = _tok(v).transpose(1, 2)
    return big.to(dtype).to(dev)[:, r0:r0 + C]


def _embed(x, ld, off, dtype, dev):
    """token matrix as columns off .. off + C of a [B, T, ld] matrix; every other column holds NaN."""
    b, t, C = x.shape
    m = torch.full((b, t, ld), float("nan"), dtype=torch.float64)
    m[..., off:off + C] = x
    return m.to(dtype).to(dev)


def _forward(case, dev, layout="separate", want_lse=False):
    """-> (o [B, H, Tq, d] float64 on the CPU, lse [B, H, Tq] float64 or None, the raw output tensor)."""
    from uni_renderer_amd import ops
    q, k, v, dt = case["q"], case["k"], case["v"], case["dtype"]
    b, h, tq, d = q.shape
    tk, C = k.shape[2], h * d
    kw = dict(B=b, H=h, Tq=tq, Tk=tk, d=d, scale=0.0 if case["prescaled"] else None)
    vt = _vt(v, dt, dev, wide=layout == "wide")
    if layout == "separate":
        qd, kd = _tok(q).to(dt).to(dev), _tok(k).to(dt).to(dev)
        kw.update(ldq=C, ldk=C)
    elif layout == "fused_qk":          # the self-attention projection: q | k in one matrix
        qd = kd = torch.cat([_tok(q), _tok(k)], -1).to(dt).to(dev)
        kw.update(ldq=2 * C, ldk=2 * C, q_off=0, k_off=C)
    elif layout == "wide":              # column ranges of wider matrices, NaN outside what the descriptor names
        qd, kd = _embed(_tok(q), C + 24, 8, dt, dev), _embed(_tok(k), 2 * C + 16, C + 8, dt, dev)
        kw.update(ldq=C + 24, ldk=2 * C + 16, q_off=8, k_off=C + 8)
    else:                               # head-major images [B, H, T, d]: hm_q, hm_k, hm_qk
        hq, hk = layout in ("hm_q", "hm_qk"), layout in ("hm_k", "hm_qk")
        qd = (q.contiguous() if hq else _tok(q)).to(dt).to(dev)
        kd = (k.contiguous() if hk else _tok(k)).to(dt).to(dev)
        kw.update(ldq=C, ldk=C, q_hstride=tq * d if hq else 0, k_hstride=tk * d if hk else 0)
    lse = None
    if want_lse:
        lse = torch.full((b * h * tq + 37,), float("nan"), dtype=torch.float32, device=dev)
        kw["lse"] = lse
    o = ops.attention(qd, kd, vt, **kw)
    torch.cuda.synchronize()
    if want_lse:
        lse = lse.cpu()
        assert torch.isnan(lse[b * h * tq:]).all(), "the kernel wrote past the B*H*Tq entries of lse"
        lse = lse[:b * h * tq].double().view(b, h, tq)
    return ua.heads(o, h), lse, o


def _check_forward(case, dev, layout, what):
    want_lse = not case["prescaled"]
    o, lse, _ = _forward(case, dev, layout, want_lse)
    ref, A, lse_ref = ua.forward_ref(case)
    figs = ua.check_forward(o, ref, A, case["dtype"], what)
    if want_lse:
        figs += (ua.check_lse(lse, lse_ref, case["dtype"], what),)
    print({"case": what, "worst_row_rel_l2": figs[0], "worst_err_over_bound": figs[1], "lse_over_bound": figs[2:]})


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("layout", ["separate", "fused_qk", "wide"])
@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_forward_kernels_and_layouts(dev, dtype, layout, kernel):
    """Every kernel instantiation (head dim 128 included) on separate q / k / v, on q | k fused in one matrix, and on
    q, k as column slices of wider matrices with V^T as a row slice of a wider batched projection (what the
    cross-attention passes); ragged query and key tiles."""
    name, d, pre = kernel
    tq, tk = (129, 129) if layout == "fused_qk" else (129, 77)
    case = ua.make_case("peaky", B, H, tq, tk, d, dtype, prescaled=pre, seed=11)
    _check_forward(case, dev, layout, f"{name} {layout} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("size", [(129, 77), (256, 333)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pre", [False, True], ids=["scaled", "prescaled"])
@pytest.mark.parametrize("layout", ["hm_q", "hm_k", "hm_qk"])
@pytest.mark.parametrize("d", [32, 40, 64])
def test_forward_head_major(dev, dtype, size, pre, layout, d):
    """Head-major q / k images against the reference (not only bit-for-bit through the chain kernels), with
    Tk % 64 != 0 and Tq % 128 != 0, at all three head dims of the 32x32 kernel."""
    case = ua.make_case("peaky", B, H, size[0], size[1], d, dtype, prescaled=pre, seed=12)
    _check_forward(case, dev, layout, f"d{d} {layout} {size} prescaled={pre} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tk", [1, 63, 64, 65, 77, 127, 333])
@pytest.mark.parametrize("tq", [1, 31, 129, 256])
@pytest.mark.parametrize("kernel", THREE, ids=[k[0] for k in THREE])
def test_forward_sizes(dev, dtype, tk, tq, kernel):
    name, d, pre = kernel
    case = ua.make_case("peaky", B, H, tq, tk, d, dtype, prescaled=pre, seed=13)
    _check_forward(case, dev, "separate", f"{name} {tq}x{tk} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tk", [77, 256, 333])
@pytest.mark.parametrize("kernel", THREE, ids=[k[0] for k in THREE])
@pytest.mark.parametrize("family", ua.FAMILIES)
def test_forward_families(dev, dtype, tk, kernel, family):
    """Every score / value family on the slot kernel, the 32x32 kernel without slot and attention_kernel, with a ragged
    2-tile, a full 4-tile and a ragged 6-tile key count; 160 queries = one full workgroup and a ragged one, so the
    mixed-row families put their odd query into 5 different waves."""
    name, d, pre = kernel
    case = ua.make_case(family, B, H, 160, tk, d, dtype, prescaled=pre, seed=14)
    _check_forward(case, dev, "separate", f"{family} {name} Tk {tk} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("pre", [False, True], ids=["scaled", "prescaled"])
@pytest.mark.parametrize("d", [32, 40, 64, 80])
def test_forward_layout_poison_bitwise(dev, dtype, pre, d):
    """q and k as column ranges of wider matrices (ldq, ldk > H*d, non-zero offsets), V^T as a row range, NaN in every
    element the descriptor does not name: bitwise equal to the run on compact copies.  For d = 40 this pins that the
    16-byte chunk after a head's 40 columns is never taken from memory (the last head's would be NaN)."""
    case = ua.make_case("peaky", B, H, 129, 77, d, dtype, prescaled=pre, seed=15)
    _, _, compact = _forward(case, dev, "separate")
    _, _, wide = _forward(case, dev, "wide")
    assert torch.isfinite(wide.float()).all()
    assert torch.equal(compact, wide)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_forward_product_size(dev, dtype):
    """The launch that dominates the step: B = 1, H = 8, d = 40, T = 4096, pre-scaled scores (slot kernel), head-major q / k."""
    case = ua.make_case("peaky", 1, 8, 4096, 4096, 40, dtype, prescaled=True, seed=16)
    _check_forward(case, dev, "hm_qk", f"product size {dtype}")


def test_lse_needs_a_scale(dev):
    from uni_renderer_amd import ops
    case = ua.make_case("flat", 1, 2, 64, 64, 40, torch.float16, prescaled=True, seed=17)
    q, k = _tok(case["q"]).half().to(dev), _tok(case["k"]).half().to(dev)
    lse = torch.full((2 * 64,), float("nan"), dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        ops.attention(q, k, _vt(case["v"], torch.float16, dev), B=1, H=2, Tq=64, Tk=64, d=40, ldq=80, ldk=80, scale=0.0, lse=lse)
    torch.cuda.synchronize()
    assert torch.isnan(lse).all()


# ---------------------------------------------------------------------------------------------------------------
# backward
_cache = {}


def _bwd_case(family, tq, tk, d, dtype, materialised=False):
    key = (family, tq, tk, d, dtype, materialised)
    if _cache.get("key") != key:  # the path parameter varies fastest: one reference serves its cases
        case = ua.make_case(family, B, H, tq, tk, d, dtype, seed=21)
        _cache.update(key=key, case=case, ref=ua.backward_ref(case, materialised=materialised), fwd=ua.forward_ref(case))
    return _cache["case"], _cache["ref"], _cache["fwd"]


PATHS = [("fwd_lse", 0), ("fwd_lse", 1000), ("own_lse", 0), ("own_lse", 1000), ("fused_qkv", 0), ("fused_qkv", 1000)]
PID = [f"{p}-direct{m}" for p, m in PATHS]


def _flash(case, path, dev):
    """forward (with its lse) + ur_attention_backward -> dict of [B, H, T, d] float64, lse [B, H, Tq]."""
    from uni_renderer_amd import backward as bw, ops
    dt = case["dtype"]
    q, k, v, do = (_tok(case[n]).to(dt).to(dev) for n in ("q", "k", "v", "do"))
    b, tq, C = q.shape
    tk, d = k.shape[1], C // H
    assert bw.FLASH_BACKWARD and bw._lib.load().ur_attention_backward_supported(tq, tk, d)
    stats = bw.flash_stats(b, H, tq, tk, d, dev)
    assert stats is not None
    stats.fill_(float("nan"))
    vt = _vt(case["v"], dt, dev)
    if path == "fused_qkv":
        qkv = torch.cat([q, k, v], -1)
        o = ops.attention(qkv, qkv, vt, B=b, H=H, Tq=tq, Tk=tk, d=d, ldq=3 * C, ldk=3 * C, q_off=0, k_off=C, lse=stats[0])
        g = bw.attention_backward(qkv, qkv, qkv, do, H, fused_qkv=True, o=o, stats=stats).split(C, dim=-1)
    else:
        o = ops.attention(q, k, vt, B=b, H=H, Tq=tq, Tk=tk, d=d, ldq=C, ldk=C, lse=stats[0])
        g = bw.attention_backward(q, k, v, do, H, o=o, stats=stats if path == "fwd_lse" else None)
    torch.cuda.synchronize()
    return {n: ua.heads(t, H) for n, t in zip(("dq", "dk", "dv"), g)}, stats[0].double().cpu().view(b, H, tq)


def _check_flash(family, tq, tk, d, dtype, path, direct, dev, monkeypatch):
    from uni_renderer_amd import backward as bw
    monkeypatch.setattr(bw, "FLASH_DIRECT_MIN_D", direct)  # 0: [B, T, H*d] read in place; 1000: through per-head copies
    case, ref, fwd = _bwd_case(family, tq, tk, d, dtype)
    what = f"flash {family} {tq}x{tk} d{d} {path} direct_min_d={direct} {dtype}"
    got, lse = _flash(case, path, dev)
    ua.check_lse(lse, fwd[2], dtype, what)
    figs = ua.check_backward(got, ref, dtype, what, family)
    print({"case": what, "rel_l2_and_err_over_bound": figs})


@pytest.mark.parametrize("path", PATHS, ids=PID)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("d", [32, 40, 80, 160])
@pytest.mark.parametrize("family", ua.BWD_FAMILIES)
def test_flash_backward_self(dev, monkeypatch, path, dtype, d, family):
    """Self-attention (Tq = Tk = 128): the forward's lse or the dq kernel's own, head dims read in place or through
    per-head copies, separate operands or the fused q | k | v projection."""
    _check_flash(family, 128, 128, d, dtype, path[0], path[1], dev, monkeypatch)


@pytest.mark.parametrize("path", PATHS[:4], ids=PID[:4])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(128, 77, 32), (128, 77, 40), (128, 77, 80), (128, 77, 160), (512, 77, 40)],
                         ids=lambda s: f"{s[0]}x{s[1]}-d{s[2]}")
@pytest.mark.parametrize("family", ua.BWD_FAMILIES)
def test_flash_backward_cross(dev, monkeypatch, path, dtype, shape, family):
    """77 of 128 keys valid (masked, padded tile; sink_last sits on key 76), and 512 queries for which the dk / dv kernel
    splits the queries and folds fp32 partial sums."""
    from uni_renderer_amd import backward as bw
    tq, tk, d = shape
    if tq == 512:
        assert bw._lib.load().ur_attention_backward_splits(B * H, tq, 128, 64) > 1
    _check_flash(family, tq, tk, d, dtype, path[0], path[1], dev, monkeypatch)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(200, 77), (96, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("family", ua.MAT_FAMILIES)
def test_materialised_backward(dev, dtype, shape, d, family):
    """``o=None``: the materialised-P path that shapes with Tq % 64 != 0 fall back to, with the bound terms of its stored
    scores, P, dP and dS (util_attention docstring); flat, peaky and sink families only."""
    from uni_renderer_amd import backward as bw
    tq, tk = shape
    case, ref, _ = _bwd_case(family, tq, tk, d, dtype, materialised=True)
    q, k, v, do = (_tok(case[n]).to(dtype).to(dev) for n in ("q", "k", "v", "do"))
    g = bw.attention_backward(q, k, v, do, H)
    torch.cuda.synchronize()
    got = {n: ua.heads(t, H) for n, t in zip(("dq", "dk", "dv"), g)}
    what = f"materialised {family} {tq}x{tk} d{d} {dtype}"
    figs = ua.check_backward(got, ref, dtype, what, family, path="materialised")
    print({"case": what, "rel_l2_and_err_over_bound": figs})
