"""IP-Adapter without a GPU: the id -> module map, the loader, every argument error, load / unload hygiene, the float
restatement against ``F.scaled_dot_product_attention``, and the kernel test's element-wise bound -- checked against an fp32
emulation of the kernel's arithmetic and shown to catch planted errors."""
import copy
import math
import os

import pytest
import torch
import torch.nn.functional as F

import util_ip_adapter as IP
from util_models import O, product_config

CLIP = 48
DTYPES = [torch.float16, torch.bfloat16]


def _unet(cfg=O.TINY_CONFIG, device=None):
    import uni_renderer_amd as U

    if device is None:
        return U.UNet2DConditionModel(**product_config(cfg)).eval()
    with torch.device(device):
        return U.UNet2DConditionModel(**product_config(cfg))


@pytest.fixture(scope="module")
def unet():
    return _unet()


@pytest.fixture(scope="module")
def sd(unet):
    return IP.ip_state_dict(unet, CLIP, n_tokens=4, std=0.1, seed=7)


def test_processor_ids_of_the_sd15_unet():
    """The SD-1.x UNet: 32 attention processors, the 16 cross-attentions at the odd ids -- down 1..11, up 13..29, mid 31."""
    from uni_renderer_amd.ip_adapter import attn_processor_ids

    ids = attn_processor_ids(_unet(O.SD15_CONFIG, device="meta"))
    assert list(ids) == list(range(32))
    cross = {i: p for i, p in ids.items() if p.endswith("attn2")}
    assert list(cross) == list(range(1, 32, 2))
    want = {}
    n = 1
    for b in range(3):
        for a in range(2):
            want[n] = f"down_blocks.{b}.attentions.{a}.transformer_blocks.0.attn2"
            n += 2
    for b in (1, 2, 3):
        for a in range(3):
            want[n] = f"up_blocks.{b}.attentions.{a}.transformer_blocks.0.attn2"
            n += 2
    want[31] = "mid_block.attentions.0.transformer_blocks.0.attn2"
    assert cross == want
    assert all(ids[i - 1] == p[:-1] + "1" for i, p in cross.items())  # attn1 right before its attn2
    assert ids == IP.attn_processor_ids(_unet(O.SD15_CONFIG, device="meta"))  # the test util walks the same order


@pytest.mark.parametrize("ext", [".safetensors", ".bin"])
def test_loader_round_trip(tmp_path, unet, sd, ext):
    """Random tensors in the original key layout through a file: the UNet holds exactly them, knows clip_dim and N from the
    shapes, and has the config of the reference's branch."""
    from uni_renderer_amd.pipeline import UniRendererPipeline

    path = os.path.join(tmp_path, "adapter" + ext)
    if ext == ".safetensors":
        from safetensors.torch import save_file

        save_file(sd, path)
    else:
        nested = {"image_proj": {k[len("image_proj."):]: v for k, v in sd.items() if k.startswith("image_proj.")},
                  "ip_adapter": {k[len("ip_adapter."):]: v for k, v in sd.items() if k.startswith("ip_adapter.")}}
        torch.save(nested, path)  # the nested layout of the original checkpoints
    pipe = UniRendererPipeline(unet=unet)
    for args in ((path,), (str(tmp_path), None, "adapter" + ext)):
        pipe.load_ip_adapter(*args)
        try:
            st = unet._ip
            assert set(st.tensors) == set(sd) and all(torch.equal(st.tensors[k], sd[k]) for k in sd)
            assert (st.clip_dim, st.n_tokens, st.cross_dim, st.scale) == (CLIP, 4, 64, 1.0)
            assert list(st.ids) == list(range(1, 32, 2)) and len(st.slices) == 16
            assert st.total == sum(m.inner for m in unet._cross)
            assert unet.config["encoder_hid_dim_type"] == "ip_image_proj" and unet.config["encoder_hid_dim"] == CLIP
            assert unet.encoder_hid_proj is not None and unet.encoder_hid_proj.num_image_text_embeds == 4
            pipe.set_ip_adapter_scale(0.25)
            assert unet.ip_adapter_state() == (st.serial, 4, 0.25)
        finally:
            pipe.unload_ip_adapter()
    with pytest.raises(FileNotFoundError, match="local files only"):
        pipe.load_ip_adapter("h94/IP-Adapter", subfolder="models", weight_name="ip-adapter_sd15.bin")


def test_load_then_unload_leaves_the_network_as_it_was(tmp_path, unet, sd):
    keys, cfg, nparam = list(unet.state_dict()), copy.deepcopy(dict(unet.config)), sum(1 for _ in unet.parameters())
    unet._load_ip_adapter_weights(sd)
    try:
        assert list(unet.state_dict()) == keys and sum(1 for _ in unet.parameters()) == nparam  # the adapter is outside both
        unet.save_pretrained(os.path.join(tmp_path, "with_adapter"))
        assert unet.config["encoder_hid_dim_type"] == "ip_image_proj"
    finally:
        unet.unload_ip_adapter()
    assert list(unet.state_dict()) == keys and dict(unet.config) == cfg
    assert unet._ip is None and unet.encoder_hid_proj is None and unet.ip_adapter_state() is None
    unet.unload_ip_adapter()  # a second unload is a no-op
    back = type(unet).from_pretrained(os.path.join(tmp_path, "with_adapter"))  # the checkpoint is the network's own
    assert list(back.state_dict()) == keys and back.config["encoder_hid_dim_type"] is None and back._ip is None


def test_loader_argument_errors(unet, sd):
    def bad(change, exc, match):
        d = dict(sd)
        change(d)
        with pytest.raises(exc, match=match):
            unet._load_ip_adapter_weights(d)
        assert unet._ip is None and unet.config["encoder_hid_dim_type"] is None  # nothing half-loaded

    bad(lambda d: d.pop("ip_adapter.13.to_v_ip.weight"), KeyError, r"ip_adapter\.13\.to_v_ip\.weight")
    bad(lambda d: d.pop("image_proj.norm.bias"), KeyError, r"image_proj\.norm\.bias")
    bad(lambda d: d.update({"ip_adapter.5.to_k_ip.weight": torch.zeros(64, 64)}), ValueError, r"ip_adapter\.5\.to_k_ip\.weight")
    bad(lambda d: d.update({"ip_adapter.31.to_v_ip.weight": torch.zeros(128, 32)}), ValueError, r"ip_adapter\.31\.to_v_ip\.weight")
    bad(lambda d: d.update({"ip_adapter.2.to_k_ip.weight": torch.zeros(64, 64)}), ValueError, r"ip_adapter\.2\.to_k_ip\.weight")
    bad(lambda d: d.update({"image_proj.proj.weight": torch.zeros(4 * 64 + 8, CLIP)}), ValueError, r"image_proj\.proj\.weight")
    bad(lambda d: d.update({"image_proj.proj.bias": torch.zeros(7)}), ValueError, r"image_proj\.proj\.weight")
    bad(lambda d: d.update({"image_proj.norm.weight": torch.zeros(32)}), ValueError, r"image_proj\.norm\.weight")
    bad(lambda d: d.update({"image_proj.proj.weight": torch.zeros(17 * 64, CLIP), "image_proj.proj.bias": torch.zeros(17 * 64)}),
        NotImplementedError, r"image_proj\.proj\.weight.*17 image tokens")
    bad(lambda d: d.update({"image_proj.latents": torch.zeros(1, 16, 64)}), NotImplementedError, r"image_proj\.latents")  # "plus"
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        unet.set_ip_adapter_scale(0.5)
    unet._load_ip_adapter_weights(sd)
    try:
        with pytest.raises(ValueError, match="already loaded"):
            unet._load_ip_adapter_weights(sd)
        with pytest.raises(ValueError, match="not finite"):
            unet.set_ip_adapter_scale(float("nan"))
    finally:
        unet.unload_ip_adapter()


def test_forward_argument_errors(unet, sd):
    x, t, ehs = torch.zeros(1, 4, 8, 8), torch.tensor([1]), torch.zeros(1, 77, 64)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="added_cond_kwargs"):  # without an adapter: refused as before
            unet(x, t, ehs, added_cond_kwargs={"image_embeds": torch.zeros(1, CLIP)})
        unet._load_ip_adapter_weights(sd)
        try:
            for akw in (None, {}, {"text_embeds": torch.zeros(1, 8)}):
                with pytest.raises(ValueError, match="`encoder_hid_dim_type` set to 'ip_image_proj' which requires the keyword "
                                                     "argument `image_embeds`"):
                    unet(x, t, ehs, added_cond_kwargs=akw)
            with pytest.raises(NotImplementedError, match="text_embeds"):
                unet(x, t, ehs, added_cond_kwargs={"image_embeds": torch.zeros(1, CLIP), "text_embeds": torch.zeros(1, 8)})
            with pytest.raises(ValueError, match=rf"\[batch, {CLIP}\]"):
                unet(x, t, ehs, added_cond_kwargs={"image_embeds": torch.zeros(1, CLIP + 1)})
            unet.compute_dtype = torch.float16
            with pytest.raises(ValueError, match="requires the keyword argument `image_embeds`"):
                unet.ip_added_cond_kwargs(3)  # no embeddings were ever set for a batch of 3
        finally:
            unet.compute_dtype = None
            unet.unload_ip_adapter()
    unet._load_ip_adapter_weights(sd)
    try:
        with pytest.raises(NotImplementedError, match="IP-Adapter"):  # autograd: inference only, like FreeU
            unet(x.requires_grad_(True), t, ehs, added_cond_kwargs={"image_embeds": torch.zeros(1, CLIP)})
    finally:
        unet.unload_ip_adapter()


def test_pipeline_argument_errors(unet, sd):
    from uni_renderer_amd.pipeline import UniRendererPipeline

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    pipe = UniRendererPipeline(unet=unet, controlnet=unet, controldec=unet)
    pipe.set_progress_bar_config(disable=True)
    kw = dict(prompt_embeds=torch.zeros(1, 77, 64), image_latents=torch.zeros(1, 4, 8, 8), mask_latents=torch.zeros(1, 4, 8, 8),
              num_inference_steps=1, guidance_scale=0.0, output_type="latent")
    px = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe.real_image2mask_3mod_albedo(ip_adapter_image=px, **kw)
    with pytest.raises(ValueError, match="no IP-Adapter is loaded"):
        pipe.mask2image_3mod_albedo(prompt_embeds=kw["prompt_embeds"], attr_latents=torch.zeros(1, 28, 8, 8), ip_adapter_image=px,
                                    num_inference_steps=1, guidance_scale=0.0, output_type="latent")
    pipe.load_ip_adapter(sd)
    try:
        with pytest.raises(ValueError, match="image_encoder"):
            pipe.real_image2mask_3mod_albedo(ip_adapter_image=px, **kw)
        with pytest.raises(ValueError, match="pass ip_adapter_image"):
            pipe.image2mask_3mod_albedo(**kw)
        pipe.image_encoder = Enc()
        with pytest.raises(ValueError, match="feature_extractor"):
            pipe.real_image2mask_3mod_albedo(ip_adapter_image=[[0.0]], **kw)
    finally:
        pipe.unload_ip_adapter()
    with pytest.raises(ValueError, match="must have `unet`"):
        UniRendererPipeline().load_ip_adapter(sd)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement and the bound
# ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_sdpa():
    """``ip_reference`` (softmax in base 2 over scores that carry d^-1/2 log2 e) == hidden + scale * SDPA(q, k_ip, v_ip) with the
    raw q, per head; and the oracle restatement of a whole cross-attention: scale 0 is the oracle's own attention, the image
    term is linear in scale and equals to_out's weight applied to ``ip_reference``'s addend."""
    g = torch.Generator().manual_seed(0)
    B, T, H, d, N = 2, 9, 8, 40, 4
    C = H * d
    q, o = torch.randn(B, T, C, generator=g).double(), torch.randn(B, T, C, generator=g).double()
    k, v = torch.randn(B, N, C, generator=g).double(), torch.randn(B, N, C, generator=g).double()
    split = lambda t: t.view(B, -1, H, d).transpose(1, 2)
    want = o + 0.7 * F.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(1, 2).reshape(B, T, C)
    got = IP.ip_reference(o, q * (d ** -0.5 * IP.LOG2E), k, v, 0.7, H)
    assert float((got - want).abs().max()) < 1e-12

    attn = O.Attention(64, 2, 32, cross_attention_dim=48).double()
    x, ctx, tok = torch.randn(B, T, 64, generator=g).double(), torch.randn(B, 77, 48, generator=g).double(), torch.randn(B, N, 48, generator=g).double()
    wk, wv = torch.randn(64, 48, generator=g).double(), torch.randn(64, 48, generator=g).double()
    with torch.no_grad():
        y0, y1, y3 = (IP.ip_attention(attn, x, ctx, tok, wk, wv, s) for s in (0.0, 1.0, 3.0))
        assert float((y0 - attn(x, ctx)).abs().max()) < 1e-12
        assert float(((y3 - y0) - 3 * (y1 - y0)).abs().max()) < 1e-11
        qlog = attn.to_q(x) * (32 ** -0.5 * IP.LOG2E)
        add = IP.ip_reference(torch.zeros(B, T, 64).double(), qlog, tok @ wk.t(), tok @ wv.t(), 1.0, 2)
        assert float(((y1 - y0) - add @ attn.to_out[0].weight.t()).abs().max()) < 1e-11
    proj = IP.ImageProjection(CLIP, 64, 4)
    e = torch.randn(3, CLIP, generator=g)
    with torch.no_grad():
        want_tok = F.layer_norm(F.linear(e, proj.image_embeds.weight, proj.image_embeds.bias).view(3, 4, 64), (64,), proj.norm.weight, proj.norm.bias)
        assert torch.equal(proj(e), want_tok)


def _kernel_case(H, d, N, T, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + d + N)
    C = H * d
    r = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return r(2, T, C), r(2, T, C), r(2, N, C), r(2, N, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("H,d,N", [(8, 40, 4), (8, 80, 16), (8, 160, 4), (8, 160, 1), (2, 32, 4), (2, 64, 5)])
def test_bound_holds_for_the_fp32_emulation_and_catches_planted_errors(dtype, H, d, N):
    """The bound the GPU test asserts (derived in util_ip_adapter.py) against the kernel's arithmetic emulated in numpy fp32 on
    N(0, 1) data: every element inside, and not loosely -- the storage rounding alone reaches half of it somewhere.  A dropped
    token, keys and values of the wrong head, and ``scale`` applied twice each land far outside."""
    o, q, k, v = _kernel_case(H, d, N, 21, dtype)
    scale = 0.7
    ref, bound = IP.ip_reference(o, q, k, v, scale, H), IP.ip_bound(o, q, k, v, scale, H, dtype)
    ratio = ((IP.ip_emulate_fp32(o, q, k, v, scale, H, dtype) - ref).abs() / bound).max()
    assert 0.5 < float(ratio) <= 1.0, float(ratio)
    planted = [dict(wrong_head=True), dict(scale_twice=True)] + ([dict(drop_token=0), dict(drop_token=N - 1)] if N > 1 else [])
    for kw in planted:
        bad = ((IP.ip_emulate_fp32(o, q, k, v, scale, H, dtype, **kw) - ref).abs() / bound)
        # (a dropped token only shows in the rows where it carries weight: about 1 / N of them on this peaked data)
        assert float(bad.max()) > 100 and float((bad > 1).double().mean()) > 0.5 / max(N, 2), (kw, float(bad.max()))


def test_bound_terms():
    """The pieces of the derivation: the summation tree of every head width the kernel instantiates, the monotonicity of the
    bound in the score magnitudes, and its floor of one storage rounding."""
    assert [IP.tree(d) for d in (32, 40, 64, 80, 128, 160)] == [(4, 1, 10), (1, 5, 12), (8, 1, 11), (2, 5, 13), (16, 1, 12), (4, 5, 14)]
    o, q, k, v = _kernel_case(8, 40, 4, 5, torch.float16)
    b1 = IP.ip_bound(o, q, k, v, 0.7, 8, torch.float16)
    b2 = IP.ip_bound(o, q * 8, k, v, 0.7, 8, torch.float16)
    ref = IP.ip_reference(o, q, k, v, 0.7, 8)
    assert bool((b1 >= IP.U_[torch.float16] * ref.abs()).all())
    assert float(b2.sum()) > 0 and math.isfinite(float(b2.max()))
    s = torch.einsum("bthd,bjhd->bthj", q.double().view(2, 5, 8, 40), k.double().view(2, 4, 8, 40))
    assert float(s.abs().max()) > 1  # the scores are not degenerate
