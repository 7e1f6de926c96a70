"""IP-Adapter image prompts on the MI355X: the UNet with a random adapter against the float restatement on the CPU oracle
(util_ip_adapter.py) through every executor -- module forward, grouped step and its graph, hoisted rendering and inverse steps,
the 320-channel chain path -- and through the pipeline with a stub image encoder.  Tolerances: the tiny-config bounds of
tests/test_freeu_gpu.py (``TOLS``)."""
import functools
import json
import types

import pytest
import torch

import util_ip_adapter as IP
from conftest import rel_l2
from util_models import O, build_product_from_oracle

pytestmark = pytest.mark.gpu

LATENTS = [(32, 32), (20, 12)]
TOLS = [(torch.float16, 3e-3), (torch.bfloat16, 2.5e-2)]  # tests/test_freeu_gpu.py, tests/test_model_gpu.py
CLIP_DIM = 48   # no multiple of the GEMM's 64-column K chunk: the zero-padded buffer is exercised
N_TOKENS = 4
STD = 0.1       # of the random to_k_ip / to_v_ip: the CPU oracle's img_pred then moves by 0.36 - 0.38 rel-L2 (>= 10 x 2.5e-2)
SCALE = 0.8
# the 320-channel level of the SD-1.x UNet (8 heads of 40: the chain kernels) above three 256-channel levels (8 heads of 32)
CHAIN_CONFIG = dict(O.TINY_CONFIG, block_out_channels=(320, 256, 256, 256), attention_head_dim=8)


@functools.lru_cache(maxsize=None)
def _oracle(chain=False):
    return O.build_triplet(CHAIN_CONFIG if chain else O.TINY_CONFIG, seed=1234)


@functools.lru_cache(maxsize=None)
def _adapter(chain=False):
    return IP.ip_state_dict(_oracle(chain)[0], CLIP_DIM, n_tokens=N_TOKENS, std=STD, seed=7)


@functools.lru_cache(maxsize=None)
def _embeds():
    return torch.randn(2, CLIP_DIM, generator=torch.Generator().manual_seed(5))


@functools.lru_cache(maxsize=None)
def _case(hw):
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 4, *hw, generator=g)
    c = torch.randn(2, 28, *hw, generator=g)
    ehs = torch.randn(2, 77, 64, generator=g) * 0.5
    return x, c, ehs, torch.tensor([500, 200]), torch.tensor([300, 700])


@functools.lru_cache(maxsize=None)
def _ref(hw, on, exchange=True, run_decoder=True, t_attr0=False, t_img0=False, chain=False):
    """The oracle's outputs, computed once per case and shared (never modified)."""
    x, c, ehs, ti, ta = _case(hw)
    ta = torch.zeros_like(ta) if t_attr0 else ta
    ti = torch.zeros_like(ti) if t_img0 else ti
    return IP.oracle_step(*_oracle(chain), x, c, ehs, ti, ta, adapter=_adapter(chain) if on else None, image_embeds=_embeds(),
                          scale=SCALE, exchange=exchange, run_decoder=run_decoder)


@functools.lru_cache(maxsize=None)
def _product(dtype, chain=False):
    return build_product_from_oracle(*_oracle(chain), dtype, torch.device("cuda:0"))


class _Loaded:
    """``with _Loaded(unet):`` the random adapter at SCALE with the test embeddings in the static buffer; unloaded afterwards."""

    def __init__(self, unet, chain=False, embeds=True):
        self.unet, self.chain, self.embeds = unet, chain, embeds

    def __enter__(self):
        self.unet._load_ip_adapter_weights(_adapter(self.chain))
        self.unet.set_ip_adapter_scale(SCALE)
        if self.embeds:
            self.unet.set_ip_adapter_image_embeds(_embeds().to(self.unet.device))
        return self.unet

    def __exit__(self, *exc):
        self.unet.unload_ip_adapter()
        return False


def _assert_sees_adapter(ref_on, ref_off, tol, got_on, key="img_pred"):
    """Non-vacuity: the oracle's UNet sample moves by >= 10 x the tolerance when the adapter is switched on, and the product's
    output with the adapter fails the bound against the adapter-off oracle."""
    sep = rel_l2(ref_on[key], ref_off[key])
    assert sep >= 10 * tol, sep
    assert rel_l2(got_on, ref_off[key]) > 2 * tol
    return sep


def _modules_step(unet, enc, dec, x, c, ehs, ti, ta, embeds=None):
    """The reference's per-step call pattern with the image prompt going to the UNet only."""
    res, mid, raw_enc, raw_mid_enc = enc(x, ta, encoder_hidden_states=ehs, controlnet_cond=c, return_dict=False)
    img, raw_unet, raw_mid_unet, ups = unet(x, ti, encoder_hidden_states=ehs, down_block_additional_residuals=res,
                                            mid_block_additional_residual=mid, return_dict=False,
                                            added_cond_kwargs=None if embeds is None else {"image_embeds": embeds})
    attr = dec(sample=raw_mid_enc, down_block_res_samples=raw_enc, timestep=ta, encoder_hidden_states=ehs,
               down_block_additional_residuals=raw_unet, mid_block_additional_residual=raw_mid_unet, return_dict=False)
    return dict(img_pred=img, attr_pred=attr, raw_unet=raw_unet, raw_mid_unet=raw_mid_unet, up_res=ups)


def _errs(out, ref):
    e = {k: rel_l2(out[k], ref[k]) for k in ("img_pred", "attr_pred", "raw_mid_unet") if out.get(k) is not None and ref.get(k) is not None}
    for k in ("raw_unet", "up_res"):
        if k in out and k in ref:
            for i, (a, b) in enumerate(zip(out[k], ref[k])):
                e[f"{k}[{i}]"] = rel_l2(a, b)
    return e


@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_module_forward_vs_oracle(dev, dtype, tol, hw):
    """enc -> unet -> dec through the modules (or the UNet alone) with ``added_cond_kwargs={"image_embeds": ...}``: img_pred /
    attr_pred within the tiny-config bound, every raw / up_res tensor within twice it.  scale = 0 and load-then-unload are
    ``torch.equal`` to the network that never had an adapter."""
    for exchange in (True, False):
        _module_forward_case(dev, dtype, tol, hw, exchange)


def _module_forward_case(dev, dtype, tol, hw, exchange):
    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    e = _embeds().to(dev)

    def run(embeds):
        with torch.no_grad():
            if exchange:
                return _modules_step(unet, enc, dec, x, c, ehs, ti, ta, embeds)
            img, raw, raw_mid, ups = unet(x, ti, ehs, return_dict=False, added_cond_kwargs=None if embeds is None else {"image_embeds": embeds})
            return dict(img_pred=img, raw_unet=raw, raw_mid_unet=raw_mid, up_res=ups)

    base = run(None)
    with _Loaded(unet, embeds=False):
        on = run(e)
        unet.set_ip_adapter_scale(0.0)
        zero = run(e)
    after = run(None)
    errs = _errs(on, _ref(hw, True, exchange))
    sep = _assert_sees_adapter(_ref(hw, True, exchange), _ref(hw, False, exchange), tol, on["img_pred"])
    print(json.dumps(dict(executor="modules", dtype=str(dtype), hw=hw, exchange=exchange, oracle_on_vs_off=round(sep, 4),
                          on={k: round(v, 6) for k, v in errs.items()})))
    assert errs["img_pred"] < tol and errs.get("attr_pred", 0.0) < tol, errs
    assert max(errs.values()) < 2 * tol, errs
    for k in ("img_pred", "attr_pred", "raw_mid_unet"):
        if base.get(k) is not None:
            assert torch.equal(zero[k], base[k]) and torch.equal(after[k], base[k]), k
    assert unet.config["encoder_hid_dim_type"] is None and unet.encoder_hid_proj is None


@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_grouped_step_vs_oracle_and_its_graph(dev, dtype, tol, hw):
    """The grouped executor (the UNet's rows of the [enc ; unet] and [unet ; dec] launches get the image attention), eager
    against the oracle and its captured graph against the eager run bit for bit; new embeddings reach a captured graph through
    the static buffer; scale = 0 and unload equal the executor without an adapter."""
    from uni_renderer_amd.fused import GroupedDualStreamStep
    from uni_renderer_amd.graph import GraphedDualStreamStep

    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    step = lambda: {k: v.clone() for k, v in GroupedDualStreamStep(unet, enc, dec)(x, c, ehs, ti, ta).items()}
    with torch.no_grad():
        base = step()
        with _Loaded(unet):
            on = step()
            g = GraphedDualStreamStep(unet, enc, dec, 2, hw, 64, dtype=dtype, device=dev, mode="grouped")
            rep = {k: v.clone() for k, v in g.step(x.to(dtype), c.to(dtype), ehs.to(dtype), ti, ta).items()}
            unet.set_ip_adapter_image_embeds(-_embeds().to(dev))  # other embeddings: a device copy, no capture
            other_eager = step()
            other_rep = {k: v.clone() for k, v in g.step(x.to(dtype), c.to(dtype), ehs.to(dtype), ti, ta).items()}
            unet.set_ip_adapter_scale(0.0)
            zero = step()
        after = step()
    errs = _errs(on, _ref(hw, True))
    _assert_sees_adapter(_ref(hw, True), _ref(hw, False), tol, on["img_pred"])
    print(json.dumps(dict(executor="grouped", dtype=str(dtype), hw=hw, on=errs)))
    assert errs["img_pred"] < tol and errs["attr_pred"] < tol, errs
    for k in ("img_pred", "attr_pred"):
        assert torch.equal(rep[k], on[k]) and torch.equal(other_rep[k], other_eager[k]), k
        assert torch.equal(zero[k], base[k]) and torch.equal(after[k], base[k]), k
    assert not torch.equal(other_eager["img_pred"], on["img_pred"])


@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_hoisted_steps_vs_oracle_and_their_graphs(dev, dtype, tol, hw):
    """The hoisted loops' steps.  Rendering (encoder once, UNet per step; t_attr = 0): img_pred against the oracle.  Inverse
    (UNet down + mid once, on the clean image at t_img = 0, the image K / V computed in the prologue with the prompt's; encoder
    and decoder per step): attr_pred, which the adapter reaches through the exchange.  Captured graphs == eager, bit for bit."""
    from uni_renderer_amd.graph import GraphedHoistedStep
    from uni_renderer_amd.hoist import HoistedSamplingStep

    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    t0 = torch.zeros(2, device=dev)

    def render():
        return HoistedSamplingStep(unet, enc, dec, "render").prologue(c, ehs, t0).step(x, ti.float())["img_pred"].clone()

    def inverse():
        return HoistedSamplingStep(unet, enc, dec, "inverse").prologue(x, ehs, t0).step(c, ta.float())["attr_pred"].clone()

    with torch.no_grad():
        base_r, base_i = render(), inverse()
        with _Loaded(unet):
            on_r, on_i = render(), inverse()
            gr = GraphedHoistedStep(unet, enc, dec, 2, hw, 64, dtype=dtype, device=dev, run_decoder=False)
            rep_r = gr.step(x.to(dtype), c.to(dtype), ehs.to(dtype), ti.float(), t0)["img_pred"].clone()
            gi = GraphedHoistedStep(unet, enc, dec, 2, hw, 64, dtype=dtype, device=dev, run_decoder=True)
            rep_i = gi.step(x.to(dtype), c.to(dtype), ehs.to(dtype), t0, ta.float())["attr_pred"].clone()
            unet.set_ip_adapter_scale(0.0)
            zero_r, zero_i = render(), inverse()
        after_r, after_i = render(), inverse()
    ref_r = {o: _ref(hw, o, True, run_decoder=False, t_attr0=True) for o in (True, False)}
    ref_i = {o: _ref(hw, o, True, t_img0=True) for o in (True, False)}
    e_r, e_i = rel_l2(on_r, ref_r[True]["img_pred"]), rel_l2(on_i, ref_i[True]["attr_pred"])
    sep_i = rel_l2(ref_i[True]["attr_pred"], ref_i[False]["attr_pred"])
    print(json.dumps(dict(executor="hoisted", dtype=str(dtype), hw=hw, render=e_r, inverse=e_i, oracle_attr_on_vs_off=round(sep_i, 4))))
    _assert_sees_adapter(ref_r[True], ref_r[False], tol, on_r)
    assert e_r < tol and e_i < tol, (e_r, e_i)
    assert torch.equal(rep_r, on_r) and torch.equal(rep_i, on_i)
    assert not torch.equal(on_i, base_i)  # the decoder sees the adapted UNet's raw skips
    assert torch.equal(zero_r, base_r) and torch.equal(zero_i, base_i) and torch.equal(after_r, base_r) and torch.equal(after_i, base_i)


@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_chain_path_vs_oracle(dev, dtype, tol, monkeypatch):
    """A 320-channel first level (8 heads of 40) whose transformers run as ``ur_tchain`` launches: the image attention reads
    the head-major q2 the chain hands to the cross-attention.  Grouped step with the chain against the oracle, and against the
    same step on the GEMM-by-GEMM path (the chain folds the q scale into the weights: close, not equal).  A 16x16 latent takes
    the chain only with the row threshold lowered, which the test does; (20, 12) above never does."""
    from uni_renderer_amd import fused, ops

    hw = (16, 16)
    unet, enc, dec = _product(dtype, chain=True)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    monkeypatch.setattr(fused, "TCHAIN_MIN_ROWS", 0)
    seen = []
    real = ops.ip_attention_add
    monkeypatch.setattr(ops, "ip_attention_add", lambda *a, **k: (seen.append(k.get("q_hstride", 0)), real(*a, **k))[1])

    def step(chain):
        s = fused.GroupedDualStreamStep(unet, enc, dec)
        s.use_tchain = chain
        return {k: v.clone() for k, v in s(x, c, ehs, ti, ta).items()}

    with torch.no_grad():
        base = step(True)
        with _Loaded(unet, chain=True):
            on = step(True)
            n_chain = sum(1 for h in seen if h)
            plain = step(False)
            unet.set_ip_adapter_scale(0.0)
            zero = step(True)
    ref_on, ref_off = (_ref(hw, o, chain=True) for o in (True, False))
    errs, errs_plain = _errs(on, ref_on), _errs(plain, ref_on)
    sep = rel_l2(ref_on["img_pred"], ref_off["img_pred"])
    print(json.dumps(dict(executor="grouped+chain", dtype=str(dtype), on=errs, gemm_path=errs_plain, oracle_on_vs_off=round(sep, 4),
                          head_major_launches=n_chain, chain_vs_gemm=rel_l2(on["img_pred"], plain["img_pred"]))))
    assert n_chain == 5  # the 320-channel cross-attentions: 2 down + 3 up, all on head-major q
    assert sep >= 10 * tol and rel_l2(on["img_pred"], ref_off["img_pred"]) > 2 * tol
    assert errs["img_pred"] < tol and errs["attr_pred"] < tol, errs
    assert errs_plain["img_pred"] < tol and errs_plain["attr_pred"] < tol, errs_plain
    assert torch.equal(zero["img_pred"], base["img_pred"]) and torch.equal(zero["attr_pred"], base["attr_pred"])


def test_module_graph_replay_equals_eager(dev):
    """serial and concurrent captures of the module path with the adapter == the eager launches, bit for bit."""
    from uni_renderer_amd.graph import GraphedDualStreamStep, dual_stream_step

    unet, enc, dec = _product(torch.float16)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case((20, 12))]
    x, c, ehs, ti, ta = x.half(), c.half(), ehs.half(), ti.float(), ta.float()
    with _Loaded(unet), torch.no_grad():
        ref = dual_stream_step(unet, enc, dec, x, c, ehs, ti, ta)
        for mode in ("serial", "concurrent"):
            o = GraphedDualStreamStep(unet, enc, dec, 2, (20, 12), 64, mode=mode).step(x, c, ehs, ti, ta)
            for k in ("img_pred", "attr_pred"):
                assert torch.equal(o[k], ref[k]), (mode, k)
    assert rel_l2(ref["img_pred"], _ref((20, 12), True)["img_pred"]) < 3e-3


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------------
class StubImageEncoder(torch.nn.Module):
    """Stands in for the CLIP vision tower: fixed ``image_embeds`` = a fixed linear map of the pixels."""

    def __init__(self, clip_dim=CLIP_DIM):
        super().__init__()
        w = torch.randn(3 * 8 * 8, clip_dim, generator=torch.Generator().manual_seed(3)) * 0.1
        self.w = torch.nn.Parameter(w, requires_grad=False)
        self.calls = 0

    def forward(self, pixels):
        self.calls += 1
        return types.SimpleNamespace(image_embeds=pixels.flatten(1) @ self.w)


def _pipe(dev, seed=21):
    from uni_renderer_amd.pipeline import UniRendererPipeline

    models = O.build_triplet(O.TINY_CONFIG, seed=seed)
    unet, enc, dec = build_product_from_oracle(*models, torch.float16, dev)
    pipe = UniRendererPipeline(unet=unet, controlnet=enc, controldec=dec, image_encoder=StubImageEncoder().to(dev).half())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _pipe_inputs(dev, batch=2):
    g = torch.Generator().manual_seed(5)
    ehs = (torch.randn(1, 77, 64, generator=g) * 0.5).to(dev).half()
    noise = torch.randn(batch, 4, 16, 16, generator=g)
    attr = torch.randn(batch, 28, 16, 16, generator=g).to(dev)
    img, mask = torch.randn(1, 4, 16, 16, generator=g).to(dev), torch.randn(1, 4, 16, 16, generator=g).to(dev)
    pixels = torch.randn(1, 3, 8, 8, generator=g)
    return ehs, noise, attr, img, mask, pixels


@pytest.mark.parametrize("fused_sampler", [True, False], ids=["device_loop", "step_by_step"])
def test_pipeline_toggle_on_off_on(dev, fused_sampler):
    """Both loops through the pipeline: off after on == a pipeline that never loaded an adapter, the second on == the first (no
    stale graph in either direction), on != off; the same call twice gives the same latents; a scale change is never served by
    a graph captured at another scale."""
    ehs, noise, attr, img, mask, pixels = _pipe_inputs(dev)
    kw = dict(prompt_embeds=ehs, attr_latents=attr, latents=noise, num_inference_steps=2, guidance_scale=0.0, output_type="latent")
    kwi = dict(prompt_embeds=ehs, image_latents=img.repeat(2, 1, 1, 1), mask_latents=mask.repeat(2, 1, 1, 1), latents=noise,
               num_inference_steps=2, guidance_scale=0.0, output_type="latent")
    never = _pipe(dev)
    never.use_fused_sampler = fused_sampler
    base, base_inv = never.mask2image_3mod_albedo(**kw), never.real_image2mask_3mod_albedo(**kwi)
    pipe = _pipe(dev)
    pipe.use_fused_sampler = fused_sampler
    sd = IP.ip_state_dict(pipe.unet, CLIP_DIM, n_tokens=N_TOKENS, std=STD, seed=7)
    assert torch.equal(pipe.mask2image_3mod_albedo(**kw), base)
    pipe.load_ip_adapter(sd)
    on1 = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    on1_again = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    inv_on = pipe.real_image2mask_3mod_albedo(ip_adapter_image=pixels, **kwi)
    pipe.set_ip_adapter_scale(0.5)
    half = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    pipe.set_ip_adapter_scale(1.0)
    on_back = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    other = pipe.mask2image_3mod_albedo(ip_adapter_image=-pixels, **kw)  # another image through the same graphs
    pipe.unload_ip_adapter()
    off1, off_inv = pipe.mask2image_3mod_albedo(**kw), pipe.real_image2mask_3mod_albedo(**kwi)
    pipe.load_ip_adapter(sd)
    on2 = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    inv_on2 = pipe.real_image2mask_3mod_albedo(ip_adapter_image=pixels, **kwi)
    pipe.set_ip_adapter_scale(0.5)
    half2 = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw)
    assert torch.equal(off1, base) and all(torch.equal(a, b) for a, b in zip(off_inv, base_inv))
    assert torch.equal(on1_again, on1) and torch.equal(on_back, on1) and torch.equal(on2, on1) and torch.equal(half2, half)
    assert all(torch.equal(a, b) for a, b in zip(inv_on2, inv_on))
    assert rel_l2(on1, base) > 1e-2 and rel_l2(half, on1) > 1e-3 and rel_l2(half, base) > 1e-3 and rel_l2(other, on1) > 1e-3
    assert any(not torch.equal(a, b) for a, b in zip(inv_on, base_inv))


@pytest.mark.parametrize("fused_sampler", [True, False], ids=["device_loop", "step_by_step"])
def test_pipeline_guidance_and_images_per_prompt(dev, fused_sampler):
    """guidance != 0 (the batch is [zeros ; embeds]) with num_images_per_prompt = 2 (one image prompt folded over two
    latents), inverse and rendering loops: twice the same, and the adapter moves the result.  With the adapter at scale 0 the guided result equals the pipeline without one."""
    ehs, noise, attr, img, mask, pixels = _pipe_inputs(dev)
    kwi = dict(prompt_embeds=ehs, image_latents=img, mask_latents=mask, latents=noise, num_inference_steps=2, guidance_scale=3.0,
               num_images_per_prompt=2, output_type="latent")
    kw = dict(prompt_embeds=ehs, attr_latents=attr, latents=noise, num_inference_steps=2, guidance_scale=3.0,
              num_images_per_prompt=2, output_type="latent")
    pipe = _pipe(dev)
    pipe.use_fused_sampler = fused_sampler
    base, base_inv = pipe.mask2image_3mod_albedo(**kw), pipe.real_image2mask_3mod_albedo(**kwi)
    pipe.load_ip_adapter(IP.ip_state_dict(pipe.unet, CLIP_DIM, n_tokens=N_TOKENS, std=STD, seed=7))
    on, inv = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw), pipe.real_image2mask_3mod_albedo(ip_adapter_image=pixels, **kwi)
    on_b, inv_b = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw), pipe.real_image2mask_3mod_albedo(ip_adapter_image=pixels, **kwi)
    buf = pipe.unet._ip.buffer(4, torch.float16, pipe.unet.device)
    assert buf is not None and float(buf[:2].abs().max()) == 0.0 and float(buf[2:].abs().max()) > 0  # [zeros ; embeds]
    assert torch.equal(buf[2], buf[3])                                                                # folded over the two latents
    pipe.set_ip_adapter_scale(0.0)
    zero, zero_inv = pipe.mask2image_3mod_albedo(ip_adapter_image=pixels, **kw), pipe.real_image2mask_3mod_albedo(ip_adapter_image=pixels, **kwi)
    assert on.shape[0] == 2 and torch.equal(on_b, on) and all(torch.equal(a, b) for a, b in zip(inv_b, inv))
    assert rel_l2(on, base) > 1e-2 and any(not torch.equal(a, b) for a, b in zip(inv, base_inv))
    assert torch.equal(zero, base) and all(torch.equal(a, b) for a, b in zip(zero_inv, base_inv))


def test_autograd_forward_with_adapter_raises(dev):
    unet, enc, dec = _product(torch.float16)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case((32, 32))]
    with _Loaded(unet):
        with pytest.raises(NotImplementedError, match="IP-Adapter"):
            unet(x.half().requires_grad_(True), ti, ehs.half(), added_cond_kwargs={"image_embeds": _embeds().to(dev)})
