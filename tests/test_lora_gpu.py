"""GPU tests of the LoRA merge: ur_lora_merge_multi per element (exactly on integer data, within the derived bound on random
data, many items in guarded buffers) and the merged adapter through the networks, the executors' packed copies and the
pipeline's graphs."""
import pytest
import torch

import util_lora as L
from conftest import rel_l2
from util_models import O, build_product_from_oracle, product_step

gpu = pytest.mark.gpu
NET_SEED, ADAPTER_SEED, NET_SCALE = 1234, 77, 0.7
SHAPES = [(1, 1, 1), (3, 5, 2), (64, 36, 4), (65, 257, 33), (16, 2880, 8), (320, 320, 4), (130, 64, 0)]
RANKS = [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129]
SCALES = [1.0, -2.0, 0.5]


def _cap():
    from uni_renderer_amd import lora

    return lora.max_rank()


def exact_cases():
    """((N, K, R), scale, seed) of the exact test; the scales (a negative one and 0.5 among them) rotate over the cases."""
    shapes = SHAPES + [(33, 72, r) for r in RANKS + [_cap()]]
    return [(s, SCALES[i % len(SCALES)], 100 + i) for i, s in enumerate(shapes)]


@gpu
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_merge_is_exact_on_integer_data(dev, dtype):
    cases = exact_cases()
    problems = [L.int_problem(N, K, R, dtype, seed, scale) for (N, K, R), scale, seed in cases]
    refs = []
    for p in problems:
        ref, _ = L.ref_merge(*p)
        assert L.representable(ref, dtype)  # ... so the one rounding at the store cannot move it
        refs.append(ref)
    ws, _ = L.launch(problems, dtype, dev)
    for (shape, scale, _), w, ref in zip(cases, ws, refs):
        assert torch.equal(w.cpu(), ref.to(dtype)), (shape, scale)


@gpu
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_rank_zero_copies_bits(dev, dtype):
    """R == 0: w receives base bit for bit -- -0.0, a NaN with a payload, an infinity and subnormals included."""
    N, K = 130, 64
    base, *_ = L.int_problem(N, K, 0, dtype, 5, 1.0)
    iv = L.INT_VIEW[dtype.itemsize]
    bits = base.view(iv)
    special = {torch.float16: [-0x8000, 0x7E01, 0x7C00, 0x0001, 0x7D55], torch.bfloat16: [-0x8000, 0x7FC1, 0x7F80, 0x0001, 0x7FA5],
               torch.float32: [-0x80000000, 0x7FC00001, 0x7F800000, 0x00000001, 0x7FA00055]}[dtype]  # last: a signalling NaN
    for i, v in enumerate(special):
        bits[i, 7 * i] = v
        bits[N - 1 - i, K - 1 - i] = v
    for shape in ((N, K), (N - 2, K + 1)):  # the 4-element path and the element-wise one (K = 65)
        b = base.reshape(-1)[:shape[0] * shape[1]].reshape(shape).clone() if shape != (N, K) else base
        ws, bases = L.launch([(b, None, None, None, 1.0)], dtype, dev)
        assert torch.equal(ws[0].view(iv).cpu(), b.view(iv)) and torch.equal(bases[0].view(iv).cpu(), b.view(iv))


@gpu
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_merge_random_data_within_the_derived_bound(dev, dtype):
    shapes = SHAPES[:-1] + [(33, 72, r) for r in (17, 129, _cap())]
    problems = [L.rand_problem(N, K, R, dtype, 200 + i, (0.7, -1.3, 1.0)[i % 3]) for i, (N, K, R) in enumerate(shapes)]
    problems[1] = problems[1][:3] + (None,) + problems[1][4:]  # rscale = NULL: ones
    ws, _ = L.launch(problems, dtype, dev)
    for shape, p, w in zip(shapes, problems, ws):
        ref, _ = L.ref_merge(*p)
        got = w.cpu().double()
        err, bnd = (got - ref).abs(), L.bound(*p, got, dtype)
        print(f"{str(dtype):15s} {str(shape):18s} worst |got - ref| / bound = {float((err / bnd).max()):.3f}")
        assert bool((err <= bnd).all()), (shape, float((err / bnd).max()))


@gpu
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_one_launch_of_many_items_in_guarded_buffers(dev, dtype):
    """lora.multi_max() items of mixed shapes in ONE launch, one-workgroup items first and last, every output between
    canaries (some at element offsets that force the element-wise path): exact results, canaries and every base untouched,
    identical bits on a second run."""
    from uni_renderer_amd import lora

    nmax = lora.multi_max()
    cycle = [(1, 1, 1), (65, 257, 33), (64, 36, 4), (33, 72, 17), (130, 64, 0), (16, 2880, 8), (40, 128, 64), (3, 5, 2)]
    shapes = [cycle[i % len(cycle)] for i in range(nmax)]
    shapes[0], shapes[-1] = (1, 1, 1), (3, 5, 2)
    problems = [L.int_problem(N, K, R, dtype, 300 + i, SCALES[i % 3]) for i, (N, K, R) in enumerate(shapes)]
    runs = []
    for _ in range(2):
        g = L.Guarded(dtype, dev)
        for i, (N, K, _) in enumerate(shapes):
            g.reserve(N * K, offset=i % 4)  # offsets 1..3: rows of K % 4 == 0 that do not start on a 4-element boundary
        g.allocate()
        outs = [g.view(i, (N, K)) for i, (N, K, _) in enumerate(shapes)]
        ws, bases = L.launch(problems, dtype, dev, outs=outs)
        g.check()
        for p, b in zip(problems, bases):
            assert torch.equal(b.cpu().view(L.INT_VIEW[dtype.itemsize]), p[0].view(L.INT_VIEW[dtype.itemsize]))
        runs.append(g.buf.clone())
        for shape, p, w in zip(shapes, problems, ws):
            ref, _ = L.ref_merge(*p)
            assert L.representable(ref, dtype)
            assert torch.equal(w.cpu(), ref.to(dtype)), shape
    assert torch.equal(runs[0].view(L.INT_VIEW[dtype.itemsize]), runs[1].view(L.INT_VIEW[dtype.itemsize]))


# ---------------------------------------------------------------------------------------------------------------------
# through the networks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net_ref():
    """The oracle triplet, inputs, the adapter and the CPU oracle's outputs without it and with the float64-merged weights."""
    oracle = O.build_triplet(O.TINY_CONFIG, seed=NET_SEED)
    inputs = O.make_inputs(2, 16, 64, seed=99)
    sd, alphas, spec = L.make_adapter(oracle[0], seed=ADAPTER_SEED)
    merged = O.dual_stream_step(L.oracle_with_merged(oracle[0], spec, NET_SCALE), oracle[1], oracle[2], *inputs)
    return oracle, inputs, (sd, alphas, spec), merged


@gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 3e-3), (torch.bfloat16, 2.5e-2)])
def test_tiny_step_with_adapter_vs_oracle_with_merged_weights(dev, net_ref, dtype, tol):
    oracle, inputs, (sd, alphas, spec), merged = net_ref
    unet, enc, dec = build_product_from_oracle(*oracle, dtype, dev)
    g = [t.to(dev) for t in inputs]
    with torch.no_grad():
        plain = L.step_with_scale(unet, enc, dec, *g, None)
        unet.load_attn_procs({"unet." + k: v for k, v in sd.items()}, network_alphas=alphas)
        assert unet.lora_scale == 1.0
        out = L.step_with_scale(unet, enc, dec, *g, {"scale": NET_SCALE})
        assert unet.lora_scale == NET_SCALE
    errs = {k: rel_l2(out[k], merged[k]) for k in ("img_pred", "attr_pred")}
    moved = rel_l2(out["img_pred"], plain["img_pred"])
    print(f"{dtype}: vs merged oracle {errs}, vs no adapter {moved:.3f}")
    assert max(errs.values()) < tol, errs
    assert moved > 10 * tol, moved
    # the merged parameters are the float64 merge of the parameters the model held, to the derived bound
    with torch.no_grad():
        fresh = build_product_from_oracle(*oracle, dtype, dev)[0]
    want = L.merged_weights(fresh, [(spec, 1.0)], NET_SCALE)
    for n, (down, up, factor) in list(spec.items())[::7]:
        w0 = fresh.get_submodule(n).weight.detach().cpu()
        got = unet.get_submodule(n).weight.detach().cpu().double().reshape(w0.shape[0], -1)
        rs = torch.full((down.shape[0],), factor)
        bnd = L.bound(w0, up.reshape(up.shape[0], -1), down.reshape(down.shape[0], -1), rs, NET_SCALE, got, dtype)
        assert bool(((got - want[n + ".weight"].reshape(got.shape)).abs() <= bnd).all()), n


@gpu
def test_no_packed_copy_survives_a_merge(dev, net_ref):
    """Both executors run BEFORE the adapter arrives (every packed copy exists), then with it; a fresh UNet that received the
    merged parameters through load_state_dict must give the same bits."""
    from uni_renderer_amd.fused import GroupedDualStreamStep

    oracle, inputs, (sd, alphas, spec), _ = net_ref
    unet, enc, dec = build_product_from_oracle(*oracle, torch.float16, dev)
    g = [t.to(dev) for t in inputs]
    grouped = GroupedDualStreamStep(unet, enc, dec)
    with torch.no_grad():
        before = (product_step(unet, enc, dec, *g), grouped(*g))
        unet.load_attn_procs(sd, network_alphas=alphas)
        unet.fuse_lora(NET_SCALE)
        eager, fused = product_step(unet, enc, dec, *g), grouped(*g)
        fresh = build_product_from_oracle(*oracle, torch.float16, dev)[0]
        fresh.load_state_dict(unet.state_dict())  # state_dict() of a model with a merged adapter: the merged weights
        eager2, fused2 = product_step(fresh, enc, dec, *g), GroupedDualStreamStep(fresh, enc, dec)(*g)
    for k in ("img_pred", "attr_pred"):
        assert torch.equal(eager[k], eager2[k]) and torch.equal(fused[k], fused2[k]), k
    assert rel_l2(eager["img_pred"], before[0]["img_pred"]) > 3e-2 and rel_l2(fused["img_pred"], before[1]["img_pred"]) > 3e-2


def _pipe(dev, seed=21):
    from uni_renderer_amd.pipeline import UniRendererPipeline

    oracle = O.build_triplet(O.TINY_CONFIG, seed=seed)
    unet, enc, dec = build_product_from_oracle(*oracle, torch.float16, dev)
    pipe = UniRendererPipeline(unet=unet, controlnet=enc, controldec=dec)
    pipe.set_progress_bar_config(disable=True)
    pipe.use_hip_graph = True
    g = torch.Generator().manual_seed(5)
    ehs = torch.randn(1, 77, 64, generator=g) * 0.5
    attr = torch.randn(2, 28, 16, 16, generator=g)
    noise = torch.randn(2, 4, 16, 16, generator=g)
    kw = dict(prompt_embeds=ehs.to(dev).half(), attr_latents=attr.to(dev), latents=noise, num_inference_steps=3,
              guidance_scale=0.0, output_type="latent")
    return pipe, oracle, kw


@gpu
def test_pipeline_round_trip_through_scales_fuse_and_unload(dev):
    pipe, oracle, kw = _pipe(dev)
    run = lambda **extra: pipe.mask2image_3mod_albedo(**kw, **extra).clone()
    before = {k: v.detach().clone() for k, v in pipe.unet.state_dict().items()}
    sd, alphas, _ = L.make_adapter(oracle[0], seed=ADAPTER_SEED, prefix="unet.")
    a = run()
    pipe.load_lora_weights({**sd, **{k + ".alpha": torch.tensor(v) for k, v in alphas.items()}})
    b = run()
    c = run(cross_attention_kwargs={"scale": 0.3})
    assert pipe.unet.lora_scale == 0.3
    b2 = run(cross_attention_kwargs={"scale": 1.0})
    pipe.fuse_lora(0.3)
    c2 = run(cross_attention_kwargs={"scale": 1.0})  # pinned: the per-call scale is ignored
    assert pipe.unet.lora_scale == 0.3
    pipe.unfuse_lora()
    b3 = run()
    pipe.unload_lora_weights()
    a2 = run()
    assert torch.equal(b, b2) and torch.equal(b, b3) and torch.equal(c, c2) and torch.equal(a, a2)
    assert min(rel_l2(b, a), rel_l2(c, a), rel_l2(b, c)) > 1e-2, (rel_l2(b, a), rel_l2(c, a), rel_l2(b, c))
    after = pipe.unet.state_dict()
    assert all(torch.equal(after[k].view(torch.int16), v.view(torch.int16)) for k, v in before.items())
    # the inverse-rendering entry point takes the scale as well
    g = torch.Generator().manual_seed(6)
    inv = dict(prompt_embeds=kw["prompt_embeds"], image_latents=torch.randn(2, 4, 16, 16, generator=g).to(dev),
               mask_latents=torch.randn(2, 4, 16, 16, generator=g).to(dev), latents=kw["latents"], num_inference_steps=2,
               guidance_scale=0.0, output_type="latent")
    i0 = pipe.real_image2mask_3mod_albedo(**inv)[1].clone()
    pipe.load_lora_weights(sd)
    i1 = pipe.real_image2mask_3mod_albedo(**inv, cross_attention_kwargs={"scale": 0.5})[1].clone()
    pipe.unload_lora_weights()
    i2 = pipe.real_image2mask_3mod_albedo(**inv, cross_attention_kwargs={"scale": 0.5})[1].clone()  # no adapter: accepted, no effect
    assert torch.equal(i0, i2) and rel_l2(i1, i0) > 1e-3


@gpu
def test_fresh_adapter_with_zero_up_changes_nothing(dev):
    pipe, oracle, kw = _pipe(dev, seed=22)
    a = pipe.mask2image_3mod_albedo(**kw).clone()
    sd, alphas, _ = L.make_adapter(oracle[0], seed=3, zero_up=True)
    pipe.unet.load_attn_procs(sd, network_alphas=alphas)
    b = pipe.mask2image_3mod_albedo(**kw, cross_attention_kwargs={"scale": 0.6}).clone()
    assert pipe.unet.lora_scale == 0.6 and torch.equal(a, b)


@gpu
def test_pipeline_eager_path_keeps_the_per_call_scale(dev):
    """``use_hip_graph = False``: the step-by-step eager path calls ``unet(...)`` through ``graph.dual_stream_step``.  The scale the
    entry point merged must survive those calls (a ``forward`` without kwargs would re-merge at 1.0), on every entry point."""
    pipe, oracle, kw = _pipe(dev, seed=23)
    sd, alphas, _ = L.make_adapter(oracle[0], seed=ADAPTER_SEED)
    run = lambda **extra: pipe.mask2image_3mod_albedo(**kw, **extra).clone()
    graph = {}
    pipe.use_hip_graph = True
    graph["a"] = run()
    pipe.unet.load_attn_procs(sd, network_alphas=alphas)
    graph["b"], graph["c"] = run(), run(cross_attention_kwargs={"scale": 0.3})
    pipe.unload_lora_weights()
    pipe.use_hip_graph = False
    a = run()
    pipe.unet.load_attn_procs(sd, network_alphas=alphas)
    b = run()
    assert pipe.unet.lora_scale == 1.0
    c = run(cross_attention_kwargs={"scale": 0.3})
    assert pipe.unet.lora_scale == 0.3
    assert min(rel_l2(b, a), rel_l2(c, a), rel_l2(c, b)) > 1e-2, (rel_l2(b, a), rel_l2(c, a), rel_l2(c, b))
    # the eager launches pick other tiles than the captured executors (close, not bit-equal): each eager output must lie much
    # nearer to the graph path's output at ITS scale than the three scales lie apart
    apart = min(rel_l2(b, a), rel_l2(c, a), rel_l2(c, b))
    for k, v in (("a", a), ("b", b), ("c", c)):
        print(k, rel_l2(v, graph[k]), apart)
        assert rel_l2(v, graph[k]) < 0.25 * apart, (k, rel_l2(v, graph[k]), apart)
    g = torch.Generator().manual_seed(6)
    inv = dict(prompt_embeds=kw["prompt_embeds"], image_latents=torch.randn(2, 4, 16, 16, generator=g).to(dev),
               mask_latents=torch.randn(2, 4, 16, 16, generator=g).to(dev), latents=kw["latents"], num_inference_steps=2,
               guidance_scale=0.0, output_type="latent")
    i1 = pipe.real_image2mask_3mod_albedo(**inv)[1].clone()
    i3 = pipe.real_image2mask_3mod_albedo(**inv, cross_attention_kwargs={"scale": 0.3})[1].clone()
    assert pipe.unet.lora_scale == 0.3 and rel_l2(i3, i1) > 1e-3
    m3 = pipe.image2mask_3mod_albedo(image=None, masks=None, **inv, cross_attention_kwargs={"scale": 0.3})[1]
    assert torch.equal(m3, i3) and pipe.unet.lora_scale == 0.3


@gpu
def test_serial_and_concurrent_capture_keep_the_merged_scale(dev):
    """``GraphedDualStreamStep(mode="serial")`` warms up and captures through ``unet.forward``: no merge may happen in there."""
    from uni_renderer_amd.graph import GraphedDualStreamStep

    oracle = O.build_triplet(O.TINY_CONFIG, seed=NET_SEED)
    unet, enc, dec = build_product_from_oracle(*oracle, torch.float16, dev)
    x, c, ehs, ti, ta = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=99)]
    sd, alphas, _ = L.make_adapter(oracle[0], seed=ADAPTER_SEED)
    unet.load_attn_procs(sd, network_alphas=alphas)
    with torch.no_grad():
        unet(x, ti, encoder_hidden_states=ehs, cross_attention_kwargs={"scale": 0.3})
    versions = [p._version for p in unet.parameters()]
    outs = {}
    for mode in ("grouped", "serial", "concurrent"):
        g = GraphedDualStreamStep(unet, enc, dec, 2, 16, 64, mode=mode)
        outs[mode] = g.step(x, c, ehs, ti, ta)["img_pred"].clone()
        assert unet.lora_scale == 0.3 and [p._version for p in unet.parameters()] == versions, mode
    assert rel_l2(outs["serial"], outs["concurrent"]) < 3e-3 and rel_l2(outs["serial"], outs["grouped"]) < 3e-3  # the fp16 step tolerance


@gpu
def test_outside_write_into_a_merged_weight_is_loud(dev):
    """An in-place write (load_state_dict, an optimizer step) into a parameter that holds a merged adapter makes the kept copy
    stale: the next merge or unload raises instead of silently undoing the write; ``keep_weights=True`` lets go of the adapter."""
    oracle = O.build_triplet(O.TINY_CONFIG, seed=NET_SEED)
    unet = build_product_from_oracle(*oracle, torch.float16, dev)[0]
    sd, alphas, spec = L.make_adapter(oracle[0], seed=ADAPTER_SEED)
    unet.load_attn_procs(sd, network_alphas=alphas)
    unet.fuse_lora(0.5)
    unet.unfuse_lora()                                                        # merging again and again is fine
    name = next(iter(spec))
    with torch.no_grad():
        unet.get_submodule(name).weight.mul_(1.0)
    held = unet.get_submodule(name).weight.detach().clone()
    for op in (lambda: unet.fuse_lora(0.5), unet.unload_lora):
        with pytest.raises(RuntimeError, match="written from outside"):
            op()
    unet.unload_lora(keep_weights=True)
    assert unet.lora_scale is None and torch.equal(unet.get_submodule(name).weight, held)
