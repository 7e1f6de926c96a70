"""CPU tests of the LoRA surface: key mapping of the three formats, rejected inputs, multi-adapter assembly, which classes
carry the loader, the item table and the launcher's argument checks (no device is touched), and that the adapters the GPU
tests use move the oracle's output."""
import ctypes

import pytest
import torch

import util_lora as L
from conftest import rel_l2
from util_models import O, build_product_from_oracle

_P = 0x7f0000001000  # a non-null, 16-byte aligned dummy address: the host never dereferences the pointers of an item


def _unet():
    import uni_renderer_amd as U

    return U.UNet2DConditionModel(**dict(O.TINY_CONFIG))


def test_three_key_formats_map_onto_the_unet_modules():
    from uni_renderer_amd import lora

    unet = _unet()
    sd, alphas, spec = L.make_adapter(unet, seed=1)
    kinds = L.targets(unet)
    assert set(kinds) == set(L.KINDS)                                       # the tiny UNet has every kind of target
    assert any(".processor.to_out_lora.down.weight" in k for k in sd)       # legacy
    assert any(".attn2.to_k.lora_A.weight" in k for k in sd) and any(".lora_B.weight" in k for k in sd)  # PEFT
    assert any(".ff.net.0.proj.lora.down.weight" in k for k in sd)          # current diffusers
    for prefix in ("", "unet."):
        sd_p = {prefix + k: v for k, v in sd.items()}
        al_p = {prefix + k: v for k, v in alphas.items()}
        parsed = lora.parse_adapter(unet, sd_p, al_p)
        assert set(parsed) == set(spec) and len(parsed) == sum(len(v) for v in kinds.values())
        for n, (down, up, factor) in spec.items():
            pd, pu, pf = parsed[n]
            w = unet.get_submodule(n).weight
            assert pd.dtype == pu.dtype == torch.float32
            assert pd.shape == (down.shape[0], w[0].numel()) and pu.shape == (w.shape[0], down.shape[0])
            assert torch.equal(pd, down.reshape(down.shape[0], -1)) and torch.equal(pu, up.reshape(up.shape[0], -1))
            assert pf == factor                                              # alpha / rank, or 1 without an alpha
    # alphas may also ride inside the file as `<key>.alpha`
    name = next(iter(alphas))
    sd_a = dict(sd)
    sd_a["unet." + name + ".alpha"] = torch.tensor(alphas[name])
    parsed = lora.parse_adapter(unet, sd_a, {k: v for k, v in alphas.items() if k != name})
    assert parsed[name][2] == spec[name][2]


def test_rejected_inputs_name_the_offending_key():
    from uni_renderer_amd import lora

    unet = _unet()
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    conv = "down_blocks.0.resnets.0.conv1"
    ok = {q + ".lora.down.weight": torch.zeros(4, 64), q + ".lora.up.weight": torch.zeros(64, 4)}
    lora.parse_adapter(unet, ok)
    cases = {
        "lora_unet_down_blocks_0_attentions_0_proj_in.lora_down.weight": torch.zeros(4, 64),          # kohya
        "down_blocks.9.attentions.0.proj_in.lora.down.weight": torch.zeros(4, 64),                    # no such module
        "down_blocks.0.attentions.0.norm.lora.down.weight": torch.zeros(4, 64),                       # not a Linear / Conv2d
        q + ".lora.sideways.weight": torch.zeros(4, 64),                                              # no known spelling
    }
    for key, t in cases.items():
        with pytest.raises(ValueError) as e:
            lora.parse_adapter(unet, {**ok, key: t})
        assert key in str(e.value), key
    bad_shapes = [
        ({q + ".lora.down.weight": torch.zeros(4, 65), q + ".lora.up.weight": torch.zeros(64, 4)}, q + ".lora.down.weight"),
        ({q + ".lora.down.weight": torch.zeros(4, 64), q + ".lora.up.weight": torch.zeros(64, 5)}, q + ".lora.up.weight"),
        ({q + ".lora.down.weight": torch.zeros(4, 64), q + ".lora.up.weight": torch.zeros(63, 4)}, q + ".lora.up.weight"),
        ({q + ".lora.down.weight": torch.zeros(4, 64)}, q + ".lora.down.weight"),                   # a factor alone
        ({conv + ".lora.down.weight": torch.zeros(4, 64, 1, 1), conv + ".lora.up.weight": torch.zeros(64, 4, 1, 1)},
         conv + ".lora.down.weight"),                                                                 # 1x1 down on a 3x3 conv
        ({conv + ".lora.down.weight": torch.zeros(4, 32, 3, 3), conv + ".lora.up.weight": torch.zeros(64, 4, 1, 1)},
         conv + ".lora.down.weight"),
    ]
    for sd, key in bad_shapes:
        with pytest.raises(ValueError) as e:
            lora.parse_adapter(unet, sd)
        assert key in str(e.value), key
    with pytest.raises(ValueError, match="no_such.alpha"):
        lora.parse_adapter(unet, ok, {"no_such.alpha": 4.0})
    # a conv adapter in the module's own kernel size is fine
    lora.parse_adapter(unet, {conv + ".lora.down.weight": torch.zeros(4, 64, 3, 3), conv + ".lora.up.weight": torch.zeros(64, 4, 1, 1)})


def test_several_adapters_concatenate_along_r_with_their_weights():
    unet = _unet()
    sd_a, al_a, spec_a = L.make_adapter(unet, seed=2, rank=3)
    q = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q"
    conv = "up_blocks.1.resnets.0.conv1"
    wq, wc = unet.get_submodule(q).weight, unet.get_submodule(conv).weight
    g = torch.Generator().manual_seed(3)
    sd_b = {q + ".lora_A.weight": torch.randn(5, wq.shape[1], generator=g), q + ".lora_B.weight": torch.randn(wq.shape[0], 5, generator=g),
            "unet." + conv + ".lora.down.weight": torch.randn(2, *wc.shape[1:], generator=g),
            "unet." + conv + ".lora.up.weight": torch.randn(wc.shape[0], 2, 1, 1, generator=g)}
    unet.load_attn_procs(sd_a, network_alphas=al_a, adapter_name="a")
    unet.load_attn_procs(sd_b, network_alphas={q: 10.0}, adapter_name="b")
    assert unet.lora_scale is None                                             # on the CPU nothing is merged yet
    with pytest.raises(ValueError, match="already in use"):
        unet.load_attn_procs(sd_b, adapter_name="b")
    st = unet._lora
    up, down, rscale = st.assembled()[q]
    ra = spec_a[q][0].shape[0]
    assert up.shape == (wq.shape[0], ra + 5) and down.shape == (ra + 5, wq.shape[1]) and rscale.shape == (ra + 5,)
    assert torch.equal(down[:ra], spec_a[q][0]) and torch.equal(down[ra:], sd_b[q + ".lora_A.weight"])
    assert torch.equal(up[:, :ra], spec_a[q][1]) and torch.equal(up[:, ra:], sd_b[q + ".lora_B.weight"])
    assert rscale.tolist() == [spec_a[q][2]] * ra + [2.0] * 5                   # alpha / rank = 10 / 5
    unet.set_adapters(["b", "a"], [0.25, 3.0])                                  # order and weights follow the call
    up, down, rscale = st.assembled()[q]
    assert torch.equal(down[:5], sd_b[q + ".lora_A.weight"]) and torch.equal(up[:, 5:], spec_a[q][1])
    assert rscale.tolist() == [0.5] * 5 + [3.0 * spec_a[q][2]] * ra
    upc, downc, rsc = st.assembled()[conv]
    rc = spec_a[conv][0].shape[0]
    assert downc.shape == (2 + rc, wc[0].numel()) and torch.equal(downc[:2], sd_b["unet." + conv + ".lora.down.weight"].reshape(2, -1))
    assert rsc.tolist() == [0.25] * 2 + [3.0 * spec_a[conv][2]] * rc
    unet.set_adapters("b")                                                      # modules only `a` touches fall back to base
    only_a = next(n for n in spec_a if n not in (q, conv))
    assert st.assembled()[only_a] is None and st.assembled()[q][2].tolist() == [2.0] * 5
    with pytest.raises(ValueError, match="not loaded"):
        unet.set_adapters(["c"])
    with pytest.raises(ValueError):
        unet.set_adapters(["a", "b"], [1.0])
    # the float64 reference of the assembled factors is the sum of the adapters' updates
    unet.set_adapters(["a", "b"], [1.0, 0.5])
    up, down, rscale = st.assembled()[q]
    got, _ = L.ref_merge(wq.detach(), up, down, rscale, 0.7)
    spec_b = {q: (sd_b[q + ".lora_A.weight"], sd_b[q + ".lora_B.weight"], 2.0)}
    want = L.merged_weights(unet, [(spec_a, 1.0), (spec_b, 0.5)], 0.7)[q + ".weight"]
    assert float((got - want).abs().max()) < 1e-12
    unet.unload_lora()
    assert unet._lora is None and unet.lora_scale is None
    with pytest.raises(ValueError, match="no LoRA adapter"):
        unet.fuse_lora(0.5)


def test_surface_is_on_the_unet_and_the_pipeline_only():
    import uni_renderer_amd as U
    from uni_renderer_amd import lora
    from uni_renderer_amd.pipeline import UniRendererPipeline

    for name in ("load_attn_procs", "fuse_lora", "unfuse_lora", "unload_lora", "set_adapters", "lora_scale"):
        assert hasattr(U.UNet2DConditionModel, name), name
        for cls in (U.AttributeEncoderModel, U.AttributeDecoderModel, U.ControlNetModel):
            assert not hasattr(cls, name), (cls.__name__, name)
    assert isinstance(U.UNet2DConditionModel.lora_scale, property) and U.UNet2DConditionModel.lora_scale.fset is None
    for name in ("load_lora_weights", "unload_lora_weights", "fuse_lora", "unfuse_lora"):
        assert callable(getattr(UniRendererPipeline, name)), name
    assert lora.scale_of(None) is None and lora.scale_of({"scale": 0.3}) == 0.3 and lora.scale_of({}) is None
    with pytest.raises(NotImplementedError, match="gligen"):
        lora.scale_of({"scale": 1.0, "gligen": {}})
    # every network refuses any other key before it computes anything and lets a scale-only dict through: on the CPU the
    # accepted call then stops at the next check (fp32 parameters have no compute dtype; the decoder's mandatory residual)
    unet_o, enc_o, dec_o = O.build_triplet(O.TINY_CONFIG, seed=5)
    unet, enc, dec = build_product_from_oracle(unet_o, enc_o, dec_o)
    cn = U.ControlNetModel.from_unet(unet)
    x, c, ehs, ti, ta = O.make_inputs(1, 16, 64, seed=4)
    calls = [
        (lambda kw: enc(x, ta, encoder_hidden_states=ehs, controlnet_cond=c, return_dict=False, cross_attention_kwargs=kw), RuntimeError),
        (lambda kw: unet(x, ti, encoder_hidden_states=ehs, return_dict=False, cross_attention_kwargs=kw), RuntimeError),
        (lambda kw: cn(x, ti, encoder_hidden_states=ehs, controlnet_cond=torch.zeros(1, 3, 128, 128), return_dict=False,
                       cross_attention_kwargs=kw), RuntimeError),
        (lambda kw: dec(sample=x, down_block_res_samples=(x,), timestep=ta, encoder_hidden_states=ehs, return_dict=False,
                        cross_attention_kwargs=kw), ValueError),
    ]
    with torch.no_grad():
        for call, accepted_stops_at in calls:
            with pytest.raises(NotImplementedError, match="gligen"):
                call({"gligen": 1})
            for kw in ({"scale": 0.5}, None):
                with pytest.raises(accepted_stops_at) as e:
                    call(kw)
                assert not isinstance(e.value, NotImplementedError)


def test_pipeline_forwards_unet_keys_and_refuses_the_text_encoder(tmp_path):
    from safetensors.torch import save_file

    from uni_renderer_amd.pipeline import UniRendererPipeline

    unet = _unet()
    pipe = UniRendererPipeline(unet=unet)
    sd, alphas, spec = L.make_adapter(unet, seed=4, prefix="unet.")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "pytorch_lora_weights.safetensors"))
    pipe.load_lora_weights(str(tmp_path), adapter_name="file")                 # a directory holding the default name
    assert set(unet._lora.adapters["file"]) == set(spec)
    pipe.load_lora_weights(str(tmp_path / "pytorch_lora_weights.safetensors"), adapter_name="path")
    pipe.load_lora_weights(sd, adapter_name="dict")
    assert unet._lora.active == ["file", "path", "dict"]
    with pytest.raises(NotImplementedError, match="text_encoder.text_model"):
        pipe.load_lora_weights({**sd, "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight": torch.zeros(4, 8)})
    with pytest.raises(FileNotFoundError):
        pipe.load_lora_weights(str(tmp_path / "missing"))
    pipe.unload_lora_weights()
    assert unet._lora is None
    # merging has no CPU fallback, and the differentiable forward refuses a loaded adapter
    unet.load_attn_procs(sd)
    x, c, ehs, ti, ta = O.make_inputs(1, 16, 64, seed=4)
    with pytest.raises(NotImplementedError, match="LoRA"):
        unet(x, ti, encoder_hidden_states=ehs)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        unet(x, ti, encoder_hidden_states=ehs, cross_attention_kwargs={"scale": 0.5})


def test_item_table_and_limits():
    """The items of ur_lora_merge_multi are a host table of nine int64_t words (the header's struct and constant census stays
    as tests/test_host_cpu.py pins it); the limits are host calls."""
    import struct

    from uni_renderer_amd import _lib, lora

    lib = _lib.load()
    assert lib.ur_abi_version() == _lib.ABI_VERSION
    assert lib.ur_lora_item_words() == lora.ITEM_WORDS == 9
    assert lora.multi_max() == lib.ur_lora_multi_max() >= 16 and lora.max_rank() == lib.ur_lora_max_rank() >= 256
    assert _lib.SYMBOLS["ur_lora_merge_multi"] == (ctypes.c_int, [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int, ctypes.c_void_p])
    base, w = torch.zeros(6, 10, dtype=torch.float16), torch.zeros(6, 2, 5, dtype=torch.float16)
    up, down, rs = torch.zeros(6, 3), torch.zeros(3, 10), torch.zeros(3)
    rows = [(base, w, up, down, rs, -0.5), (base, w, up, down, None, 2.0), (base, w, None, None, None, 1.0)]
    (t0, k0), (t1, k1) = lora.item_tables(rows, 2)                              # chunked by the limit handed in
    assert (k0, k1) == (2, 1) and len(t0) == 18 and len(t1) == 9
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    assert list(t0[:9]) == [base.data_ptr(), w.data_ptr(), up.data_ptr(), down.data_ptr(), rs.data_ptr(), 6, 10, 3, bits(-0.5)]
    assert list(t0[9:]) == [base.data_ptr(), w.data_ptr(), up.data_ptr(), down.data_ptr(), 0, 6, 10, 3, bits(2.0)]
    assert list(t1) == [base.data_ptr(), w.data_ptr(), 0, 0, 0, 6, 10, 0, bits(1.0)]


_GOOD = dict(base=_P, w=_P + 0x1000, up=_P + 0x2000, down=_P + 0x3000, rscale=0, N=8, K=36, R=4, scale=0x3F800000)
_WORD = {k: i for i, k in enumerate(_GOOD)}


def _items(n, **kw):
    arr = (ctypes.c_int64 * (9 * n))(*(list({**_GOOD, **kw}.values()) * n))
    return arr


def _set(arr, i, **kw):
    for k, v in kw.items():
        arr[9 * i + _WORD[k]] = v


def test_launcher_rejects_bad_items_without_gpu():
    from uni_renderer_amd import _lib, lora

    fn, A = _lib.load().ur_lora_merge_multi, _lib.ABI
    nmax = lora.multi_max()
    assert fn(_items(1), 0, 0, None) == A.UR_E_BADARG
    assert fn(_items(1), -1, 0, None) == A.UR_E_BADARG
    assert fn(None, 1, 0, None) == A.UR_E_BADARG
    assert fn(_items(nmax + 1), nmax + 1, 0, None) == A.UR_E_BADARG
    for dtype in (-1, 3, 7):
        assert fn(_items(1), 1, dtype, None) == A.UR_E_BADARG
    spoils = [dict(base=0), dict(w=0), dict(up=0), dict(down=0), dict(N=0), dict(N=-3), dict(K=0), dict(K=-1), dict(R=-1),
              dict(w=_P), dict(base=_P + 1), dict(up=_P + 2), dict(N=2**31), dict(K=2**32 + 36), dict(R=-2**32)]
    for dtype in (A.UR_DT_F16, A.UR_DT_BF16, A.UR_DT_F32):
        for n in (1, 3, nmax):  # the bad item is the LAST one: every item is validated
            for spoil in spoils:
                arr = _items(n)
                _set(arr, n - 1, **spoil)
                assert fn(arr, n, dtype, None) == A.UR_E_BADARG, (dtype, n, spoil)
    arr = _items(2)
    _set(arr, 1, base=_P + 2)                                                  # 2-byte aligned: fine at 16 bits, not for fp32
    assert fn(arr, 2, A.UR_DT_F32, None) == A.UR_E_BADARG
    # the rank cap, and more workgroups than one grid holds
    assert fn(_items(3, R=lora.max_rank() + 1), 3, 0, None) == A.UR_E_UNSUPPORTED
    for big in (1 << 20, 2**31, 2**40):
        arr = _items(3)
        _set(arr, 2, R=big)
        assert fn(arr, 3, 1, None) == A.UR_E_UNSUPPORTED
    assert fn(_items(nmax, N=2**31 - 1, K=2**31 - 1), nmax, 0, None) == A.UR_E_UNSUPPORTED
    arr = _items(nmax, N=2**31 - 1, K=2**31 - 1)
    _set(arr, 0, base=0)                                                       # an invalid item in front of the overflow
    assert fn(arr, nmax, 0, None) == A.UR_E_BADARG
    arr = _items(2, R=lora.max_rank() + 1)
    _set(arr, 1, K=0)                                                          # ... and behind a rank over the cap
    assert fn(arr, 2, 0, None) == A.UR_E_BADARG
    arr = _items(nmax, N=2**31 - 1, K=2**31 - 1)
    _set(arr, nmax - 1, w=0)                                                   # ... and behind the overflow: every item is checked first
    assert fn(arr, nmax, 0, None) == A.UR_E_BADARG


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_exact_problems_of_the_gpu_test_are_representable(dtype):
    """The data of tests/test_lora_gpu.py's exact test: every float64 result is a value of the dtype (checked here as well,
    where it needs no device)."""
    import test_lora_gpu as T

    for (N, K, R), scale, seed in T.exact_cases():
        base, up, down, rscale, s = L.int_problem(N, K, R, dtype, seed, scale)
        ref, _ = L.ref_merge(base, up, down, rscale, s)
        assert L.representable(ref, dtype), (N, K, R, scale)


def test_adapter_of_the_gpu_test_moves_the_oracle():
    """The oracle alone: with the magnitudes the GPU network test uses (make_adapter's default, scale 0.7) the float64-merged
    weights move img_pred by rel-L2 > 0.05 -- far above the 3e-3 / 2.5e-2 the GPU comparison allows."""
    import test_lora_gpu as T

    from uni_renderer_amd import lora

    unet_o, enc_o, dec_o = O.build_triplet(O.TINY_CONFIG, seed=T.NET_SEED)
    x, c, ehs, ti, ta = O.make_inputs(2, 16, 64, seed=99)
    sd, alphas, spec = L.make_adapter(unet_o, seed=T.ADAPTER_SEED)
    # ... with the factors as the product reads them out of the file (the oracle's modules carry the same names)
    parsed = lora.parse_adapter(build_product_from_oracle(unet_o, enc_o, dec_o)[0], sd, alphas)
    assert set(parsed) == set(spec)
    spec = {n: (down.reshape(spec[n][0].shape), up.reshape(spec[n][1].shape), f) for n, (down, up, f) in parsed.items()}
    plain = O.dual_stream_step(unet_o, enc_o, dec_o, x, c, ehs, ti, ta)
    merged = O.dual_stream_step(L.oracle_with_merged(unet_o, spec, T.NET_SCALE), enc_o, dec_o, x, c, ehs, ti, ta)
    assert rel_l2(merged["img_pred"], plain["img_pred"]) > 0.05
