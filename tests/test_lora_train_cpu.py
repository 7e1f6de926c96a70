"""CPU tests of the trainable LoRA surface: add_adapter (targets, shapes, init, refusals), registration of the factors
(parameters() sees them, state_dict() does not), save_attn_procs / load_attn_procs round trips, what the differentiable
forward refuses, and the ABI of the two kernels (argument errors are returned before any launch)."""
import ctypes
import struct

import pytest
import torch

import util_lora as L
from util_models import O, build_product_from_oracle

_P = 0x7f0000001000  # a non-null, 16-byte aligned dummy address: the host never dereferences the pointers of an item
ATTN = ("to_q", "to_k", "to_v", "to_out.0")


def _unet(seed=5):
    return build_product_from_oracle(*O.build_triplet(O.TINY_CONFIG, seed=seed))[0]


def test_add_adapter_targets_shapes_and_init():
    unet = _unet()
    keys = set(unet.state_dict())
    n_params = len(list(unet.parameters()))
    unet.add_adapter(rank=4, generator=torch.Generator().manual_seed(1))
    st = unet._lora
    want = {n for n, m in unet.named_modules() if isinstance(m, torch.nn.Linear) and any(n.endswith("." + t) for t in ATTN)}
    assert want and set(st.adapters["default"]) == want and all(".attn1." in n or ".attn2." in n for n in want)
    assert st.active == ["default"] and st.trainable == "default" and unet.lora_scale is None  # on the CPU nothing is merged
    downs = []
    for name, (down, up, factor) in st.adapters["default"].items():
        w = unet.get_submodule(name).weight
        assert down.shape == (4, w.shape[1]) and up.shape == (w.shape[0], 4) and factor == 1.0
        assert down.dtype == up.dtype == torch.float32 and down.is_contiguous() and up.is_contiguous() and down.device == w.device
        assert isinstance(down, torch.nn.Parameter) and down.requires_grad and up.requires_grad and not w.requires_grad
        assert float(up.detach().abs().max()) == 0.0
        downs.append(down.detach().reshape(-1))
    std = float(torch.cat(downs).std())
    assert abs(std - 0.25) < 0.01, std                                          # N(0, (1 / rank)^2)
    # registration: parameters() yields the factors, the checkpoint keeps its keys
    params = list(unet.parameters())
    assert len(params) == n_params + 2 * len(want)
    lp = unet.lora_parameters()
    assert len(lp) == 2 * len(want) and all(any(p is q for q in params) for p in lp)
    assert set(unet.state_dict()) == keys
    unet.load_state_dict(unet.state_dict(), strict=True)                       # ... and loads without them
    # rscale = lora_alpha / rank; a second trainable adapter and a name in use are refused
    with pytest.raises(ValueError, match="already in use"):
        unet.add_adapter(rank=2)
    with pytest.raises(ValueError, match="trainable already"):
        unet.add_adapter(rank=2, adapter_name="second")
    unet.unload_lora()
    assert unet._lora is None and len(list(unet.parameters())) == n_params and set(unet.state_dict()) == keys
    assert all(unet.get_submodule(n).weight.requires_grad for n in want)       # the flags add_adapter took are given back
    unet.add_adapter(rank=8, lora_alpha=4.0, target_modules=("to_q", "ff.net.2", "proj_in"))
    kinds = {n.rsplit(".", 1)[-1] if not n.endswith("ff.net.2") else "ff.net.2" for n in unet._lora.adapters["default"]}
    assert kinds == {"to_q", "ff.net.2", "proj_in"}
    assert all(f == 0.5 for _, _, f in unet._lora.adapters["default"].values())


def test_add_adapter_refuses_a_3x3_conv_and_an_empty_target_list():
    unet = _unet()
    with pytest.raises(ValueError, match=r"resnets\.0\.conv1"):
        unet.add_adapter(target_modules=("conv1",))
    assert unet._lora is None and "lora_factors" not in dict(unet.named_children())
    with pytest.raises(ValueError, match="name no Linear"):
        unet.add_adapter(target_modules=("no_such_module",))
    name = L.targets(unet)["conv1"][0]
    w = unet.get_submodule(name).weight
    sd = {name + ".lora.down.weight": torch.zeros(2, *w.shape[1:]), name + ".lora.up.weight": torch.zeros(w.shape[0], 2, 1, 1)}
    with pytest.raises(ValueError, match="conv1"):
        unet.load_attn_procs(sd, trainable=True)
    unet.load_attn_procs(sd)                                                   # merged (not trained), a 3x3 conv is fine


def test_save_and_load_round_trip(tmp_path):
    unet = _unet()
    unet.add_adapter(rank=3, lora_alpha=6.0, target_modules=ATTN + ("proj_in", "conv_shortcut"),
                     generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        for p in unet.lora_parameters()[1::2]:
            p.normal_(generator=torch.Generator().manual_seed(3))
    sd = unet.lora_state_dict()
    convs = [n for n in unet._lora.adapters["default"] if unet.get_submodule(n).weight.dim() == 4]
    assert convs and any(n.endswith("conv_shortcut") for n in convs)
    for n in convs:                                                             # conv factors are stored 4-D, as diffusers does
        w = unet.get_submodule(n).weight
        assert sd[n + ".lora.down.weight"].shape == (3, w.shape[1], 1, 1) and sd[n + ".lora.up.weight"].shape == (w.shape[0], 3, 1, 1)
    assert all(float(sd[n + ".alpha"]) == 6.0 for n in unet._lora.adapters["default"])
    assert set(sd) == {n + s for n in unet._lora.adapters["default"] for s in (".lora.down.weight", ".lora.up.weight", ".alpha")}
    unet.save_attn_procs(str(tmp_path))
    assert (tmp_path / "pytorch_lora_weights.safetensors").is_file()
    src = unet._lora.adapters["default"]
    for trainable in (False, True):
        fresh = _unet()
        fresh.load_attn_procs(str(tmp_path), trainable=trainable)
        got = fresh._lora.adapters["default"]
        assert set(got) == set(src)                                            # (a safetensors file keeps its keys sorted)
        for n in src:
            assert torch.equal(got[n][0], src[n][0]) and torch.equal(got[n][1], src[n][1]) and got[n][2] == src[n][2] == 2.0
            assert isinstance(got[n][0], torch.nn.Parameter) == trainable
        assert (fresh._lora.trainable == "default") == trainable
        if trainable:
            back = fresh.lora_state_dict()
            assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
            assert len(fresh.lora_parameters()) == 2 * len(src)
        else:
            with pytest.raises(ValueError, match="no trainable"):
                fresh.lora_parameters()
    # without lora_alpha no alpha key is written
    plain = _unet()
    plain.add_adapter(rank=2)
    assert not any(k.endswith(".alpha") for k in plain.lora_state_dict())
    # the other key spellings load as trainable factors too
    sd_m, alphas, spec = L.make_adapter(plain, seed=4)
    keep = {k: v for k, v in sd_m.items() if ".attn" in k}
    other = _unet()
    other.load_attn_procs({"unet." + k: v for k, v in keep.items()}, network_alphas={k: v for k, v in alphas.items() if ".attn" in k},
                          trainable=True)
    assert len(other.lora_parameters()) == len(keep)


def test_what_the_differentiable_forward_refuses():
    unet = _unet()
    x, c, ehs, ti, ta = O.make_inputs(1, 16, 64, seed=4)
    sd, alphas, _ = L.make_adapter(unet, seed=7)
    sd = {k: v for k, v in sd.items() if ".attn1.to_q" in k or ".attn1.processor.to_q" in k}
    unet.load_attn_procs(sd, adapter_name="merged")
    with pytest.raises(NotImplementedError, match="LoRA"):                     # not trainable: as before
        unet(x, ti, encoder_hidden_states=ehs)
    unet.add_adapter(rank=2, adapter_name="train")
    assert unet._lora.active == ["merged", "train"]
    with pytest.raises(ValueError, match="only active one"):
        unet(x, ti, encoder_hidden_states=ehs)
    unet.set_adapters("train")
    w = unet.get_submodule(next(iter(unet._lora.adapters["train"]))).weight
    w.requires_grad_(True)
    with pytest.raises(ValueError, match="freeze it"):
        unet(x, ti, encoder_hidden_states=ehs)


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_item_words():
    from uni_renderer_amd import _lib, lora

    lib = _lib.load()
    I64P = ctypes.POINTER(ctypes.c_int64)
    assert _lib.SYMBOLS["ur_lora_merge_cast_multi"] == (ctypes.c_int, [I64P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p])
    assert _lib.SYMBOLS["ur_lora_grad_multi"] == (ctypes.c_int, [I64P, ctypes.c_int, ctypes.c_int, ctypes.c_void_p])
    assert _lib.SYMBOLS["ur_lora_grad_item_words"] == (ctypes.c_int, [])
    assert lib.ur_lora_grad_item_words() == lora.GRAD_ITEM_WORDS == 10
    dw, up, down, rs = torch.zeros(6, 10, dtype=torch.bfloat16), torch.zeros(6, 3), torch.zeros(3, 10), torch.zeros(3)
    du, dd = torch.zeros(6, 3), torch.zeros(3, 10)
    (t0, k0), (t1, k1) = lora.grad_item_tables([(dw, up, down, rs, du, dd, -0.5), (dw, up, down, None, du, dd, 2.0),
                                                (dw, up, down, None, du, dd, 1.0)], 2)
    bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    assert (k0, k1) == (2, 1) and len(t0) == 20 and len(t1) == 10
    assert list(t0[:10]) == [dw.data_ptr(), up.data_ptr(), down.data_ptr(), rs.data_ptr(), du.data_ptr(), dd.data_ptr(), 6, 10, 3, bits(-0.5)]
    assert list(t0[10:])[3] == 0 and list(t1)[9] == bits(1.0)


_GOOD = dict(dw=_P, up=_P + 0x10000, down=_P + 0x20000, rscale=0, d_up=_P + 0x30000, d_down=_P + 0x40000, N=8, K=36, R=4,
             scale=0x3F800000)
_WORD = {k: i for i, k in enumerate(_GOOD)}
# the same item with its matrices 2^42 bytes apart: no overlap at N = 2^31 - 1 either
_FAR = {**_GOOD, **{k: _P + (i << 42) for i, k in enumerate(("dw", "up", "down", "d_up", "d_down"))}}


def _items(n, proto=_GOOD, **kw):
    return (ctypes.c_int64 * (10 * n))(*(list({**proto, **kw}.values()) * n))


def _set(arr, i, **kw):
    for k, v in kw.items():
        arr[10 * i + _WORD[k]] = v


def test_grad_launcher_rejects_bad_items_without_gpu():
    from uni_renderer_amd import _lib, lora

    fn, A = _lib.load().ur_lora_grad_multi, _lib.ABI
    nmax = lora.multi_max()
    assert fn(_items(1), 0, 0, None) == A.UR_E_BADARG
    assert fn(_items(1), -1, 0, None) == A.UR_E_BADARG
    assert fn(None, 1, 0, None) == A.UR_E_BADARG
    assert fn(_items(nmax + 1), nmax + 1, 0, None) == A.UR_E_BADARG
    for dtype in (-1, 3, 7):
        assert fn(_items(1), 1, dtype, None) == A.UR_E_BADARG
    g = _GOOD
    spoils = [dict(dw=0), dict(up=0), dict(down=0), dict(d_up=0), dict(d_down=0), dict(N=0), dict(N=-3), dict(K=0), dict(K=-1),
              dict(R=0), dict(R=-1), dict(N=2**31), dict(K=2**32 + 36), dict(R=-2**32),
              dict(dw=_P + 1), dict(up=_P + 0x10002), dict(down=_P + 0x20001), dict(rscale=_P + 0x50002), dict(d_up=_P + 0x30002),
              dict(d_down=_P + 0x40001),
              # d_up / d_down on an input (the same address, and a partial overlap), and on each other
              dict(d_up=g["up"]), dict(d_up=g["dw"]), dict(d_up=g["down"] + 64), dict(d_down=g["down"]), dict(d_down=g["dw"] + 16),
              dict(d_down=g["up"]), dict(d_down=g["d_up"]), dict(d_up=g["d_down"] + 4 * 35), dict(rscale=g["d_up"] + 8),
              dict(rscale=g["d_down"])]
    for dtype in (A.UR_DT_F16, A.UR_DT_BF16, A.UR_DT_F32):
        for n in (1, 3, nmax):  # the bad item is the LAST one: every item is validated
            for spoil in spoils:
                arr = _items(n)
                _set(arr, n - 1, **spoil)
                assert fn(arr, n, dtype, None) == A.UR_E_BADARG, (dtype, n, spoil)
    arr = _items(2)
    _set(arr, 1, dw=_P + 2)                                                    # 2-byte aligned: fine at 16 bits, not for fp32
    assert fn(arr, 2, A.UR_DT_F32, None) == A.UR_E_BADARG
    # the rank cap, and more workgroups than one grid holds
    assert fn(_items(3, R=lora.max_rank() + 1), 3, 0, None) == A.UR_E_UNSUPPORTED
    for big in (1 << 20, 2**31, 2**40):
        arr = _items(3)
        _set(arr, 2, R=big)
        assert fn(arr, 3, 1, None) == A.UR_E_UNSUPPORTED
    assert fn(_items(nmax, _FAR, N=2**31 - 1), nmax, 0, None) == A.UR_E_UNSUPPORTED
    arr = _items(nmax, _FAR, N=2**31 - 1)
    _set(arr, 0, dw=0)                                                         # an invalid item in front of the overflow
    assert fn(arr, nmax, 0, None) == A.UR_E_BADARG
    arr = _items(2, R=lora.max_rank() + 1)
    _set(arr, 1, K=0)                                                          # ... and behind a rank over the cap
    assert fn(arr, 2, 0, None) == A.UR_E_BADARG
    arr = _items(nmax, _FAR, N=2**31 - 1)
    _set(arr, nmax - 1, d_down=0)                                              # ... and behind the overflow: every item is checked first
    assert fn(arr, nmax, 0, None) == A.UR_E_BADARG


def test_merge_cast_launcher_rejects_bad_items_without_gpu():
    from uni_renderer_amd import _lib, lora

    fn, A = _lib.load().ur_lora_merge_cast_multi, _lib.ABI
    nmax = lora.multi_max()
    good = dict(base=_P, w=_P + 0x1000, up=_P + 0x2000, down=_P + 0x3000, rscale=0, N=8, K=36, R=4, scale=0x3F800000)
    word = {k: i for i, k in enumerate(good)}

    def items(n, **kw):
        return (ctypes.c_int64 * (9 * n))(*(list({**good, **kw}.values()) * n))

    assert fn(items(1), 0, 2, 0, None) == A.UR_E_BADARG and fn(None, 1, 2, 0, None) == A.UR_E_BADARG
    assert fn(items(nmax + 1), nmax + 1, 2, 0, None) == A.UR_E_BADARG
    for bad in (-1, 3, 7):
        assert fn(items(1), 1, bad, 0, None) == A.UR_E_BADARG and fn(items(1), 1, 2, bad, None) == A.UR_E_BADARG
    spoils = [dict(base=0), dict(w=0), dict(up=0), dict(down=0), dict(N=0), dict(K=-1), dict(R=-1), dict(w=_P), dict(up=_P + 2),
              dict(N=2**31), dict(w=_P + 0x1001)]
    for base_dt in (A.UR_DT_F16, A.UR_DT_BF16, A.UR_DT_F32):
        for out_dt in (A.UR_DT_F16, A.UR_DT_BF16, A.UR_DT_F32):
            for n in (1, nmax):
                for spoil in spoils:
                    arr = items(n)
                    for k, v in spoil.items():
                        arr[9 * (n - 1) + word[k]] = v
                    assert fn(arr, n, base_dt, out_dt, None) == A.UR_E_BADARG, (base_dt, out_dt, n, spoil)
    # alignment goes by side: a 2-byte aligned base is fine at 16 bits and not as fp32, whatever the output is
    assert fn(items(1, base=_P + 2), 1, A.UR_DT_F32, A.UR_DT_BF16, None) == A.UR_E_BADARG
    assert fn(items(1, w=_P + 0x1002), 1, A.UR_DT_BF16, A.UR_DT_F32, None) == A.UR_E_BADARG
    assert fn(items(3, R=lora.max_rank() + 1), 3, 2, 1, None) == A.UR_E_UNSUPPORTED
    assert fn(items(nmax, N=2**31 - 1, K=2**31 - 1), nmax, 2, 0, None) == A.UR_E_UNSUPPORTED
