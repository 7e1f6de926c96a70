"""CPU tests of training_utils.EMAModel: the decay schedule's known answers, the update bit for bit against the three-rounding
fp32 emulation of tests/util_ema.py (and against torch's own ``s.sub_(d * (s - p))``), the round trips of its state, and the
host side of the two kernels' ABI (argument errors are returned before any launch)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import util_ema as E
from util_models import O, build_product_from_oracle

_P = 0x7f0000001000  # a non-null, 16-byte aligned dummy address: the host never dereferences the pointers of an item


def _ema(params, **kw):
    from uni_renderer_amd import EMAModel

    return EMAModel(params, **kw)


def _params(shapes, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(scale * torch.randn(s, generator=g)) for s in shapes]


def test_get_decay_known_answers():
    e = _ema([])
    assert [e.get_decay(s) for s in (0, 1)] == [0.0, 0.0]  # step <= update_after_step + 1
    assert [e.get_decay(s) for s in (2, 3, 4)] == [2 / 11, 3 / 12, 4 / 13]
    assert e.get_decay(10 ** 9) == 0.9999 and _ema([], decay=0.5).get_decay(11) == 0.5  # min(., decay): 11 / 20 > 0.5
    assert _ema([], min_decay=0.3).get_decay(2) == 0.3 and _ema([], min_decay=0.3).get_decay(1) == 0.0  # max(., min_decay), k > 0 only
    late = _ema([], update_after_step=5)
    assert [late.get_decay(s) for s in (5, 6, 7, 8)] == [0.0, 0.0, 2 / 11, 3 / 12]
    w = _ema([], use_ema_warmup=True)  # inv_gamma 1, power 2 / 3
    assert w.get_decay(1) == 0.0
    assert abs(w.get_decay(2) - 0.37003947505256) < 1e-14 and w.get_decay(2) == 1 - 2 ** (-2 / 3)
    assert abs(w.get_decay(8) - 0.75) < 1e-15  # k = 7: 1 - 8 ** (-2 / 3)
    w2 = _ema([], use_ema_warmup=True, inv_gamma=2.0, power=1.0, update_after_step=3)
    assert w2.get_decay(4) == 0.0 and w2.get_decay(6) == 1 - 1 / (1 + 2 / 2.0)
    for kw in (dict(), dict(use_ema_warmup=True), dict(decay=0.7, min_decay=0.2, update_after_step=2), dict(use_ema_warmup=True, power=0.75, inv_gamma=3.0)):
        e = _ema([], **kw)
        assert [e.get_decay(s) for s in range(40)] == [E.get_decay(s, **kw) for s in range(40)]
    for bad in (dict(decay=1.5), dict(min_decay=-0.1), dict(inv_gamma=0.0)):
        with pytest.raises(ValueError):
            _ema([], **bad)


@pytest.mark.parametrize("late", [100, 12345, 10 ** 6])
def test_step_is_the_three_rounding_emulation_bit_for_bit(late):
    """100,003 N(0, 1) * 3 elements.  Steps 2 to 5 are where a contraction of d * t and s - u into one fma would show (a third
    of the elements; at step 1 d = 1 and d * t is exact, at a late step d is small and few elements differ): the first five
    steps are checked every time."""
    n = 100003
    p, = _params([(n,)], 1)
    g = torch.Generator().manual_seed(2)
    s0 = 3.0 * torch.randn(n, generator=g)
    e = _ema([p])
    e.shadow_params[0].copy_(s0)
    s, t = E.widen(s0), s0.clone()
    for step in list(range(1, 6)) + [late]:
        if step == late:
            e.optimization_step = late - 1
        with torch.no_grad():
            p.copy_(3.0 * torch.randn(n, generator=g))
        e.step([p])
        d = E.one_minus_decay32(step)
        want, fused = E.emulate32(s, E.widen(p), d), E.contracted32(s, E.widen(p), d)
        got = E.widen(e.shadow_params[0])
        assert e.optimization_step == step and e.cur_decay_value == E.get_decay(step)
        assert np.array_equal(got, want), (step, int((got != want).sum()))
        t.sub_(torch.tensor(float(d)) * (t - p.detach()))  # diffusers' line
        assert np.array_equal(got, E.widen(t)), step
        differs = int((fused != want).sum())
        assert differs > (10000 if 2 <= step <= 5 else 0 if step > 5 else -1), (step, differs)  # the data would see a contraction
        err = np.abs(got.astype(np.float64) - E.definition64(s, E.widen(p), d))
        assert np.all(err <= E.bound64(s, E.widen(p), d)), step
        s = got


def test_sixteen_bit_parameters_keep_fp32_shadows():
    for dt in (torch.float16, torch.bfloat16):
        p = torch.nn.Parameter(_params([(1000,)], 3)[0].detach().to(dt))
        e = _ema([p])
        assert e.shadow_params[0].dtype == torch.float32 and torch.equal(e.shadow_params[0], p.detach().float())
        s = E.widen(e.shadow_params[0])
        for step in range(1, 4):
            with torch.no_grad():
                p.add_(1.0)
            e.step([p])
            s = E.emulate32(s, E.widen(p), E.one_minus_decay32(step))
            assert np.array_equal(E.widen(e.shadow_params[0]), s), (dt, step)


def test_frozen_parameter_is_copied_not_averaged():
    a, b = _params([(257,), (33, 3)], 4)
    b.requires_grad_(False)
    e = _ema([a, b])
    s = [E.widen(x) for x in e.shadow_params]
    for step in range(1, 4):
        with torch.no_grad():
            a.mul_(1.5)
            b.add_(2.0)
        e.step([a, b])
        s = E.replay(s, [E.widen(a), E.widen(b)], step, requires_grad=[True, False])
        assert np.array_equal(E.widen(e.shadow_params[0]), s[0])
        assert torch.equal(e.shadow_params[1], b) and np.array_equal(E.widen(b), s[1])
    assert not torch.equal(e.shadow_params[0], a.detach())


def test_argument_errors():
    ps = _params([(4, 5), (7,)], 5)
    e = _ema(ps)
    with pytest.raises(ValueError, match="1 parameters for 2 shadows"):
        e.step(ps[:1])
    with pytest.raises(ValueError, match="parameter 1 has shape"):
        e.step([ps[0], torch.nn.Parameter(torch.zeros(8))])
    with pytest.raises(ValueError):
        e.copy_to(ps + ps)
    with pytest.raises(RuntimeError, match="store"):
        e.restore(ps)
    with pytest.raises(NotImplementedError):
        e.to(dtype=torch.float16)
    with pytest.raises(ValueError, match="model_cls"):
        e.save_pretrained("/nonexistent")
    assert e.optimization_step == 0 and e.cur_decay_value is None  # nothing above counted as a step
    with pytest.raises(ValueError, match="shadow_params"):
        e.load_state_dict(dict(shadow_params=[torch.zeros(4, 5)]))
    with pytest.raises(ValueError, match="Invalid decay"):
        e.load_state_dict(dict(decay="0.5"))


def test_state_dict_round_trip_is_in_place():
    ps = _params([(31,), (8, 9)], 6)
    e = _ema(ps, decay=0.99, min_decay=0.1, update_after_step=1, use_ema_warmup=True, inv_gamma=2.0, power=0.75)
    for _ in range(4):
        with torch.no_grad():
            for p in ps:
                p.add_(0.5)
        e.step(ps)
    sd = e.state_dict()
    assert set(sd) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"}
    assert (sd["decay"], sd["min_decay"], sd["optimization_step"], sd["update_after_step"], sd["use_ema_warmup"], sd["inv_gamma"],
            sd["power"]) == (0.99, 0.1, 4, 1, True, 2.0, 0.75)
    kept = [s.clone() for s in sd["shadow_params"]]
    with torch.no_grad():
        ps[0].add_(1.0)
    e.step(ps)
    assert all(torch.equal(a, b) for a, b in zip(sd["shadow_params"], kept))  # a state dict does not follow later steps
    after5 = [s.clone() for s in e.shadow_params]

    other = _ema(_params([(31,), (8, 9)], 7))
    addr = [s.data_ptr() for s in other.shadow_params] + [other._step.data_ptr(), other._one_minus_decay.data_ptr(), other._cur_decay.data_ptr()]
    other.load_state_dict(sd)
    assert addr == [s.data_ptr() for s in other.shadow_params] + [other._step.data_ptr(), other._one_minus_decay.data_ptr(),
                                                                 other._cur_decay.data_ptr()]
    assert other.optimization_step == 4 and other.cur_decay_value == e.get_decay(4)
    assert all(torch.equal(a, b) for a, b in zip(other.shadow_params, kept))
    back = other.state_dict()
    assert {k: v for k, v in back.items() if k != "shadow_params"} == {k: v for k, v in sd.items() if k != "shadow_params"}
    other.step(ps)  # continues exactly where the saved one did
    assert other.optimization_step == 5 and all(torch.equal(a, b) for a, b in zip(other.shadow_params, after5))


def test_store_copy_to_restore():
    ps = _params([(65,), (3, 4, 5)], 8)
    e = _ema(ps)
    for _ in range(3):
        with torch.no_grad():
            for p in ps:
                p.mul_(0.9)
        e.step(ps)
    orig = [p.detach().clone() for p in ps]
    versions = [p._version for p in ps]
    e.store(ps)
    e.copy_to(ps)
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, e.shadow_params)) and not torch.equal(ps[0].detach(), orig[0])
    assert all(p._version > v for p, v in zip(ps, versions))  # packed copies and captured graphs are keyed by it
    versions = [p._version for p in ps]
    e.restore(ps)
    assert all(torch.equal(p.detach(), o) for p, o in zip(ps, orig)) and all(p._version > v for p, v in zip(ps, versions))
    assert e.temp_stored_params is None


def _tiny_unet(seed=5):
    return build_product_from_oracle(*O.build_triplet(O.TINY_CONFIG, seed=seed))[0]


def test_save_pretrained_from_pretrained_on_a_tiny_unet(tmp_path):
    from uni_renderer_amd import EMAModel, UNet2DConditionModel

    unet = _tiny_unet()
    unet.requires_grad_(True)
    ps = list(unet.parameters())
    e = EMAModel(ps, decay=0.999, min_decay=0.05, update_after_step=1, use_ema_warmup=True, inv_gamma=1.5, power=0.8,
                 model_cls=UNet2DConditionModel, model_config=unet.config)
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        with torch.no_grad():
            for p in ps:
                p.add_(0.01 * torch.randn(p.shape, generator=g))
        e.step(ps)
    plain = str(tmp_path / "plain")
    unet.save_pretrained(plain)
    path = str(tmp_path / "unet_ema")
    e.save_pretrained(path)
    cfg, cfg_plain = json.load(open(os.path.join(path, "config.json"))), json.load(open(os.path.join(plain, "config.json")))
    scalars = dict(decay=0.999, min_decay=0.05, optimization_step=3, update_after_step=1, use_ema_warmup=True, inv_gamma=1.5, power=0.8)
    assert {k: cfg[k] for k in scalars} == scalars
    assert {k: v for k, v in cfg.items() if k not in scalars} == cfg_plain  # a model without EMA keys is written as before
    assert UNet2DConditionModel.load_config(plain, return_unused_kwargs=True) == (cfg_plain, {})
    back = EMAModel.from_pretrained(path, UNet2DConditionModel)
    assert {k: v for k, v in back.state_dict().items() if k != "shadow_params"} == scalars
    assert len(back.shadow_params) == len(ps) and all(torch.equal(a, b) for a, b in zip(back.shadow_params, e.shadow_params))
    assert back.model_cls is UNet2DConditionModel and back.cur_decay_value == e.get_decay(3)
    loaded = UNet2DConditionModel.from_pretrained(path)  # ... and it is an ordinary model folder holding the averaged weights
    assert all(torch.equal(a, b) for a, b in zip(loaded.parameters(), e.shadow_params))


def test_lora_parameters_can_be_averaged():
    unet = _tiny_unet()
    unet.requires_grad_(False)
    unet.add_adapter(rank=4, generator=torch.Generator().manual_seed(1))
    lp = unet.lora_parameters()
    assert lp and all(p.requires_grad for p in lp)
    e = _ema(lp, decay=0.5)
    s = [E.widen(x) for x in e.shadow_params]
    g = torch.Generator().manual_seed(2)
    for step in range(1, 4):
        with torch.no_grad():
            for p in lp:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        e.step(unet.lora_parameters())
        s = E.replay(s, [E.widen(p) for p in lp], step, decay=0.5)
        assert all(np.array_equal(E.widen(a), b) for a, b in zip(e.shadow_params, s)), step
    assert not torch.equal(e.shadow_params[1], lp[1].detach())


def test_kernel_abi_and_argument_errors_without_a_gpu():
    from uni_renderer_amd import _lib

    lib, BAD = _lib.load(), _lib.ABI.UR_E_BADARG
    I64P = ctypes.POINTER(ctypes.c_int64)
    assert _lib.SYMBOLS["ur_ema_multi"] == (ctypes.c_int, [I64P, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SYMBOLS["ur_ema_advance"] == (ctypes.c_int, [I64P, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                             ctypes.c_void_p, ctypes.c_void_p])
    assert (lib.ur_ema_multi_max(), lib.ur_ema_item_words()) == (64, 4)
    B = lib.ur_ema_block_elems()
    assert B > 0 and B % 1024 == 0  # whole 16-byte groups of 256 threads: a workgroup's first element keeps the tensor's alignment

    def table(rows):
        return (ctypes.c_int64 * (4 * len(rows)))(*(w for r in rows for w in r))

    good = (_P, _P + 4096, 100, _lib.ABI.UR_DT_F32)
    for rows in ([(0,) + good[1:]], [(good[0], 0) + good[2:]], [good[:2] + (0, good[3])], [good[:2] + (-5, good[3])],
                 [good[:3] + (7,)], [good[:3] + (0x200,)], [(_P + 2,) + good[1:]], [(good[0], _P + 1, 100, _lib.ABI.UR_DT_F16)],
                 [good, (0,) + good[1:]], [good] * 65):
        assert lib.ur_ema_multi(table(rows), len(rows), _P, None) == BAD, rows[-1]
    assert lib.ur_ema_multi(table([good]), 0, _P, None) == BAD and lib.ur_ema_multi(None, 1, _P, None) == BAD
    assert lib.ur_ema_multi(table([good]), 1, None, None) == BAD
    sched = (ctypes.c_double * 4)(1.0, 2 / 3, 0.0, 0.9999)
    step = ctypes.cast(_P, I64P)
    assert lib.ur_ema_advance(None, 0, 0, sched, _P, _P, None) == BAD and lib.ur_ema_advance(step, 0, 0, None, _P, _P, None) == BAD
    assert lib.ur_ema_advance(step, 0, 0, sched, None, _P, None) == BAD and lib.ur_ema_advance(step, 0, 0, sched, _P, None, None) == BAD
    for bad in ((0.0, 1.0, 0.0, 0.5), (1.0, float("nan"), 0.0, 0.5), (1.0, 1.0, -0.1, 0.5), (1.0, 1.0, 0.0, 1.5)):
        assert lib.ur_ema_advance(step, 0, 0, (ctypes.c_double * 4)(*bad), _P, _P, None) == BAD, bad
