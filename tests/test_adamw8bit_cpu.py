"""CPU tests of the 8-bit AdamW (ABI 17): the library's code books, the argument checks of ur_adamw8_multi (everything
returns before a launch), the constructor and state layout of optim.AdamW8bit, and the float64 restatement the GPU tests
compare against (tests/util_adamw8bit.py)."""
import ctypes

import numpy as np
import pytest
import torch

import util_adamw8bit as U
from util_models import ROOT  # noqa: F401  (puts the repository on sys.path)

HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)


def _lib_book(signed):
    from uni_renderer_amd import _lib

    out = (ctypes.c_float * 256)()
    assert _lib.load().ur_adam8_codebook(int(signed), out) == 0
    return np.frombuffer(out, dtype=np.float32).copy()


@pytest.mark.parametrize("signed", [True, False])
def test_codebook_is_the_formula_rounded_to_fp32(signed):
    from uni_renderer_amd import _lib, optim

    b = _lib_book(signed)
    assert b.shape == (256,) and np.all(np.diff(b.astype(np.float64)) > 0)
    assert np.array_equal(b.astype(np.float64), U.BOOKS[signed])  # bit for bit: both are fp32 values
    zero = 127 if signed else 0
    assert b[zero] == 0.0 and b[255] == 1.0 and b[0] == (np.float32(-0.99296875) if signed else 0.0)
    assert np.isclose(b[zero + 1], 5.5e-7 if signed else 3.25e-7, rtol=1e-6)
    if signed:
        assert np.array_equal(b[128:255], -b[126::-1])  # every magnitude with both signs; only +1 has no partner
    assert torch.equal(optim.codebook(signed), torch.from_numpy(b))
    assert _lib.load().ur_adam8_codebook(int(signed), None) == _lib.ABI.UR_E_BADARG


_P = 0x7f0000001000  # non-null, 16-byte aligned: the host never dereferences an item's pointers


def test_adamw8_multi_rejects_bad_lists_and_oversized_grids_without_gpu():
    """What test_host_cpu.py makes the other multi-tensor launchers reject, on ur_adamw8_multi."""
    from uni_renderer_amd import _lib

    lib, A = _lib.load(), _lib.ABI
    nmax, BADARG = A.UR_ADAMW_MAX_TENSORS, A.UR_E_BADARG
    assert _lib.SYMBOLS["ur_adamw8_multi"][1][0] == ctypes.POINTER(ctypes.c_int64)  # the item table: seven words per tensor
    assert lib.ur_abi_version() == 17 == _lib.ABI_VERSION
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.0, _P, None, None, None, None)
    ptrs = range(6)  # p, g, m, v, absmax_m, absmax_v; word 6 is n

    def items(n, count):
        return (ctypes.c_int64 * (7 * n))(*([_P] * 6 + [count]) * n)

    fn = lib.ur_adamw8_multi
    assert fn(items(1, 100), 0, *tail) == BADARG
    assert fn(items(1, 100), -1, *tail) == BADARG
    assert fn(items(nmax + 1, 100), nmax + 1, *tail) == BADARG
    assert fn(None, 1, *tail) == BADARG
    for n in (1, 3, nmax):  # the bad item is the LAST one
        for k in ptrs:
            arr = items(n, 100)
            arr[7 * (n - 1) + k] = 0
            assert fn(arr, n, *tail) == BADARG, (n, k)
        for bad_n in (0, -5):
            arr = items(n, 100)
            arr[7 * (n - 1) + 6] = bad_n
            assert fn(arr, n, *tail) == BADARG, (n, bad_n)
    # 2**45 elements = 2**31 workgroups of 16384: more than one grid holds, alone or behind valid small items
    assert fn(items(nmax, 2**45), nmax, *tail) == BADARG
    arr = items(nmax, 100)
    arr[7 * (nmax - 1) + 6] = 2**45
    assert fn(arr, nmax, *tail) == BADARG
    # the scalar arguments ur_adamw_multi checks
    assert fn(items(1, 100), 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, None, None, None, None) == BADARG  # no step counter
    assert fn(items(1, 100), 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, _P, None, None, None, None) == BADARG
    assert fn(items(1, 100), 1, 1e-3, 0.9, -0.1, 1e-8, 0.0, _P, None, None, None, None) == BADARG
    for f in (lib.ur_adam8_quantize, lib.ur_adam8_dequantize):
        for args in ((None, _P, _P, 10), (_P, None, _P, 10), (_P, _P, None, 10), (_P, _P, _P, 0), (_P, _P, _P, -1)):
            assert f(*args, 1, None) == BADARG


def _three_groups(cls, **kw):
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (8192, 100, 4096)]
    return ps, cls([{"params": ps[:1]}, {"params": ps[1:2], "lr": 3e-4}, {"params": ps[2:], "weight_decay": 0.0}], **kw)


def test_constructor_matches_fusedadamw():
    import uni_renderer_amd
    from uni_renderer_amd.optim import AdamW8bit, FusedAdamW

    assert uni_renderer_amd.AdamW8bit is AdamW8bit and issubclass(AdamW8bit, torch.optim.Optimizer)
    _, ref = _three_groups(FusedAdamW)
    _, opt = _three_groups(AdamW8bit)
    assert opt.defaults == ref.defaults and opt.min_8bit_size == 4096 and opt.generation == 0
    assert opt.defaults["lr"] == 1e-3 and opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-8
    assert opt.defaults["weight_decay"] == 1e-2 and opt.defaults["fused"] is True
    assert len(opt.param_groups) == 3 and opt._step_supports_amp_scaling
    for g, r in zip(opt.param_groups, ref.param_groups):
        assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in r.items() if k != "params"}
    assert opt.param_groups[1]["lr"] == 3e-4 and opt.param_groups[2]["weight_decay"] == 0.0
    p = [torch.nn.Parameter(torch.zeros(8))]
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                dict(min_8bit_size=-1)):
        with pytest.raises(ValueError):
            AdamW8bit(p, **bad)
    for switch in (dict(amsgrad=True), dict(percentile_clipping=5), dict(block_wise=False)):
        with pytest.raises(NotImplementedError):
            AdamW8bit(p, **switch)
    AdamW8bit(p, amsgrad=False, percentile_clipping=100, block_wise=True)  # the defaults, spelled out, are accepted


def test_state_bytes_and_layout():
    from uni_renderer_amd.optim import AdamW8bit

    sizes = [(4096,), (4097,), (640, 3, 3, 3), (65536,), (4095,), (320,), (1,)]
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in sizes]
    opt = AdamW8bit(ps)
    for p in ps:
        st = opt._init_state(p)
        n = p.numel()
        nbytes = sum(t.numel() * t.element_size() for k, t in st.items() if k != "step")
        if n >= 4096:
            assert nbytes == 2 * n + 8 * -(-n // 256)
            assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.uint8 and st["exp_avg"].shape == p.shape
            assert st["exp_avg_absmax"].dtype == torch.float32 and st["exp_avg_absmax"].shape == (-(-n // 256),)
            assert st["exp_avg_sq_absmax"].dtype == torch.float32 and st["exp_avg_sq_absmax"].shape == (-(-n // 256),)
            # fresh state: the zero codes, absmax 0
            assert bool((st["exp_avg"] == 127).all()) and not st["exp_avg_sq"].any()
            assert not st["exp_avg_absmax"].any() and not st["exp_avg_sq_absmax"].any()
        else:
            assert nbytes == 8 * n and set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].dtype == torch.float32
        assert st["step"].dtype == torch.float32 and st["step"].shape == ()
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "exp_avg_absmax", "exp_avg_sq_absmax"}
    assert AdamW8bit(ps[:1], min_8bit_size=10**6)._init_state(ps[0])["exp_avg"].dtype == torch.float32


# ---- the restatement itself ----
def test_restatement_edge_blocks():
    # a zero block: zero codes, absmax 0, decodes to zeros (no division happened: no nan)
    for signed in (True, False):
        c, am = U.encode(np.zeros(300), signed)
        assert np.all(c == U.ZERO_CODE[signed]) and np.all(am == 0) and np.all(U.decode(c, am, signed) == 0)
    # one non-zero: it is the block's absmax and takes the code of 1.0; the rest stay zero
    x = np.zeros(256)
    x[17] = 3.5e-4
    for signed in (True, False):
        c, am = U.encode(x, signed)
        assert am[0] == 3.5e-4 and c[17] == 255 and np.all(np.delete(c, 17) == U.ZERO_CODE[signed])
        assert np.array_equal(U.decode(c, am, signed), x)
    # all negative: there is no -1 in the signed book, the block's extreme takes code 0 = -0.99296875
    x = -np.linspace(0.5, 2.0, 256)
    c, am = U.encode(x, True)
    assert am[0] == 2.0 and c[-1] == 0 and np.all(c < 127)
    assert U.decode(c, am, True)[-1] == -2.0 * float(np.float32(0.99296875))  # the book holds fp32 values
    assert np.abs(U.decode(c, am, True) - x).max() <= 2.0 * (0.00703125 + 1e-7)
    # a v entry at 1e-8 of its block maximum: nearest is 0 (the first entry is 3.25e-7), the rule stores code 1
    v = np.full(256, 1.0)
    v[3] = 1e-8
    v[4] = 0.0
    c, am = U.encode(v, False)
    assert c[3] == 1 and c[4] == 0 and U.nearest(np.array([1e-8]), False)[0] == 0
    # a partial last block has its own absmax
    c, am = U.encode(np.r_[np.ones(256), np.full(3, 1e-3)], False)
    assert am.tolist() == [1.0, 1e-3] and np.all(c == 255)
    # nearest really is nearest (brute force), ties aside
    rng = np.random.default_rng(0)
    r = np.r_[rng.uniform(-1, 1, 2000), 10.0 ** rng.uniform(-8, 0, 2000)]
    for signed in (True, False):
        rr = r if signed else np.abs(r)
        brute = np.abs(U.BOOKS[signed][None, :] - rr[:, None]).argmin(axis=1)
        assert np.array_equal(U.nearest(rr, signed), brute)


def test_restatement_round_trip_error_on_gaussian_data():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(1 << 16)
    for signed, bound in ((True, 0.00703125), (False, 0.003515625)):  # half the widest gap of each book
        y = x if signed else x * x
        c, am = U.encode(y, signed)
        err = np.abs(U.decode(c, am, signed) - y) / np.repeat(am, 256)
        assert err.max() <= bound + 1e-7 and err.max() > 0.9 * bound  # 1e-7: the entries are fp32 roundings


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_trajectory_figures(seed):
    """20 steps on the trajectory data of the GPU test.  The issue's prototype measured rel-L2 of the displacement against fp32
    AdamW at 0.0132 (5 steps) and 0.0223 - 0.0224 (20 steps), the worst element at in-block spread exp(1.5 N) at 0.68 - 0.74
    lr t with the code-1 rule and above 1e3 lr t without it.  This generator's draws give 0.0133 - 0.0134, 0.0223 - 0.0225,
    0.64 - 0.72 and 515 - 1432: the bands below hold both."""
    p0, grads = U.trajectory_data(seed)
    ref, q = U.adamw_fp64(p0, grads, **HP), U.adamw8_trajectory(p0, grads, **HP)
    r5, r20 = U.rel_l2(q[4] - p0, ref[4] - p0), U.rel_l2(q[19] - p0, ref[19] - p0)
    print(f"seed {seed}: rel-L2 of the displacement after 5 / 20 steps: {r5:.4f} / {r20:.4f}")
    assert 0.0128 <= r5 <= 0.0137 and 0.0220 <= r20 <= 0.0228
    p0, grads = U.trajectory_data(seed, spread=1.5)
    ref = U.adamw_fp64(p0, grads, **HP)
    worst = np.abs(U.adamw8_trajectory(p0, grads, **HP)[19] - ref[19]).max() / (HP["lr"] * 20)
    plain = np.abs(U.adamw8_trajectory(p0, grads, code1_rule=False, **HP)[19] - ref[19]).max() / (HP["lr"] * 20)
    print(f"seed {seed}: worst element / (lr t): {worst:.3f} with the code-1 rule, {plain:.0f} with plain nearest rounding")
    assert 0.6 <= worst <= 0.8 and plain > 100
