"""GPU tests of the two kernels of LoRA training, per element against float64 on the host: ur_lora_grad_multi (exact on integer
data, within the derived bound on random data, guarded outputs, bit-reproducible and independent of the other items) and
ur_lora_merge_cast_multi (fp32 base -> fp16 / bf16, and bit-identical to ur_lora_merge_multi with equal dtypes)."""
import pytest
import torch

import util_lora as L
import util_lora_train as T

pytestmark = pytest.mark.gpu
SCALES = [0.5, 2.0]


def _many():
    """50 items (more than lora.multi_max(): two launches): every shape, then duplicates."""
    return [T.SHAPES[i % len(T.SHAPES)] for i in range(50)]


def _check_exact(problems, outs):
    for p, (du, dd) in zip(problems, outs):
        r_up, r_down, _, _ = T.ref_grad(*p)
        assert torch.equal(du.cpu().double(), r_up), ("d_up", tuple(p[0].shape), p[1].shape[1])
        assert torch.equal(dd.cpu().double(), r_down), ("d_down", tuple(p[0].shape), p[1].shape[1])


def _check_inputs(problems, inputs, dtype):
    for p, dev_in in zip(problems, inputs):
        want = (p[0], p[1], p[2], p[3])
        for w, g in zip(want, dev_in):
            if w is not None:
                assert torch.equal(g.cpu(), w.to(g.dtype))


@pytest.mark.parametrize("dtype", T.DW_DTYPES)
def test_grad_is_exact_on_integer_data(dev, dtype):
    """Single items, every shape: outputs between canaries; also with dw one element off the wide alignment, the outputs one
    element off theirs, and rscale = 0 (ones)."""
    from uni_renderer_amd import lora

    assert len(_many()) > lora.multi_max()
    for i, (N, K, R) in enumerate(T.SHAPES):
        for shifted in (False, True):
            p = T.int_grad_problem(N, K, R, dtype, 500 + i, SCALES[i % 2], rscale_none=shifted)
            outs, guard, inputs = T.launch_grad([p], dtype, dev, dw_offset=[1] if shifted else None, out_offset=int(shifted))
            guard.check()
            _check_exact([p], outs)
            _check_inputs([p], inputs, dtype)


@pytest.mark.parametrize("dtype", T.DW_DTYPES)
def test_grad_random_data_within_the_derived_bound(dev, dtype):
    problems = [T.rand_grad_problem(N, K, R, dtype, 600 + i, (0.5, 2.0, -1.3)[i % 3]) for i, (N, K, R) in enumerate(T.SHAPES)]
    for p in problems:  # single items
        (out,), guard, _ = T.launch_grad([p], dtype, dev)
        guard.check()
        r_up, r_down, _, _ = T.ref_grad(*p)
        b_up, b_down = T.grad_bound(*p)
        e_up, e_down = (out[0].cpu().double() - r_up).abs(), (out[1].cpu().double() - r_down).abs()
        ratio = max(float((e_up / b_up.clamp_min(1e-300)).max()), float((e_down / b_down.clamp_min(1e-300)).max()))
        print(f"{str(dtype):15s} {str(tuple(p[0].shape)):14s} R {p[1].shape[1]:3d} worst |got - ref| / bound = {ratio:.3f}")
        assert bool((e_up <= b_up).all()) and bool((e_down <= b_down).all()), (tuple(p[0].shape), ratio)


@pytest.mark.parametrize("dtype", T.DW_DTYPES)
def test_fifty_items_two_launches_exact_reproducible_and_order_independent(dev, dtype):
    shapes = _many()
    problems = [T.int_grad_problem(N, K, R, dtype, 700 + i, SCALES[i % 2], rscale_none=(i % 5 == 4)) for i, (N, K, R) in enumerate(shapes)]
    offs = [i % 4 for i in range(len(problems))]  # offsets 1 .. 3: rows of K % 4 == 0 that do not start on a 4-element boundary
    outs, guard, inputs = T.launch_grad(problems, dtype, dev, dw_offset=offs)
    guard.check()
    _check_exact(problems, outs)
    _check_inputs(problems, inputs, dtype)
    # random data: a second run and a permuted item list give the same bits per item
    rnd = [T.rand_grad_problem(N, K, R, dtype, 800 + i, 0.7) for i, (N, K, R) in enumerate(shapes)]
    first, g1, _ = T.launch_grad(rnd, dtype, dev, dw_offset=offs)
    again, g2, _ = T.launch_grad(rnd, dtype, dev, dw_offset=offs)
    g1.check()
    assert torch.equal(g1.buf.view(torch.int32), g2.buf.view(torch.int32))
    perm = torch.randperm(len(rnd), generator=torch.Generator().manual_seed(9)).tolist()
    shuffled, g3, _ = T.launch_grad([rnd[j] for j in perm], dtype, dev, dw_offset=[offs[j] for j in perm])
    g3.check()
    for pos, j in enumerate(perm):
        assert torch.equal(shuffled[pos][0].view(torch.int32), first[j][0].view(torch.int32)), ("d_up", j)
        assert torch.equal(shuffled[pos][1].view(torch.int32), first[j][1].view(torch.int32)), ("d_down", j)
    # ... and the bits of an item alone in its launch
    for j in (1, 3, 7, 47):
        (alone,), _, _ = T.launch_grad([rnd[j]], dtype, dev, dw_offset=[offs[j]])
        assert torch.equal(alone[0].view(torch.int32), first[j][0].view(torch.int32))
        assert torch.equal(alone[1].view(torch.int32), first[j][1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# ur_lora_merge_cast_multi
# ---------------------------------------------------------------------------------------------------------------------
def _launch_cast(problems, out_dtype, dev):
    from uni_renderer_amd import lora

    rows, ws, keep = [], [], []
    for base, up, down, rscale, scale in problems:
        b = base.to(dev).contiguous()
        w = torch.empty(b.shape, dtype=out_dtype, device=dev)
        dv = [None if t is None else t.to(dev).contiguous() for t in (up, down, rscale)]
        keep.append(dv)
        rows.append((b, w, dv[0], dv[1], dv[2], float(scale)))
        ws.append(w)
    lora.merge_cast_items(rows, problems[0][0].dtype, out_dtype)
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16])
def test_merge_cast_from_fp32_base(dev, out_dtype):
    """fp32 base -> half output on the shapes above: exact on integer data, within util_lora.bound (ulp of the OUT dtype) on
    random data."""
    ints = [L.int_problem(N, K, R, torch.float32, 900 + i, SCALES[i % 2]) for i, (N, K, R) in enumerate(T.SHAPES)]
    for p, w in zip(ints, _launch_cast(ints, out_dtype, dev)):
        ref, _ = L.ref_merge(*p)
        assert L.representable(ref, out_dtype)
        assert torch.equal(w.cpu(), ref.to(out_dtype)), tuple(p[0].shape)
    rnd = [L.rand_problem(N, K, R, torch.float32, 950 + i, (0.7, -1.3, 1.0)[i % 3]) for i, (N, K, R) in enumerate(T.SHAPES)]
    for p, w in zip(rnd, _launch_cast(rnd, out_dtype, dev)):
        ref, _ = L.ref_merge(*p)
        got = w.cpu().double()
        err, bnd = (got - ref).abs(), L.bound(*p, got, out_dtype)
        assert bool((err <= bnd).all()), (tuple(p[0].shape), float((err / bnd).max()))


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_merge_cast_with_equal_dtypes_is_the_merge(dev, dtype):
    rnd = [L.rand_problem(N, K, R, dtype, 970 + i, 0.7) for i, (N, K, R) in enumerate(T.SHAPES)] + [L.rand_problem(130, 64, 0, dtype, 99, 1.0)]
    rnd[-1] = (rnd[-1][0], None, None, None, 1.0)
    want, _ = L.launch(rnd, dtype, dev)
    got = _launch_cast(rnd, dtype, dev)
    iv = L.INT_VIEW[dtype.itemsize]
    for a, b in zip(want, got):
        assert torch.equal(a.view(iv), b.view(iv))
