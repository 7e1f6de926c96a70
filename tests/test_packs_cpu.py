"""uni_renderer_amd/packs.py on the CPU: every recipe declares exactly the parameters its build reads, the cache rebuilds on
exactly those, and every layout is the expression the call sites used to spell out (written here from the primitives
``pack_conv3x3`` / ``pack_matrix`` / ``f32`` / ``geglu_perm`` / ``pack_cond_conv3x3`` / ``tchain.pack_chain_*``, which keep their
own tests)."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from uni_renderer_amd import layers as L
from uni_renderer_amd import ops, tchain, vae
from uni_renderer_amd import packs as R
from uni_renderer_amd.layers import f32, geglu_perm, pack_cond_conv3x3, pack_conv3x3, pack_matrix

DTYPES = [torch.float16, torch.bfloat16]
CIN_PAD = 64


def _randomize(m, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.25)  # zero convs, unit gammas, zero biases: all made visible
    return m


def _cat(ts, dim=0):
    return torch.cat(list(ts), dim).contiguous()


def _cblock(conv):
    return ops.conv_cblock(conv.weight.shape[1])


def _fold_expect(cblock):
    def f(r, dt):
        w2 = pack_conv3x3(r.conv2.weight, dt, cblock=_cblock(r.conv2) if cblock else 0)
        return (torch.cat([w2, pack_matrix(r.conv_shortcut.weight, dt)], 1).contiguous(),
                f32(r.conv2.bias) + f32(r.conv_shortcut.bias))
    return f


def _geglu_expect(p, dt):
    perm = geglu_perm(p.weight.shape[0] // 2, p.weight.device)
    return pack_matrix(p.weight, dt)[perm].contiguous(), f32(p.bias)[perm].contiguous()


def _affine(n, dt):
    return f32(n.weight), f32(n.bias)


def _linear(m, dt):
    return pack_matrix(m.weight, dt), f32(m.bias)


def _matrix(m, dt):
    return pack_matrix(m.weight, dt)


def _conv(cblock, cin_pad=None):
    return lambda c, dt: (pack_conv3x3(c.weight, dt, cin_pad, cblock=_cblock(c) if cblock else 0), f32(c.bias))


def _pad_rows(t, n):
    return t if t.shape[0] == n else torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))], 0)


def _moments_expect(v, dt):
    q, e = v.quant_conv, v.encoder
    wq = q.weight.detach().float().reshape(q.weight.shape[0], -1)
    wc = torch.einsum("oi,icyx->ocyx", wq, e.conv_out.weight.detach().float())
    bc = wq @ e.conv_out.bias.detach().float() + q.bias.detach().float()
    return pack_conv3x3(wc, dt), bc.contiguous()


def _cs(t):
    return t.transformer_blocks[0].attn1.dim_head ** -0.5 * L.LOG2E


def _chain_pre_expect(t, dt):
    b = t.transformer_blocks[0]
    return tchain.pack_chain_pre(t.proj_in.weight, t.proj_in.bias, b.norm1.weight, b.norm1.bias, b.attn1.to_q.weight,
                                 b.attn1.to_k.weight, b.attn1.to_v.weight, math.sqrt(_cs(t)), dt)


def _chain_q_expect(t, dt):
    b = t.transformer_blocks[0]
    return tchain.pack_chain_q(b.attn1.to_out[0].weight, b.attn1.to_out[0].bias, b.norm2.weight, b.norm2.bias,
                               b.attn2.to_q.weight, _cs(t), dt)


def _chain_ff_expect(t, dt):
    b = t.transformer_blocks[0]
    return tchain.pack_chain_ff(b.attn2.to_out[0].weight, b.attn2.to_out[0].bias, b.norm3.weight, b.norm3.bias,
                                b.ff.net[0].proj.weight, b.ff.net[0].proj.bias, b.ff.net[2].weight, b.ff.net[2].bias,
                                t.proj_out.weight, t.proj_out.bias, dt)


# The smallest modules on which every branch of a recipe exists.  Each builder returns the OWNER whose parameters are all
# perturbed; a case = (id, owner key, recipe, owner -> the module(s) the recipe is applied to, the parent's expression).
OWNERS = {
    "res_sc": lambda: L.ResnetBlock2D(32, 64, 32, groups=8),
    "res": lambda: L.ResnetBlock2D(32, 32, 32, groups=8),
    "wide": lambda: L.Conv2d(640, 16, 3, padding=1),
    "conv_in": lambda: L.Conv2d(4, 32, 3, padding=1),
    "self": lambda: L.Attention(32, 2, 16),
    "cross": lambda: L.Attention(32, 2, 16, cross_attention_dim=24),
    "block": lambda: L.BasicTransformerBlock(32, 2, 16, 24),
    "tf": lambda: L.Transformer2DModel(2, 16, 32, 24, norm_num_groups=8),
    "temb": lambda: L.TimestepEmbedding(32, 128),
    "zero": lambda: L.zero_module(L.Conv2d(32, 32, 1)),
    "two_res": lambda: nn.ModuleList([L.ResnetBlock2D(32, 64, 32, groups=8), L.ResnetBlock2D(64, 32, 32, groups=8)]),
    "two_cross": lambda: nn.ModuleList([L.Attention(32, 2, 16, cross_attention_dim=24), L.Attention(64, 2, 32, cross_attention_dim=24)]),
    "vres_sc": lambda: vae._Resnet(32, 64, 8),
    "vres": lambda: vae._Resnet(32, 32, 8),
    "vattn": lambda: vae._Attention(32, 8),
    "vae": lambda: vae.AutoencoderKL(block_out_channels=(64,), layers_per_block=1, norm_num_groups=8,
                                     down_block_types=("DownEncoderBlock2D",), up_block_types=("UpDecoderBlock2D",)),
    "cond": lambda: L.ControlNetConditioningEmbedding(32, 3, (16, 32)),
    "chain": lambda: L.Transformer2DModel(8, 40, 320, 64),
}

CASES = [
    ("res_sc.norm1", "res_sc", R.affine, lambda r: r.norm1, _affine),
    ("res_sc.conv1", "res_sc", R.conv3x3, lambda r: r.conv1, _conv(True)),
    ("res_sc.conv2", "res_sc", R.conv3x3, lambda r: r.conv2, _conv(True)),
    ("res_sc.shortcut", "res_sc", R.linear, lambda r: r.conv_shortcut, _linear),
    ("res_sc.fold", "res_sc", R.fold, lambda r: r, _fold_expect(True)),
    ("res.norm2", "res", R.affine, lambda r: r.norm2, _affine),
    ("res.conv2", "res", R.conv3x3, lambda r: r.conv2, _conv(True)),
    ("wide.cblock", "wide", R.conv3x3, lambda c: c, _conv(True)),
    ("wide.tap", "wide", R.conv3x3_tap, lambda c: c, _conv(False)),
    ("conv_in", "conv_in", R.conv3x3_padded(CIN_PAD), lambda c: c, _conv(False, CIN_PAD)),
    ("conv_out.pad", "conv_in", R.conv_out(40), lambda c: c,
     lambda c, dt: (_pad_rows(pack_conv3x3(c.weight, dt), 40), _pad_rows(f32(c.bias), 40))),
    ("self.qk", "self", R.matrix_rows, lambda a: (a.to_q, a.to_k),
     lambda m, dt: torch.cat([pack_matrix(m[0].weight, dt), pack_matrix(m[1].weight, dt)], 0)),
    ("self.qkv", "self", R.matrix_rows, lambda a: (a.to_q, a.to_k, a.to_v),
     lambda m, dt: torch.cat([pack_matrix(x.weight, dt) for x in m], 0)),
    ("self.wv", "self", R.matrix, lambda a: a.to_v, _matrix),
    ("self.out", "self", R.linear, lambda a: a.to_out[0], _linear),
    ("cross.wq", "cross", R.matrix, lambda a: a.to_q, _matrix),
    ("cross.wk", "cross", R.matrix, lambda a: a.to_k, _matrix),
    ("cross.wv", "cross", R.matrix, lambda a: a.to_v, _matrix),
    ("cross.out", "cross", R.linear, lambda a: a.to_out[0], _linear),
    ("block.norm1", "block", R.affine, lambda b: b.norm1, _affine),
    ("block.norm2", "block", R.affine, lambda b: b.norm2, _affine),
    ("block.norm3", "block", R.affine, lambda b: b.norm3, _affine),
    ("block.ff_in", "block", R.geglu, lambda b: b.ff.net[0].proj, _geglu_expect),
    ("block.ff_out", "block", R.linear, lambda b: b.ff.net[2], _linear),
    ("tf.norm", "tf", R.affine, lambda t: t.norm, _affine),
    ("tf.proj_in", "tf", R.linear, lambda t: t.proj_in, _linear),
    ("tf.proj_out", "tf", R.linear, lambda t: t.proj_out, _linear),
    ("temb.linear_1", "temb", R.linear, lambda t: t.linear_1, _linear),
    ("temb.linear_2", "temb", R.linear, lambda t: t.linear_2, _linear),
    ("zero.scaled", "zero", R.scaled_linear(0.5), lambda z: z,
     lambda z, dt: ((pack_matrix(z.weight, dt) * 0.5).contiguous(), f32(z.bias) * 0.5)),
    ("zero.unit", "zero", R.scaled_linear(1.0), lambda z: z, _linear),
    ("two_res.temb_rows", "two_res", R.linear_rows, lambda rs: [r.time_emb_proj for r in rs],
     lambda ms, dt: (_cat(pack_matrix(m.weight, dt) for m in ms), _cat(f32(m.bias) for m in ms))),
    ("two_cross.wk_rows", "two_cross", R.matrix_rows, lambda al: [a.to_k for a in al],
     lambda ms, dt: _cat(pack_matrix(m.weight, dt) for m in ms)),
    ("two_cross.wkv_rows", "two_cross", R.matrix_rows, lambda al: [a.to_k for a in al] + [a.to_v for a in al],
     lambda ms, dt: _cat(pack_matrix(m.weight, dt) for m in ms)),
    ("vres_sc.conv1", "vres_sc", R.conv3x3_tap, lambda r: r.conv1, _conv(False)),
    ("vres_sc.fold", "vres_sc", R.fold_tap, lambda r: r, _fold_expect(False)),
    ("vres.conv2", "vres", R.conv3x3_tap, lambda r: r.conv2, _conv(False)),
    ("vattn.norm", "vattn", R.affine, lambda a: a.group_norm, _affine),
    ("vattn.qk", "vattn", R.linear_rows, lambda a: (a.to_q, a.to_k),
     lambda m, dt: (torch.cat([pack_matrix(m[0].weight, dt), pack_matrix(m[1].weight, dt)], 0).contiguous(),
                    torch.cat([f32(m[0].bias), f32(m[1].bias)]))),
    ("vattn.v", "vattn", R.linear, lambda a: a.to_v, _linear),
    ("vattn.out", "vattn", R.linear, lambda a: a.to_out[0], _linear),
    ("vae.moments", "vae", R.vae_moments, lambda v: v, _moments_expect),
    ("vae.post_quant", "vae", R.linear_padded(CIN_PAD), lambda v: v.post_quant_conv,
     lambda pq, dt: (F.pad(pack_matrix(pq.weight, dt), (0, CIN_PAD - pq.weight.shape[1])).contiguous(), f32(pq.bias))),
    ("vae.dec_conv_in", "vae", R.conv3x3_padded(CIN_PAD), lambda v: v.decoder.conv_in, _conv(False, CIN_PAD)),
    ("vae.dec_conv_out", "vae", R.conv3x3_tap, lambda v: v.decoder.conv_out, _conv(False)),
    ("cond.image_bgr", "cond", R.cond_conv3x3(True, True), lambda e: e.conv_in,
     lambda c, dt: (pack_cond_conv3x3(c.weight, dt, 1, image=True, bgr=True), f32(c.bias))),
    ("cond.stride2", "cond", R.cond_conv3x3(False, True), lambda e: e.blocks[1],
     lambda c, dt: (pack_cond_conv3x3(c.weight, dt, 2, image=False, bgr=False), f32(c.bias))),
    ("cond.conv_out", "cond", R.conv3x3_tap, lambda e: e.conv_out, _conv(False)),
    ("chain.pre", "chain", R.chain_pre, lambda t: t, _chain_pre_expect),
    ("chain.q", "chain", R.chain_q, lambda t: t, _chain_q_expect),
    ("chain.ff", "chain", R.chain_ff, lambda t: t, _chain_ff_expect),
]
IDS = [c[0] for c in CASES]


def _tuple(v):
    return v if isinstance(v, tuple) else (v,)


def _build(recipe, m, dt):
    """A snapshot: ``f32`` of an fp32 parameter is the parameter's own storage, which an in-place write would carry along."""
    with torch.no_grad():
        return tuple(t.clone() for t in _tuple(recipe.build(m, dt, *recipe.args)))


def _same(a, b):
    assert len(a) == len(b)
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_the_wide_conv_takes_the_block_outer_order():
    assert ops.conv_cblock(640) != 0 and ops.conv_cblock(32) == 0  # "wide.cblock" is the cblock branch, the others are not


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layout_is_the_expression_the_call_sites_used(case, dtype):
    _, owner, recipe, pick, expect = case
    m = pick(_randomize(OWNERS[owner]()))
    got = _build(recipe, m, dtype)
    with torch.no_grad():
        want = _tuple(expect(m, dtype))
    assert _same(got, want)
    assert all(t.is_contiguous() for t in got)
    assert _same(_tuple(R.one(R.PackCache(), recipe, m, dtype)), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_declared_parameters_are_exactly_the_ones_read(case, dtype):
    """+0.05 on one parameter of the owning module changes the built value (any element of a tuple) if and only if the recipe
    declares that parameter."""
    _, owner, recipe, pick, _ = case
    own = _randomize(OWNERS[owner]())
    m = pick(own)
    declared = {id(p) for p in recipe.params(m)}
    base = _build(recipe, m, dtype)
    seen = 0
    for name, p in own.named_parameters():
        keep = p.detach().clone()
        with torch.no_grad():
            p.add_(0.05)
        changed = not _same(_build(recipe, m, dtype), base)
        with torch.no_grad():
            p.copy_(keep)
        assert changed == (id(p) in declared), (name, changed)
        seen += id(p) in declared
    assert seen == len(declared) > 0
    assert _same(_build(recipe, m, dtype), base)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_every_element_of_a_tuple_follows_its_own_parameters(dtype):
    """Element by element: the weight element of a pair moves with the weight only, the bias element with the bias only, and
    in the fold each of the two elements moves with both of its sources."""
    r = _randomize(L.ResnetBlock2D(32, 64, 32, groups=8))

    def moved(recipe, m, p):
        base = _build(recipe, m, dtype)
        with torch.no_grad():
            p.add_(0.05)
        new = _build(recipe, m, dtype)
        with torch.no_grad():
            p.sub_(0.05)
        return [not torch.equal(a, b) for a, b in zip(new, base)]

    assert moved(R.conv3x3, r.conv1, r.conv1.weight) == [True, False]
    assert moved(R.conv3x3, r.conv1, r.conv1.bias) == [False, True]
    assert moved(R.affine, r.norm1, r.norm1.weight) == [True, False]
    assert moved(R.affine, r.norm1, r.norm1.bias) == [False, True]
    assert moved(R.fold, r, r.conv2.weight) == [True, False] and moved(R.fold, r, r.conv_shortcut.weight) == [True, False]
    assert moved(R.fold, r, r.conv2.bias) == [False, True] and moved(R.fold, r, r.conv_shortcut.bias) == [False, True]
    proj = r.time_emb_proj
    assert moved(R.geglu, proj, proj.weight) == [True, False] and moved(R.geglu, proj, proj.bias) == [False, True]


# ------------------------------------------------------------------------------------------------- the cache
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_one_caches_until_a_declared_parameter_changes(dtype):
    r = _randomize(L.ResnetBlock2D(32, 64, 32, groups=8))
    pk = R.PackCache()
    a = R.one(pk, R.fold, r, dtype)
    assert R.one(pk, R.fold, r, dtype) is a
    with torch.no_grad():
        r.conv1.weight.add_(0.05)   # same module, not declared by the fold
        r.norm2.bias.add_(0.05)
    assert R.one(pk, R.fold, r, dtype) is a
    with torch.no_grad():
        r.conv_shortcut.bias.add_(0.05)  # declared, in place
    b = R.one(pk, R.fold, r, dtype)
    assert b is not a and torch.equal(b[0], a[0]) and not torch.equal(b[1], a[1])
    assert _same(b, _fold_expect(True)(r, dtype))
    r.conv2.weight.data = r.conv2.weight.data.clone() + 0.05  # declared, .data replaced (a load or a cast does this)
    c = R.one(pk, R.fold, r, dtype)
    assert c is not b and not torch.equal(c[0], b[0]) and _same(c, _fold_expect(True)(r, dtype))
    assert R.one(pk, R.fold, r, dtype) is c
    # the same recipe on two sub-modules of one owner, in one cache, does not collide
    w1, w2 = R.one(pk, R.conv3x3, r.conv1, dtype), R.one(pk, R.conv3x3, r.conv2, dtype)
    assert w1[0].shape != w2[0].shape and R.one(pk, R.conv3x3, r.conv1, dtype) is w1 and R.one(pk, R.conv3x3, r.conv2, dtype) is w2
    # nor do two settings of a recipe's extra arguments
    assert R.one(pk, R.conv3x3_tap, r.conv1, dtype) is not w1 and R.one(pk, R.conv3x3, r.conv1, dtype) is w1
    z = _randomize(L.Conv2d(32, 32, 1))
    h, u = R.one(pk, R.scaled_linear(0.5), z, dtype), R.one(pk, R.scaled_linear(1.0), z, dtype)
    assert R.one(pk, R.scaled_linear(0.5), z, dtype) is h and R.one(pk, R.scaled_linear(1.0), z, dtype) is u
    assert torch.equal(h[0], (u[0] * 0.5)) and torch.equal(h[1], u[1] * 0.5)


def test_two_dtypes_coexist():
    c = _randomize(L.Conv2d(32, 32, 3, padding=1))
    pk = R.PackCache()
    h, b = R.one(pk, R.conv3x3, c, torch.float16), R.one(pk, R.conv3x3, c, torch.bfloat16)
    assert h[0].dtype == torch.float16 and b[0].dtype == torch.bfloat16
    assert R.one(pk, R.conv3x3, c, torch.float16) is h and R.one(pk, R.conv3x3, c, torch.bfloat16) is b
    rs = [c, _randomize(L.Conv2d(32, 32, 3, padding=1), 6)]
    sh, sb = R.stacked(pk, R.conv3x3, rs, torch.float16), R.stacked(pk, R.conv3x3, rs, torch.bfloat16)
    assert R.stacked(pk, R.conv3x3, rs, torch.float16) is sh and R.stacked(pk, R.conv3x3, rs, torch.bfloat16) is sb
    assert R.one(pk, R.conv3x3, c, torch.float16) is h  # and one / stacked of the same module do not collide
    s1 = R.stacked(pk, R.conv3x3, [c], torch.float16)
    assert s1[0].shape == (1,) + h[0].shape and R.one(pk, R.conv3x3, c, torch.float16) is h


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_stacked_stacks_per_stream_and_follows_either_stream(dtype):
    rs = [_randomize(L.ResnetBlock2D(32, 64, 32, groups=8), s) for s in (5, 6)]
    pk = R.PackCache()
    a = R.stacked(pk, R.fold, rs, dtype)
    want = [_fold_expect(True)(r, dtype) for r in rs]
    assert _same(a, tuple(torch.stack([w[i] for w in want], 0).contiguous() for i in range(2)))
    assert all(t.is_contiguous() and t.shape[0] == 2 for t in a)
    assert R.stacked(pk, R.fold, rs, dtype) is a
    with torch.no_grad():
        rs[1].conv1.bias.add_(0.05)  # undeclared, second stream
    assert R.stacked(pk, R.fold, rs, dtype) is a
    with torch.no_grad():
        rs[1].conv_shortcut.weight.add_(0.05)  # declared, ONLY the second stream's module
    b = R.stacked(pk, R.fold, rs, dtype)
    assert b is not a and torch.equal(b[0][0], a[0][0]) and not torch.equal(b[0][1], a[0][1])
    rs[0].conv2.bias.data = rs[0].conv2.bias.data + 0.05
    c = R.stacked(pk, R.fold, rs, dtype)
    assert c is not b and not torch.equal(c[1][0], b[1][0]) and torch.equal(c[1][1], b[1][1])
    # a single tensor stacks as a tensor
    m = R.stacked(pk, R.matrix, [r.time_emb_proj for r in rs], dtype)
    assert torch.equal(m, torch.stack([pack_matrix(r.time_emb_proj.weight, dtype) for r in rs], 0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_stacked_rows_and_the_exchange_pair(dtype):
    """The grouped path's batched operands: per stream the row-concatenation over that stream's modules ([Wk; Wv] = the K
    rows, then the V rows), and the exchange pair whose first stream alone carries the conditioning scale."""
    nets = [_randomize(OWNERS["two_cross"](), s) for s in (5, 6)]
    pk = R.PackCache()
    wk = R.stacked(pk, R.matrix_rows, [[a.to_k for a in al] for al in nets], dtype)
    wv = R.stacked(pk, R.matrix_rows, [[a.to_v for a in al] for al in nets], dtype)
    wkv = R.stacked(pk, R.matrix_rows, [[a.to_k for a in al] + [a.to_v for a in al] for al in nets], dtype)
    stk = lambda ts: torch.stack(list(ts), 0).contiguous()
    assert torch.equal(wk, stk(torch.cat([pack_matrix(a.to_k.weight, dtype) for a in al], 0) for al in nets))
    assert torch.equal(wv, stk(torch.cat([pack_matrix(a.to_v.weight, dtype) for a in al], 0) for al in nets))
    assert torch.equal(wkv, torch.cat([wk, wv], 1).contiguous()) and wkv.is_contiguous()
    with torch.no_grad():
        nets[1][1].to_v.weight.add_(0.05)
    assert R.stacked(pk, R.matrix_rows, [[a.to_k for a in al] for al in nets], dtype) is wk
    assert R.stacked(pk, R.matrix_rows, [[a.to_v for a in al] for al in nets], dtype) is not wv
    assert R.stacked(pk, R.matrix_rows, [[a.to_k for a in al] + [a.to_v for a in al] for al in nets], dtype) is not wkv

    ze, zd = _randomize(L.Conv2d(32, 32, 1), 7), _randomize(L.Conv2d(32, 32, 1), 8)
    for scale in (0.5, 1.0):
        w, b = R.stacked(pk, [R.scaled_linear(scale), R.linear], [ze, zd], dtype)
        assert torch.equal(w, stk([pack_matrix(ze.weight, dtype) * scale if scale != 1.0 else pack_matrix(ze.weight, dtype),
                                   pack_matrix(zd.weight, dtype)]))
        assert torch.equal(b, stk([f32(ze.bias) * scale, f32(zd.bias)]))
        assert R.stacked(pk, [R.scaled_linear(scale), R.linear], [ze, zd], dtype)[0] is w
    with torch.no_grad():
        zd.bias.add_(0.05)
    assert R.stacked(pk, [R.scaled_linear(1.0), R.linear], [ze, zd], dtype)[0] is not w


def test_builds_run_without_autograd_and_the_cache_name_stays_importable():
    from uni_renderer_amd.controlnet import PackCache as from_controlnet
    from uni_renderer_amd.layers import PackCache as from_layers
    assert from_layers is R.PackCache and from_controlnet is R.PackCache
    c = _randomize(L.Conv2d(32, 32, 1))
    assert c.weight.requires_grad
    w, b = R.one(R.PackCache(), R.scaled_linear(0.5), c, torch.float16)
    assert not w.requires_grad and not b.requires_grad
