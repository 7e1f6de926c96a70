"""Training a UNet LoRA adapter on the GPU (lora.py, autograd_ops.LoraMerge, ur_lora_merge_cast_multi / ur_lora_grad_multi)
against the CPU oracle whose UNet holds ``W + s * rscale * up @ down`` as differentiable fp32 expressions of leaf factors:
loss and factor gradients, the frozen base, gradient checkpointing, a few optimisation steps, the captured step, and what the
inference path and the adapter file see afterwards.  TINY_CONFIG, B = 2, 16 x 16 latent, context 64, as test_train_gpu.py."""
import pytest
import torch

import util_lora as L
import util_lora_train as T
from conftest import rel_l2
from test_train_gpu import _oracle_loss
from util_models import O, build_product_from_oracle

pytestmark = pytest.mark.gpu
NET_SEED, DOWN_SEED, UP_SEED, RANK, ALPHA = 41, 3, 4, 4, 8.0
# rel-L2 of ALL factor gradients together against the oracle's.  Measured on the MI355X (profiles/lora_train_ab.txt):
# fp16 4.74e-3, bf16 1.98e-2 (the same with the encoder / decoder frozen or trainable; fp16 4.76e-3 at scale 0.5; against the
# float64 projection of a full fine-tune's weight gradients fp16 4.61e-3, bf16 1.54e-2).  The bounds are 2x the measured
# values against the oracle, test_train_gpu.py's habit ("bounds ~2x that")
GRAD_TOL = {torch.float16: 9.5e-3, torch.bfloat16: 4.0e-2}
LOSS_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}  # test_train_gpu.py's bounds on the relative loss difference


def _data():
    x, c, ehs, ti, ta = O.make_inputs(2, 16, 64, seed=12)
    g = torch.Generator().manual_seed(13)
    return (x, c, ehs, ti, ta), (torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 28, 16, 16, generator=g))


def _product(oracle, dev, freeze_exchange=True, up_seed=UP_SEED, targets=None, ckpt=False):
    """The product triple on fp32 masters, the UNet frozen under a trainable adapter with seeded factors."""
    unet, enc, dec = nets = build_product_from_oracle(*oracle, torch.float32, dev)
    for m in nets:
        m.train()
        m.requires_grad_(True)
        if ckpt:
            m.enable_gradient_checkpointing()
    unet.requires_grad_(False)
    if freeze_exchange:
        enc.requires_grad_(False)
        dec.requires_grad_(False)
    kw = {} if targets is None else dict(target_modules=targets)
    unet.add_adapter(rank=RANK, lora_alpha=ALPHA, generator=torch.Generator().manual_seed(DOWN_SEED), **kw)
    if up_seed is not None:
        T.set_up_factors(unet, up_seed)
    return nets


def _batch(dev):
    (x, c, ehs, ti, ta), (tgt_img, tgt_attr) = _data()
    return dict(x_t=x.to(dev), cond=c.to(dev), ehs=ehs.to(dev), t_img=ti.to(dev), t_attr=ta.to(dev),
                target_img=tgt_img.to(dev), target_attr=tgt_attr.to(dev))


def _run(nets, dev, dtype, scale=None):
    from uni_renderer_amd.train_step import dual_stream_forward, mse_losses

    b = _batch(dev)
    kw = None if scale is None else {"scale": scale}
    out = dual_stream_forward(*nets, b["x_t"], b["cond"], b["ehs"], b["t_img"], b["t_attr"], dtype=dtype, cross_attention_kwargs=kw)
    loss = mse_losses(out, b["target_img"], b["target_attr"])
    loss.backward()
    return float(loss.detach())


def _factor_grads(unet):
    st = unet._lora
    out = {}
    for n, (d, u, _) in st.adapters[st.trainable].items():
        assert d.grad is not None and u.grad is not None, n
        assert d.grad.dtype == u.grad.dtype == torch.float32 and d.grad.shape == d.shape and u.grad.shape == u.shape
        out[n] = (d.grad.detach().cpu().clone(), u.grad.detach().cpu().clone())
    return out


def _flat(grads):
    return torch.cat([t.reshape(-1).double() for n in sorted(grads) for t in grads[n]])


@pytest.fixture(scope="module")
def ref(dev):
    """The oracle triple, the factors of the adapter every test starts from, and (lazily, once per scale) the oracle's loss and
    factor gradients."""
    oracle = O.build_triplet(O.TINY_CONFIG, seed=NET_SEED)
    for m in oracle:
        m.requires_grad_(False)
    unet = _product(oracle, dev)[0]
    factors = T.factors_of(unet)
    assert all(f == ALPHA / RANK for _, _, f in factors.values()) and all(float(u.abs().max()) > 0 for _, u, _ in factors.values())
    cache = {}

    def at(scale):
        if scale not in cache:
            (x, c, ehs, ti, ta), (tgt_img, tgt_attr) = _data()
            leaves = T.oracle_factor_leaves(factors)
            unet_fn = T.oracle_unet_call(oracle[0], leaves, scale)
            loss = _oracle_loss((unet_fn, oracle[1], oracle[2]), x, c, ehs, ti, ta, tgt_img, tgt_attr)
            loss.backward()
            cache[scale] = (float(loss.detach()), {n: (d.grad.clone(), u.grad.clone()) for n, (d, u, _) in leaves.items()})
        return cache[scale]

    return oracle, factors, at


@pytest.mark.parametrize("freeze_exchange", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_loss_and_factor_gradients_match_the_oracle(dev, ref, dtype, freeze_exchange):
    oracle, factors, at = ref
    loss_o, grads_o = at(1.0)
    nets = _product(oracle, dev, freeze_exchange=freeze_exchange)
    loss = _run(nets, dev, dtype)
    grads = _factor_grads(nets[0])
    err = rel_l2(_flat(grads), _flat(grads_o))
    zero = [n for n, (gd, gu) in grads.items() if float(gd.abs().max()) == 0.0 or float(gu.abs().max()) == 0.0]
    print({"dtype": str(dtype), "freeze_exchange": freeze_exchange, "loss": loss, "loss_oracle": loss_o, "factor_grad_rel_l2": err})
    assert not zero, zero
    assert abs(loss - loss_o) / loss_o < LOSS_TOL[dtype]
    assert err < GRAD_TOL[dtype]
    if not freeze_exchange:  # the other two networks train as they always did
        assert all(p.grad is not None for m in nets[1:] for p in m.parameters() if p.requires_grad)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_factor_gradients_are_the_projection_of_a_full_fine_tune(dev, ref, dtype):
    """Isolates the new code: the same networks as a plain full fine-tune at the merged weights; its fp32 ``p.grad`` of every
    adapted matrix, projected in float64 on the host.  The two paths differ by the wgrad grouping, the rounding of W' (fp32
    then compute dtype there, once here) and the projection's rounding."""
    oracle, factors, at = ref
    spec = {n: (d, u, f) for n, (d, u, f) in factors.items()}
    merged_o = (L.oracle_with_merged(oracle[0], spec, 1.0), oracle[1], oracle[2])
    full = build_product_from_oracle(*merged_o, torch.float32, dev)
    for m in full:
        m.train()
        m.requires_grad_(False)
    for n in factors:
        full[0].get_submodule(n).weight.requires_grad_(True)
    loss_f = _run(full, dev, dtype)
    want = {}
    for n, (d, u, f) in factors.items():
        g = full[0].get_submodule(n).weight.grad.detach().double().cpu()
        want[n] = (f * (u.double().t() @ g), f * (g @ d.double().t()))
    nets = _product(oracle, dev)
    loss = _run(nets, dev, dtype)
    err = rel_l2(_flat(_factor_grads(nets[0])), _flat(want))
    print({"dtype": str(dtype), "loss": loss, "loss_full_fine_tune": loss_f, "factor_grad_rel_l2_vs_projection": err})
    assert err < GRAD_TOL[dtype]


def test_scale_through_cross_attention_kwargs(dev, ref):
    oracle, factors, at = ref
    loss_o, grads_o = at(0.5)
    loss_1, grads_1 = at(1.0)
    nets = _product(oracle, dev)
    loss = _run(nets, dev, torch.float16, scale=0.5)
    grads = _factor_grads(nets[0])
    err, apart = rel_l2(_flat(grads), _flat(grads_o)), rel_l2(_flat(grads_1), _flat(grads_o))
    print({"scale": 0.5, "loss": loss, "loss_oracle": loss_o, "factor_grad_rel_l2": err, "scale_1_vs_half": apart})
    assert abs(loss - loss_o) / loss_o < LOSS_TOL[torch.float16] and err < GRAD_TOL[torch.float16] < apart / 4
    # fuse_lora pins the scale of the differentiable forward as it pins the merged one
    nets = _product(oracle, dev)
    nets[0].fuse_lora(0.5)
    loss_p = _run(nets, dev, torch.float16, scale=1.0)
    assert loss_p == loss and all(torch.equal(a, b) for n in grads for a, b in zip(grads[n], _factor_grads(nets[0])[n]))


def test_base_stays_frozen_and_frozen_weights_cost_no_weight_gradient(dev, ref, monkeypatch):
    """``backward.wgrad_stats``: "problems" counts the weight-gradient GEMM problems executed, "matrices" the weight matrices
    that received a gradient from them.  q | k | v of a self-attention and the k | v of all cross-attentions of a phase are ONE
    projection each on the differentiable path (A.cat_adjacent), i.e. one problem for several matrices: the number of
    matrices is what equals the number of adapted ones; the number of problems is the number of Linear / Conv3x3 nodes whose
    weight wants a gradient -- with a frozen base none but the adapted ones."""
    from uni_renderer_amd import autograd_ops as A, backward as B

    oracle, factors, at = ref
    nodes = {"n": 0}
    lin, conv = A.linear, A.conv3x3

    def counted(fn):
        def call(x, w, *a, **k):
            nodes["n"] += int(w.requires_grad)
            return fn(x, w, *a, **k)
        return call

    monkeypatch.setattr(A, "linear", counted(lin))
    monkeypatch.setattr(A, "conv3x3", counted(conv))
    nets = _product(oracle, dev)
    unet = nets[0]
    lp = {id(p) for p in unet.lora_parameters()}
    before = {(i, n): p.detach().clone() for i, m in enumerate(nets) for n, p in m.named_parameters()}
    base = {n: t.clone() for n, t in unet._lora.base.items()}
    assert set(base) == set(factors)
    B.wgrad_stats.update(problems=0, matrices=0)
    _run(nets, dev, torch.bfloat16)
    print({"adapted": len(factors), "wgrad_stats": dict(B.wgrad_stats), "nodes": nodes["n"]})
    assert B.wgrad_stats["matrices"] == len(factors)                            # one per adapted matrix, nothing else
    assert B.wgrad_stats["problems"] == nodes["n"] <= len(factors)
    assert all(p.grad is None for p in unet.parameters() if id(p) not in lp)
    assert all(p.grad is None for m in nets[1:] for p in m.parameters())
    for i, m in enumerate(nets):
        for n, p in m.named_parameters():
            assert torch.equal(p.detach(), before[(i, n)]), (i, n)
    assert all(torch.equal(unet._lora.base[n], base[n]) for n in base)
    # without an adapter and with everything trainable: one problem per Linear / Conv3x3 node of the graph and one matrix per
    # Linear / Conv2d module that got a gradient, as before
    plain = build_product_from_oracle(*oracle, torch.float32, dev)
    for m in plain:
        m.train()
        m.requires_grad_(True)
    nodes["n"] = 0
    B.wgrad_stats.update(problems=0, matrices=0)
    _run(plain, dev, torch.bfloat16)
    mats = sum(1 for net in plain for m in net.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)) and m.weight.grad is not None)
    print({"plain": dict(B.wgrad_stats), "nodes": nodes["n"], "modules": mats})
    assert nodes["n"] > 100 and B.wgrad_stats["problems"] == nodes["n"] and B.wgrad_stats["matrices"] == mats


def test_gradient_checkpointing_gives_the_same_bits(dev, ref):
    oracle, factors, at = ref
    targets = ("to_q", "to_k", "to_v", "to_out.0", "conv_shortcut", "proj_in")  # a merged weight INSIDE a checkpointed resnet too
    res = []
    for ckpt in (False, True):
        nets = _product(oracle, dev, targets=targets, ckpt=ckpt)
        assert any(n.endswith("conv_shortcut") for n in nets[0]._lora.adapters["default"])
        loss = _run(nets, dev, torch.bfloat16)
        res.append((loss, _factor_grads(nets[0])))
    assert res[0][0] == res[1][0] and set(res[0][1]) == set(res[1][1])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n][0], res[1][1][n][0]) and torch.equal(res[0][1][n][1], res[1][1][n][1]), n
        assert float(res[0][1][n][0].abs().max()) > 0


def test_a_few_optimizer_steps_from_zero_up_reduce_the_loss(dev, ref):
    from uni_renderer_amd.optim import FusedAdamW
    from uni_renderer_amd.train_step import train_step

    oracle, factors, at = ref
    nets = _product(oracle, dev, up_seed=None)
    opt = FusedAdamW(nets[0].lora_parameters(), lr=1e-3)
    batch = _batch(dev)
    losses = [train_step(nets, batch, optimizer=opt, dtype=torch.bfloat16)["loss"] for _ in range(6)]
    print({"losses": losses})
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]


def test_captured_step_is_the_eager_one_bit_for_bit(dev, ref):
    from uni_renderer_amd.optim import FusedAdamW
    from uni_renderer_amd.train_step import GraphedTrainStep, train_step

    oracle, factors, at = ref
    batch = _batch(dev)

    def setup():
        nets = _product(oracle, dev)
        return nets, FusedAdamW(nets[0].lora_parameters(), lr=1e-3)

    nets_e, opt_e = setup()
    eager = [train_step(nets_e, batch, optimizer=opt_e, dtype=torch.bfloat16)["loss"] for _ in range(3)]
    nets_g, opt_g = setup()
    step = GraphedTrainStep(nets_g, batch, opt_g, dtype=torch.bfloat16, warmup=0)
    graphed = [float(step.step(batch)["loss"]) for _ in range(3)]
    print({"eager": eager, "graphed": graphed})
    assert eager == graphed
    for a, b in zip(nets_e[0].lora_parameters(), nets_g[0].lora_parameters()):
        assert torch.equal(a, b)
        sa, sb = opt_e.state[a], opt_g.state[b]
        assert set(sa) == set(sb)
        for k in sa:
            if torch.is_tensor(sa[k]):
                assert torch.equal(sa[k], sb[k]), k
            else:
                assert sa[k] == sb[k], k
    assert any(not torch.equal(p.detach().cpu(), factors[n][i]) for n, pair in nets_g[0]._lora.adapters["default"].items()
               for i, p in enumerate(pair[:2]))


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 3e-3), (torch.bfloat16, 2.5e-2)])  # test_lora_gpu.py's merged-network bounds
def test_after_training_inference_file_and_unload(dev, ref, dtype, tol, tmp_path):
    from uni_renderer_amd.optim import FusedAdamW
    from uni_renderer_amd.train_step import train_step

    oracle, factors, at = ref
    nets = _product(oracle, dev)
    unet = nets[0]
    start = {n: p.detach().clone() for n, p in unet.named_parameters() if not n.startswith("lora_factors.")}
    inputs = [t.to(dev) for t in _data()[0]]
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        first = L.step_with_scale(*nets, *inputs, None)
    opt = FusedAdamW(unet.lora_parameters(), lr=1e-2)
    for _ in range(2):
        train_step(nets, _batch(dev), optimizer=opt, dtype=dtype)
    now = T.factors_of(unet)
    assert any(not torch.equal(now[n][0], factors[n][0]) for n in now)
    # a no_grad forward merges again: the oracle holding the float64-merged weights at the CURRENT factors
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        out = L.step_with_scale(*nets, *inputs, None)
    spec = {n: (d, u, f) for n, (d, u, f) in now.items()}
    want = O.dual_stream_step(L.oracle_with_merged(oracle[0], spec, 1.0), oracle[1], oracle[2], *_data()[0])
    errs = {k: rel_l2(out[k], want[k]) for k in ("img_pred", "attr_pred")}
    print({"dtype": str(dtype), "vs_merged_oracle": errs, "moved": rel_l2(out["img_pred"], first["img_pred"])})
    assert max(errs.values()) < tol, errs
    assert not torch.equal(out["img_pred"], first["img_pred"])
    # the file save_attn_procs writes gives a fresh model the same outputs at the same scale
    unet.save_attn_procs(str(tmp_path))
    fresh = build_product_from_oracle(*oracle, torch.float32, dev)
    fresh[0].load_attn_procs(str(tmp_path))
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        again = L.step_with_scale(*fresh, *inputs, None)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # unload_lora() restores every adapted parameter from `base`, bit for bit
    unet.unload_lora()
    assert not any(n.startswith("lora_factors.") for n, _ in unet.named_parameters())
    for n, p in unet.named_parameters():
        assert torch.equal(p.detach(), start[n]), n
