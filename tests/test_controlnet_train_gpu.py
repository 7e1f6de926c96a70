"""Training ControlNetModel against a frozen UNet on the GPU (train_step.controlnet_forward; the embedding's backward on
csrc/condconv_bwd.hip): loss and the gradient of every ControlNet parameter against the CPU oracle's autograd, a frozen UNet that
costs nothing, the reference's zero initialisation, the scales, `bgr`, optimizer steps, graph capture of the embedding chain, the
unchanged inference path and the two refusals.  Tiny configuration, B = 2, 8 x 8 latent, 64 x 64 image; the networks come from
util_controlnet.build_oracle / randomize, so the zero convs are not zero; the loss is the MSE of the frozen UNet's output."""
import pytest
import torch
import torch.nn.functional as F

import util_controlnet as UC
from conftest import rel_l2
from test_lora_train_gpu import GRAD_TOL, LOSS_TOL
from util_models import O

pytestmark = pytest.mark.gpu
EMB = "controlnet_cond_embedding."


def _data():
    x, cond, ehs, t = UC.make_inputs(2, (8, 8), (64, 64), 64, seed=21)
    return x, cond, ehs, t, torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(22))


@pytest.fixture(scope="module")
def ref():
    """The oracle pair (ControlNet per channel order, one frozen UNet) and, once per (order, scale, guess_mode), the oracle's loss
    and parameter gradients."""
    torch.manual_seed(77)
    unet_o = O.UNet2DConditionModel(**O.TINY_CONFIG).eval().requires_grad_(False)
    nets, cache = {}, {}

    def oracle(order="rgb"):
        if order not in nets:
            nets[order] = UC.build_oracle(O.TINY_CONFIG, seed=1234, channel_order=order)
        return nets[order]

    def at(order="rgb", scale=1.0, guess=False):
        key = (order, scale, guess)
        if key not in cache:
            cn = oracle(order).requires_grad_(True)
            cn.zero_grad(set_to_none=True)
            x, cond, ehs, t, target = _data()
            res, mid = cn(x, t, ehs, cond, conditioning_scale=scale, guess_mode=guess)
            img = unet_o(x, t, ehs, down_block_additional_residuals=res, mid_block_additional_residual=mid)[0]
            loss = F.mse_loss(img, target)
            loss.backward()
            cache[key] = (float(loss.detach()), {n: p.grad.detach().clone() for n, p in cn.named_parameters()})
            cn.zero_grad(set_to_none=True)
        return cache[key]

    return unet_o, oracle, at


def _unet(unet_o, dev, dtype):
    import uni_renderer_amd as U

    unet = U.UNet2DConditionModel(**O.TINY_CONFIG)
    unet.load_state_dict(unet_o.state_dict())
    unet = unet.to(dev).eval().requires_grad_(False)
    unet.compute_dtype = dtype
    return unet


def _controlnet(oracle_cn, dev, dtype, state=None):
    """The product on fp32 masters, every parameter trainable, computing in ``dtype``."""
    import uni_renderer_amd as U

    cn = U.ControlNetModel(controlnet_conditioning_channel_order=oracle_cn.channel_order, **UC.trunk_config(oracle_cn.cfg))
    cn.load_state_dict(oracle_cn.state_dict() if state is None else state)
    cn = cn.to(dev).train().requires_grad_(True)
    cn.compute_dtype = dtype
    return cn


# fp16 only: the gradients that reach the embedding's first layers are below fp16's range without a loss scale -- the ORACLE's
# dy at conv_in has a median of 5e-9 and a maximum of 7e-8 against fp16's smallest subnormal 6e-8 -- so the tests that look
# at those layers alone in fp16 scale the loss by a power of two (exact) like any fp16 training does, and unscale the gradients.
# 2^14 lifts that median into fp16's normal range and keeps the largest gradient of the step (the loss's own, <= 0.02) below 400.
FP16_LOSS_SCALE = 2.0 ** 14


def _loss(cn, unet, dev, **kw):
    x, cond, ehs, t, target = [v.to(dev) for v in _data()]
    res, mid = cn(x, t, ehs, cond, return_dict=False, **kw)
    img = unet(x, t, ehs, down_block_additional_residuals=res, mid_block_additional_residual=mid, return_dict=False)[0]
    return F.mse_loss(img.float(), target)


def _run(cn, unet, dev, loss_scale=1.0, **kw):
    loss = _loss(cn, unet, dev, **kw)
    (loss * loss_scale).backward()
    torch.cuda.synchronize()
    if loss_scale != 1.0:
        for p in cn.parameters():
            if p.grad is not None:
                p.grad.div_(loss_scale)
    return float(loss.detach())


def _grads(cn):
    out = {}
    for n, p in cn.named_parameters():
        assert p.grad is not None, n
        assert p.grad.shape == p.shape and p.grad.dtype == p.dtype, n
        out[n] = p.grad.detach().cpu().clone()
    return out


def _flat(grads, keep=lambda n: True):
    return torch.cat([grads[n].reshape(-1).double() for n in sorted(grads) if keep(n)])


def _narrow(n):
    return n.startswith(EMB) and not n.startswith(EMB + "conv_out")


def _compare(grads, grads_o):
    assert set(grads) == set(grads_o)
    return (rel_l2(_flat(grads), _flat(grads_o)), rel_l2(_flat(grads, lambda n: n.startswith(EMB)), _flat(grads_o, lambda n: n.startswith(EMB))),
            rel_l2(_flat(grads, _narrow), _flat(grads_o, _narrow)))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_loss_and_every_gradient_match_the_oracle(dev, ref, dtype):
    unet_o, oracle, at = ref
    loss_o, grads_o = at()
    cn, unet = _controlnet(oracle(), dev, dtype), _unet(unet_o, dev, dtype)
    loss = _run(cn, unet, dev)
    grads = _grads(cn)
    err_all, err_emb, err_narrow = _compare(grads, grads_o)
    print({"dtype": str(dtype), "loss": loss, "loss_oracle": loss_o, "grad_rel_l2_all": err_all, "grad_rel_l2_embedding": err_emb,
           "grad_rel_l2_seven_narrow_convs": err_narrow})
    # no gradient is identically zero -- except where the oracle's own is: at an 8 x 8 latent the mid block sees ONE token, its
    # self-attention's softmax is the constant 1, and to_q / to_k of that attention have no gradient
    zero = {n for n, g in grads.items() if float(g.abs().max()) == 0.0}
    zero_o = {n for n, g in grads_o.items() if float(g.abs().max()) == 0.0}
    assert zero_o == {"mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight", "mid_block.attentions.0.transformer_blocks.0.attn1.to_k.weight"}
    assert zero <= zero_o, zero - zero_o
    assert abs(loss - loss_o) / loss_o < LOSS_TOL[dtype]
    assert err_all < GRAD_TOL[dtype]
    assert err_emb < GRAD_TOL[dtype] and err_narrow < GRAD_TOL[dtype]


def test_frozen_unet_gets_no_gradient_and_costs_no_weight_gradient_problem(dev, ref):
    from uni_renderer_amd import backward as B

    unet_o, oracle, at = ref
    dtype = torch.bfloat16
    cn, unet = _controlnet(oracle(), dev, dtype), _unet(unet_o, dev, dtype)
    B.wgrad_stats.update(problems=0, matrices=0)
    _run(cn, unet, dev)
    with_cn = dict(B.wgrad_stats)
    assert all(p.grad is None for p in unet.parameters())
    mats = sum(1 for m in cn.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)) and m.weight.grad is not None)
    # the same step with the ControlNet frozen as well and only its residuals' path alive: nothing wants a weight gradient
    cn.requires_grad_(False)
    cn.controlnet_mid_block.bias.requires_grad_(True)
    B.wgrad_stats.update(problems=0, matrices=0)
    _run(cn, unet, dev)
    print({"trainable": with_cn, "modules_with_weight_grad": mats, "frozen": dict(B.wgrad_stats)})
    assert with_cn["matrices"] == mats and with_cn["problems"] > 0
    assert B.wgrad_stats == {"problems": 0, "matrices": 0}


def test_reference_initialisation_trains_the_zero_convs_first(dev, ref):
    """``from_unet``: conv_out of the embedding and the 12 + 1 zero convs are zero, so only the 13 zero convs (whose inputs are not
    zero) receive a gradient; after one optimizer step the embedding's conv_out receives one too."""
    import uni_renderer_amd as U
    from uni_renderer_amd.optim import FusedAdamW

    unet_o, oracle, at = ref
    dtype = torch.bfloat16
    unet = _unet(unet_o, dev, dtype)
    cn = U.ControlNetModel.from_unet(unet).to(dev).train().requires_grad_(True)
    cn.compute_dtype = dtype
    zero_convs = {id(p) for m in list(cn.controlnet_down_blocks) + [cn.controlnet_mid_block] for p in m.parameters()}
    opt = FusedAdamW(cn.parameters(), lr=1e-3)
    _run(cn, unet, dev)
    for n, p in cn.named_parameters():
        nz = float(p.grad.abs().max()) > 0
        assert nz == (id(p) in zero_convs), (n, nz)
    opt.step()
    opt.zero_grad(set_to_none=True)
    _run(cn, unet, dev)
    e = cn.controlnet_cond_embedding
    assert float(e.conv_out.weight.grad.abs().max()) > 0 and float(e.conv_out.bias.grad.abs().max()) > 0


@pytest.mark.parametrize("kw", [dict(scale=0.5, guess=False), dict(scale=1.0, guess=True)], ids=["scale0.5", "guess_mode"])
def test_scales_under_autograd(dev, ref, kw):
    unet_o, oracle, at = ref
    dtype = torch.float16
    loss_o, grads_o = at(scale=kw["scale"], guess=kw["guess"])
    loss_1, grads_1 = at()
    cn, unet = _controlnet(oracle(), dev, dtype), _unet(unet_o, dev, dtype)
    loss = _run(cn, unet, dev, loss_scale=FP16_LOSS_SCALE, conditioning_scale=kw["scale"], guess_mode=kw["guess"])
    err_all, err_emb, _ = _compare(_grads(cn), grads_o)
    apart = rel_l2(_flat(grads_1), _flat(grads_o))
    print({**kw, "loss": loss, "loss_oracle": loss_o, "grad_rel_l2_all": err_all, "grad_rel_l2_embedding": err_emb, "apart": apart})
    assert abs(loss - loss_o) / loss_o < LOSS_TOL[dtype]
    assert err_all < GRAD_TOL[dtype] < apart / 4 and err_emb < GRAD_TOL[dtype]


def test_bgr_first_layer_gradient(dev, ref):
    unet_o, oracle, at = ref
    dtype = torch.float16
    loss_o, grads_o = at(order="bgr")
    cn, unet = _controlnet(oracle("bgr"), dev, dtype), _unet(unet_o, dev, dtype)
    assert cn.config["controlnet_conditioning_channel_order"] == "bgr"
    _run(cn, unet, dev, loss_scale=FP16_LOSS_SCALE)
    g, go = _grads(cn)[EMB + "conv_in.weight"], grads_o[EMB + "conv_in.weight"]
    err, unflipped = rel_l2(g, go), rel_l2(g.flip(1), go)
    print({"bgr_conv_in_weight_grad_rel_l2": err, "without_the_flip": unflipped})
    assert err < GRAD_TOL[dtype] < unflipped / 4


def test_five_fused_adamw_steps_reduce_the_loss(dev, ref):
    from uni_renderer_amd.optim import AdamW8bit, FusedAdamW

    unet_o, oracle, at = ref
    dtype = torch.bfloat16
    unet = _unet(unet_o, dev, dtype)
    for make in (lambda ps: FusedAdamW(ps, lr=1e-4), lambda ps: AdamW8bit(ps, lr=1e-4)):
        cn = _controlnet(oracle(), dev, dtype)
        opt = make(list(cn.parameters()))
        losses = []
        for _ in range(6):
            opt.zero_grad(set_to_none=True)
            losses.append(_run(cn, unet, dev))
            norm = torch.nn.utils.clip_grad_norm_(cn.parameters(), 1.0)
            assert bool(torch.isfinite(norm))
            opt.step()
        print({"optimizer": type(opt).__name__, "losses": losses})
        assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]


def test_embedding_forward_and_backward_capture_in_one_graph(dev, ref):
    """Forward + backward of the embedding chain (seven narrow convs with their SiLUs) in ONE torch.cuda.graph on one stream:
    the replay gives the bits of the eager run (the wgrad workspace comes from torch's allocator)."""
    unet_o, oracle, at = ref
    dtype = torch.float16
    cn = _controlnet(oracle(), dev, dtype)
    emb = cn.controlnet_cond_embedding
    params = [p for c in [emb.conv_in] + list(emb.blocks) for p in (c.weight, c.bias)]
    cond = _data()[1].to(dev)
    gy = torch.randn(2, 8, 8, 256, generator=torch.Generator().manual_seed(3)).to(dev, dtype)

    def run():
        h = emb.forward_autograd(cond, dtype)
        return (h,) + torch.autograd.grad(h, params, gy)

    # ONE stream for the first use of the parameters under autograd, the warm-up and the capture: autograd gives a leaf's
    # gradient accumulator the stream of its first use and makes that stream wait for the gradient's producer; a capture on
    # another stream would pull the first stream into the graph as a branch that torch.autograd.grad never joins again
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in run()]
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = run()
    for _ in range(2):
        for o in out:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    assert all(float(t.float().abs().max()) > 0 for t in eager)


def test_inference_path_is_untouched_by_training(dev, ref):
    """The no-grad forward takes the fused inference path whatever the parameters' requires_grad says, and gives the same bits
    before and after a differentiable forward + backward on the same network, and the bits of a frozen eval() copy."""
    unet_o, oracle, at = ref
    dtype = torch.float16
    cn, unet = _controlnet(oracle(), dev, dtype), _unet(unet_o, dev, dtype)
    x, cond, ehs, t, _ = [v.to(dev) for v in _data()]

    def infer(net):
        with torch.no_grad():
            res, mid = net(x, t, ehs, cond, conditioning_scale=0.7, guess_mode=True, return_dict=False)
        return [r.clone() for r in res] + [mid.clone()]

    before = infer(cn)
    _run(cn, unet, dev)
    after = infer(cn)
    frozen = UC.build_product(oracle(), None, dev)
    frozen.compute_dtype = dtype
    other = infer(frozen)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and all(torch.equal(a, b) for a, b in zip(before, other))
    assert all(not r.requires_grad for r in before)


def test_refusals(dev, ref):
    from uni_renderer_amd.controlnet import CONTROLNET_AUTOGRAD_MSG
    from uni_renderer_amd.layers import COND_IMAGE_GRAD_MSG

    unet_o, oracle, at = ref
    cn = _controlnet(oracle(), dev, torch.float16)
    x, cond, ehs, t, _ = _data()
    with pytest.raises(NotImplementedError) as e:
        cn(x.to(dev), t.to(dev), ehs.to(dev), cond.to(dev).requires_grad_(True))
    assert str(e.value) == COND_IMAGE_GRAD_MSG and "inference only" not in COND_IMAGE_GRAD_MSG
    with pytest.raises(NotImplementedError) as e:
        cn.cpu()(x, t, ehs, cond)
    assert str(e.value) == CONTROLNET_AUTOGRAD_MSG
