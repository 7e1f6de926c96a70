"""GPU tests of EMAModel through the stack, on the tiny networks: inside the eager and the captured training step, around a
validation forward on the averaged weights in the middle of a captured run, and through a checkpoint."""
import functools
import os

import numpy as np
import pytest
import torch

import util_ema as E
from util_models import O, build_product_from_oracle, product_step

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
WARMUP, REPLAYS = 2, 5


def _nets(dev, seed=38):
    nets = build_product_from_oracle(*O.build_triplet(O.TINY_CONFIG, seed=seed), torch.float32, dev)
    for m in nets:
        m.train()
        m.requires_grad_(True)
    return nets


def _opt(nets, cls=None):
    from uni_renderer_amd.optim import FusedAdamW

    return (cls or FusedAdamW)([p for m in nets for p in m.parameters()], lr=4e-4, betas=(0.9, 0.99), weight_decay=1e-2)


def _emas(nets):
    from uni_renderer_amd import EMAModel

    return [EMAModel(m.parameters(), model_cls=type(m), model_config=m.config) for m in nets]  # one per network, as diffusers has it


def _batch(dev, it):
    x, c, ehs, ti, ta = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=70 + it)]
    g = torch.Generator().manual_seed(71 + it)
    return dict(x_t=x, cond=c, ehs=ehs, t_img=ti, t_attr=ta, target_img=torch.randn(2, 4, 16, 16, generator=g).to(dev),
                target_attr=torch.randn(2, 28, 16, 16, generator=g).to(dev))


def _schedule():
    """The batches of a run: the warm-up steps of GraphedTrainStep repeat the batch it is built with, then one batch per step."""
    return [0] * WARMUP + list(range(REPLAYS))


def _state(nets, emas):
    out = [p.detach().clone() for m in nets for p in m.parameters()]
    return out + [s.clone() for e in emas or () for s in e.shadow_params]


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _eager_run(dev):
    """Seven eager steps with one EMAModel per network; after each of the first five the shadows are compared with a CPU replay
    of the emulation over the parameters copied out after that step."""
    from uni_renderer_amd.train_step import train_step

    nets = _nets(dev)
    opt, emas = _opt(nets), _emas(nets)
    shadows = [[E.widen(s) for s in e.shadow_params] for e in emas]
    for step, it in enumerate(_schedule(), 1):
        train_step(nets, _batch(dev, it), optimizer=opt, dtype=DT, ema=emas)
        if step <= 5:
            for k, (e, m) in enumerate(zip(emas, nets)):
                shadows[k] = E.replay(shadows[k], [E.widen(p) for p in m.parameters()], step)
                assert all(np.array_equal(E.widen(a), b) for a, b in zip(e.shadow_params, shadows[k])), (step, k)
                assert step == 1 or not torch.equal(e.shadow_params[0], next(m.parameters()).detach())  # an average, not a copy
    return _state(nets, None), _state(nets, emas)[len(_state(nets, None)):], [e.optimization_step for e in emas]


def _graphed(dev, with_ema, seed=38):
    from uni_renderer_amd.train_step import GraphedTrainStep

    nets = _nets(dev, seed)
    opt = _opt(nets)
    emas = _emas(nets) if with_ema else None
    step = GraphedTrainStep(nets, _batch(dev, 0), opt, dtype=DT, warmup=WARMUP, ema=emas)
    return nets, opt, emas, step


@functools.lru_cache(maxsize=None)
def _graphed_run(dev, with_ema):
    nets, opt, emas, step = _graphed(dev, with_ema)
    losses = [float(step.step(_batch(dev, it))["loss"]) for it in range(REPLAYS)]  # no host write to the EMA state in between
    return _state(nets, None), ([s.clone() for e in emas for s in e.shadow_params] if emas else None), \
        ([e.optimization_step for e in emas] if emas else None), losses


def test_eager_steps_average_the_updated_parameters(dev):
    params, shadows, steps = _eager_run(dev)
    assert steps == [WARMUP + REPLAYS] * 3 and len(shadows) == len(params)
    assert not any(torch.equal(a, b) for a, b in zip(params[:3], shadows[:3]))


def test_graphed_steps_equal_eager_steps(dev):
    params, shadows, steps = _eager_run(dev)
    g_params, g_shadows, g_steps, _ = _graphed_run(dev, True)
    assert g_steps == [7, 7, 7] == steps  # two warm-up steps and five replays, counted on the device
    assert _equal(g_params, params), "graphed parameters differ from eager ones"
    assert _equal(g_shadows, shadows), "graphed shadows differ from eager ones"


def test_the_average_does_not_disturb_the_step(dev):
    with_ema, without = _graphed_run(dev, True), _graphed_run(dev, False)
    assert _equal(with_ema[0], without[0]) and with_ema[3] == without[3]


def _validate(nets, inputs):
    for m in nets:
        m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=DT):
        out = product_step(*nets, *inputs)
    for m in nets:
        m.train()
    return out["img_pred"].clone(), out["attr_pred"].clone()


def test_validation_on_the_averaged_weights_in_the_middle_of_a_graphed_run(dev):
    want_params, want_shadows, _, want_losses = _graphed_run(dev, True)
    nets, opt, emas, step = _graphed(dev, True)
    losses = [float(step.step(_batch(dev, it))["loss"]) for it in range(2)]
    inputs = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=99)]
    raw = _validate(nets, inputs)  # (packed copies of the raw weights now exist)
    live = _state(nets, None)
    for e, m in zip(emas, nets):
        e.store(m.parameters())
        e.copy_to(m.parameters())
    averaged = _validate(nets, inputs)
    for e, m in zip(emas, nets):
        e.restore(m.parameters())
    assert _equal(_state(nets, None), live)
    fresh = _nets(dev, seed=41)  # other weights, then the shadows
    with torch.no_grad():
        for e, m in zip(emas, fresh):
            for p, s in zip(m.parameters(), e.shadow_params):
                p.copy_(s)
    want = _validate(fresh, inputs)
    assert all(torch.equal(a, b) for a, b in zip(averaged, want)), "the forward did not see the averaged weights"
    assert not torch.equal(averaged[0], raw[0])
    assert all(torch.equal(a, b) for a, b in zip(_validate(nets, inputs), raw)), "the forward did not see the restored weights"
    graph = step.g_fb
    losses += [float(step.step(_batch(dev, it))["loss"]) for it in range(2, REPLAYS)]
    assert step.g_fb is graph and losses == want_losses
    assert _equal(_state(nets, None), want_params) and _equal([s for e in emas for s in e.shadow_params], want_shadows)


def test_checkpoint_round_trip_into_live_objects(dev, tmp_path):
    from uni_renderer_amd import checkpointing as C

    want_params, want_shadows, _, want_losses = _graphed_run(dev, True)
    out = str(tmp_path / "run")
    nets, opt, emas, step = _graphed(dev, True)
    assert [float(step.step(_batch(dev, it))["loss"]) for it in range(3)] == want_losses[:3]
    saved = _state(nets, emas)
    path = C.save_state(nets, out, 3, optimizer=opt, ema_models=emas)
    assert sorted(os.listdir(path)) == ["controldec", "controldec_ema", "controlnet", "controlnet_ema", "optimizer.bin", "unet", "unet_ema"]
    for it in (5, 6):  # training runs on, then the live objects are rolled back
        step.step(_batch(dev, it))
    assert [e.optimization_step for e in emas] == [WARMUP + 5] * 3
    graph, gens = step.g_fb, [e.generation for e in emas]
    addr = [t.data_ptr() for e in emas for t in e.shadow_params + [e._step, e._cur_decay, e._one_minus_decay]]
    assert C.resume_from_checkpoint(nets, out, "latest", opt, ema_models=emas) == 3
    assert addr == [t.data_ptr() for e in emas for t in e.shadow_params + [e._step, e._cur_decay, e._one_minus_decay]]
    assert gens == [e.generation for e in emas] and [e.optimization_step for e in emas] == [WARMUP + 3] * 3
    assert _equal(_state(nets, emas), saved)
    assert [float(step.step(_batch(dev, it))["loss"]) for it in (3, 4)] == want_losses[3:] and step.g_fb is graph
    assert [e.optimization_step for e in emas] == [WARMUP + REPLAYS] * 3
    assert _equal(_state(nets, None), want_params) and _equal([s for e in emas for s in e.shadow_params], want_shadows)
    # without the argument the files written are exactly what they were
    plain = C.save_state(nets, str(tmp_path / "plain"), 5, optimizer=opt)
    assert sorted(os.listdir(plain)) == ["controldec", "controlnet", "optimizer.bin", "unet"]


def test_adamw8bit_with_one_ema_over_all_networks(dev):
    from uni_renderer_amd import EMAModel
    from uni_renderer_amd.optim import AdamW8bit
    from uni_renderer_amd.train_step import train_step

    nets = _nets(dev, seed=44)
    opt = _opt(nets, AdamW8bit)
    ps = [p for m in nets for p in m.parameters()]
    ema = EMAModel(ps, update_after_step=0)
    start = [p.detach().clone() for p in ps]
    s = [E.widen(x) for x in ema.shadow_params]
    for step in (1, 2):
        train_step(nets, _batch(dev, step), optimizer=opt, dtype=DT, ema=ema)
        s = E.replay(s, [E.widen(p) for p in ps], step)
        assert all(np.array_equal(E.widen(a), b) for a, b in zip(ema.shadow_params, s)), step
    assert ema.optimization_step == 2 and not any(torch.equal(a, b.detach()) for a, b in zip(start[:3], ps[:3]))
    with pytest.raises(ValueError, match="one per network"):
        train_step(nets, _batch(dev, 3), optimizer=opt, dtype=DT, ema=[ema])
    with pytest.raises(ValueError, match="optimizer"):
        train_step(nets, _batch(dev, 3), dtype=DT, ema=ema)
