"""ControlNetModel without a GPU: parameter counts, state_dict keys against the oracle subclass of util_controlnet.py,
from_unet, the config round trip, the constructor's refusals and the inference-only rule."""
import pytest
import torch

import util_controlnet as UC
from util_models import O


def _product(cfg, **kw):
    import uni_renderer_amd as U

    return U.ControlNetModel(**UC.trunk_config(cfg), **kw)


def test_tiny_parameter_count_and_keys():
    oracle = UC.build_oracle(O.TINY_CONFIG)
    net = _product(O.TINY_CONFIG)
    assert O.count_params(oracle) == UC.TINY_PARAMS == O.count_params(net)
    assert O.count_params(net.controlnet_cond_embedding) == 496_400
    sd_o, sd_p = oracle.state_dict(), net.state_dict()
    assert set(sd_o) == set(sd_p)
    assert all(sd_o[k].shape == sd_p[k].shape for k in sd_o)
    names = [k for k in sd_p if k.startswith("controlnet_cond_embedding.")]
    assert sorted(names) == sorted(f"controlnet_cond_embedding.{m}.{p}" for m in ["conv_in", "conv_out"] + [f"blocks.{i}" for i in range(6)]
                                   for p in ("weight", "bias"))
    assert [m.stride[0] for m in net.controlnet_cond_embedding.blocks] == [1, 2, 1, 2, 1, 2]
    # zero-initialised: the embedding's conv_out and the 12 + 1 zero convs
    zeros = [net.controlnet_cond_embedding.conv_out] + list(net.controlnet_down_blocks) + [net.controlnet_mid_block]
    assert len(zeros) == 14 and all(float(p.abs().max()) == 0.0 for m in zeros for p in m.parameters())
    net.load_state_dict(sd_o)  # strict


def test_sd15_parameter_count():
    net = _product(O.SD15_CONFIG)
    assert O.count_params(net) == UC.SD_PARAMS
    assert O.count_params(net) - O.count_params(net.controlnet_cond_embedding) == 360_192_640
    assert O.count_params(net.controlnet_cond_embedding) == 1_086_480


def test_from_unet_copies_the_trunk_and_leaves_the_zero_convs_zero():
    import uni_renderer_amd as U

    torch.manual_seed(3)
    cfg = dict(O.TINY_CONFIG)
    unet = U.UNet2DConditionModel(**cfg)
    net = U.ControlNetModel.from_unet(unet, controlnet_conditioning_channel_order="bgr",
                                      conditioning_embedding_out_channels=(16, 32, 64))
    assert net.config["controlnet_conditioning_channel_order"] == "bgr"
    assert tuple(net.config["conditioning_embedding_out_channels"]) == (16, 32, 64) and len(net.controlnet_cond_embedding.blocks) == 4
    for name in ("conv_in", "time_embedding", "down_blocks", "mid_block"):
        a, b = getattr(unet, name).state_dict(), getattr(net, name).state_dict()
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), name
    assert all(float(p.abs().max()) == 0.0 for m in list(net.controlnet_down_blocks) + [net.controlnet_mid_block] for p in m.parameters())
    fresh = U.ControlNetModel.from_unet(unet, load_weights_from_unet=False)
    assert not torch.equal(fresh.conv_in.weight, unet.conv_in.weight)
    assert tuple(fresh.config["conditioning_embedding_out_channels"]) == (16, 32, 96, 256)
    for k in ("in_channels", "block_out_channels", "cross_attention_dim", "attention_head_dim", "layers_per_block"):
        assert fresh.config[k] == unet.config[k], k


def test_config_round_trip(tmp_path):
    import uni_renderer_amd as U

    net = _product(O.TINY_CONFIG, controlnet_conditioning_channel_order="bgr")
    UC.randomize(net)
    assert net.config["_class_name"] == "ControlNetModel" and net.config["conditioning_channels"] == 3
    net.register_to_config(in_channels=4)
    net.save_pretrained(str(tmp_path))
    back = U.ControlNetModel.from_pretrained(str(tmp_path))
    norm = lambda c: {k: list(v) if isinstance(v, tuple) else v for k, v in c.items()}  # json has no tuples
    assert norm(back.config) == norm(net.config)
    a, b = net.state_dict(), back.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_inactive_branches_raise():
    with pytest.raises(NotImplementedError):
        _product(O.TINY_CONFIG, global_pool_conditions=True)
    with pytest.raises(NotImplementedError, match="class_embed_type"):
        _product(O.TINY_CONFIG, class_embed_type="timestep")
    with pytest.raises(NotImplementedError):
        _product(O.TINY_CONFIG, use_linear_projection=True)
    with pytest.raises(ValueError, match="channel_order"):
        _product(O.TINY_CONFIG, controlnet_conditioning_channel_order="gbr")
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        _product(O.TINY_CONFIG, conditioning_embedding_out_channels=(16, 32, 96))
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        _product(O.TINY_CONFIG, conditioning_embedding_out_channels=(24, 64))
    net = _product(O.TINY_CONFIG).half()
    x, cond, ehs, t = UC.make_inputs(1, (8, 8), (64, 64), 64)
    with pytest.raises(NotImplementedError, match="class_labels"):
        net(x, t, ehs, cond, class_labels=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="inference only"):  # parameters require gradients, autograd is recording
        net(x, t, ehs, cond)


def test_conv_in_without_a_residual_is_the_old_call():
    """``_conv_in(res=None)`` must make the call it made before the operand existed (same arguments, (hi, lo) form included)."""
    import inspect

    from uni_renderer_amd import controlnet as CN

    src = inspect.getsource(CN._DenoiserBase._conv_in)
    assert "return ops.conv3x3(ops.to_nhwc(x_nchw, dt, CIN_PAD), w, b, hilo=ops.PRECISE_RESIDUAL)\n" in src
    assert inspect.signature(CN._DenoiserBase._conv_in).parameters["res"].default is None


def test_oracle_subclass_follows_the_reference_scaling():
    """guess_mode scales = logspace(-1, 0, 13) * conditioning_scale, mid block last; bgr = flip of the image channels."""
    oracle = UC.build_oracle(O.TINY_CONFIG, seed=5)
    x, cond, ehs, t = UC.make_inputs(1, (8, 8), (64, 64), 64, seed=3)
    with torch.no_grad():
        res, mid = oracle(x, t, ehs, cond)
        gres, gmid = oracle(x, t, ehs, cond, conditioning_scale=0.7, guess_mode=True)
        oracle.channel_order = "bgr"
        bres, _ = oracle(x, t, ehs, cond.flip(1))
    sc = torch.logspace(-1, 0, 13) * 0.7
    assert len(res) == 12 and all(torch.allclose(g, r * s, rtol=1e-5, atol=1e-7) for g, r, s in zip(gres, res, sc))
    assert torch.allclose(gmid, mid * sc[-1], rtol=1e-5, atol=1e-7) and abs(float(sc[-1]) - 0.7) < 1e-6
    assert all(torch.equal(a, b) for a, b in zip(res, bres))
    assert float(res[0].abs().max()) > 0
