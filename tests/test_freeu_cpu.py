"""FreeU (arXiv 2309.11497), the parts that need no GPU: the closed form the HIP kernel evaluates against the literal
fft form, plane-wave known answers, the enable / disable surface of the model and the pipeline, and the aliasing pattern
of the reference's in-place backbone scale as the test oracle reproduces it."""
import pytest
import torch

import util_freeu as F
from util_models import O

SHAPES = [(2, 2), (2, 3), (3, 2), (4, 4), (5, 3), (5, 7), (8, 8), (12, 20), (16, 16), (32, 32), (64, 64)]
SCALES = [0.9, 0.2, 1.7]


@pytest.mark.parametrize("hw", SHAPES)
def test_closed_form_equals_fft_form_in_float64(hw):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64) * 50 + torch.randn(2, 3, 1, 1, generator=g, dtype=torch.float64) * 40
    for s in SCALES:
        ref = F.fourier_filter_fft(x, s)
        got = F.fourier_filter_closed(x, s)
        # float64 round-off of an fft / a 7-term sum over at most 4096 values of size <= ~300
        assert float((got - ref).abs().max()) <= 1e-11, (hw, s)


@pytest.mark.parametrize("hw", [(5, 5), (5, 7), (8, 8), (12, 20), (7, 6)])
@pytest.mark.parametrize("form", ["fft", "closed"])
def test_plane_wave_known_answers(hw, form):
    fn = F.fourier_filter_fft if form == "fft" else F.fourier_filter_closed
    for (ky, kx), gain in F.PLANE_WAVES:
        x = F.plane_wave(ky, kx, *hw)
        for s in SCALES:
            assert float((fn(x, s) - gain(s) * x).abs().max()) <= 1e-12, (hw, ky, kx, s)


def _tiny_unet():
    import uni_renderer_amd as U

    return U.UNet2DConditionModel(**O.TINY_CONFIG)


def test_enable_disable_attribute_semantics_on_the_model():
    from uni_renderer_amd.unet_2d_blocks import freeu_enabled, freeu_params, freeu_state

    unet = _tiny_unet()
    assert not freeu_enabled(unet) and freeu_state(unet) == (None,) * 4
    unet.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    for blk in unet.up_blocks:  # the reference sets all four on every up block (controlnet.py:767-771)
        assert (blk.s1, blk.s2, blk.b1, blk.b2) == (0.9, 0.2, 1.2, 1.4)
    assert freeu_enabled(unet)
    assert [freeu_params(b) for b in unet.up_blocks] == [(1.2, 0.9), (1.4, 0.2), None, None]
    for zero in ("s1", "s2", "b1", "b2"):  # a single falsy factor disables it (unet_2d_blocks.py:2343-2348)
        unet.enable_freeu(**dict(F.SD14, **{zero: 0}))
        assert not freeu_enabled(unet)
        unet.enable_freeu(**dict(F.SD14, **{zero: None}))
        assert not freeu_enabled(unet)
    unet.enable_freeu(**F.SD14)
    unet.disable_freeu()
    for blk in unet.up_blocks:
        assert blk.s1 is None and blk.s2 is None and blk.b1 is None and blk.b2 is None
    assert not freeu_enabled(unet)


def test_only_the_unet_has_the_switch():
    import uni_renderer_amd as U

    for klass in (U.AttributeEncoderModel, U.AttributeDecoderModel):  # the reference gives them nothing
        assert not hasattr(klass, "enable_freeu") and not hasattr(klass, "disable_freeu")


def test_pipeline_surface_and_graph_key():
    from uni_renderer_amd.pipeline import UniRendererPipeline

    with pytest.raises(ValueError, match="unet"):
        UniRendererPipeline().enable_freeu(**F.SD14)
    unet = _tiny_unet()
    pipe = UniRendererPipeline(unet=unet)
    x, ehs = torch.zeros(2, 4, 8, 8), torch.zeros(2, 77, 64)
    k_off = pipe._graph_key(x, ehs, True)
    pipe.enable_freeu(**F.SD14)
    assert unet.up_blocks[0].b1 == 1.2 and unet.up_blocks[3].s2 == 0.2
    k_on = pipe._graph_key(x, ehs, True)
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.5)
    k_on2 = pipe._graph_key(x, ehs, True)
    assert len({k_off, k_on, k_on2}) == 3  # a graph captured in another FreeU state is never looked up
    pipe.disable_freeu()
    assert pipe._graph_key(x, ehs, True) == k_off
    pipe.enable_freeu(**F.SD14)
    assert pipe._graph_key(x, ehs, True) == k_on
    unet.disable_freeu()  # toggling on the model directly moves the key too
    assert pipe._graph_key(x, ehs, True) == k_off


def test_autograd_forward_refuses_freeu():
    unet = _tiny_unet()
    unet.enable_freeu(**F.SD14)
    x = torch.zeros(1, 4, 8, 8, requires_grad=True)
    with pytest.raises(NotImplementedError, match="FreeU"):
        unet(x, 10, torch.zeros(1, 77, 64))


@pytest.mark.parametrize("exchange", [True, False])
def test_oracle_wrapper_reproduces_the_in_place_aliasing(exchange, monkeypatch):
    """The reference scales ``hidden[:, : C // 2]`` with a setitem on the tensor it was handed, so the UNet's returned
    up_block_res_samples 0, 1, 2 (inputs of the three resnets of block 0) and 4, 5 (inputs of resnets 1, 2 of block 1) come
    back scaled, 3 and 6-12 do not; raw_mid is entry 0 itself unless a mid residual made a fresh tensor; raw_down never is."""
    calls = []
    orig = F.apply_freeu_

    def recording(idx, hidden, skip, *factors):
        before = hidden.clone()
        out = orig(idx, hidden, skip, *factors)
        calls.append((idx, hidden, before, skip, out[1]))
        return out

    monkeypatch.setattr(F, "apply_freeu_", recording)
    models = O.build_triplet(O.TINY_CONFIG, seed=1234)
    x, c, ehs, ti, ta = O.make_inputs(1, 8, 64, seed=3)
    out = F.oracle_step(*models, x, c, ehs, ti, ta, freeu=F.SD14, exchange=exchange, run_decoder=False)
    assert [i for i, *_ in calls] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    ups = out["up_res"]
    scaled = {0: (calls[0], 1.2), 1: (calls[1], 1.2), 2: (calls[2], 1.2), 4: (calls[4], 1.4), 5: (calls[5], 1.4)}
    touched = {h.data_ptr() for i, h, *_ in calls if i in (0, 1)}
    for i, t in enumerate(ups):
        if i in scaled:
            (_, hidden, before, _, _), b = scaled[i]
            half = t.shape[1] // 2
            assert t.data_ptr() == hidden.data_ptr()
            assert torch.equal(t[:, :half], before[:, :half] * b) and torch.equal(t[:, half:], before[:, half:])
            assert not torch.equal(t[:, :half], before[:, :half])
        else:
            assert t.data_ptr() not in touched, i
    assert (out["raw_mid_unet"].data_ptr() == ups[0].data_ptr()) == (not exchange)
    for i, hidden, before, skip, new_skip in calls:
        assert new_skip.data_ptr() != skip.data_ptr() or i > 1  # fourier_filter returns a new tensor
        if i > 1:
            assert torch.equal(hidden, before) and new_skip is skip
    assert all(t.data_ptr() not in touched for t in out["raw_unet"])
    # and with the wrapper gone the oracle is the plain one again
    assert "forward" not in vars(models[0].up_blocks[0])
