"""No executor keeps a stale packed weight: after an in-place update of ONE parameter of a role (a norm gamma, a conv bias, a
shortcut weight, ...) in each network, the module step, the grouped step, both hoisted steps and the VAE -- all with warm
caches -- must give the bits of networks that carry the same parameters and have never run.  (The all-parameters-at-once test
of the loop graphs cannot see one stale bias.)"""
import pytest
import torch

from util_models import O, build_product_from_oracle, product_step

from oracle import vae_oracle as V

pytestmark = pytest.mark.gpu

# role -> per network the parameter that is written (first match in named_parameters; a network without the role is left out)
ROLES = [
    ("norm gamma", ("resnets.0.norm1.weight",) * 3, "resnets.0.norm1.weight"),
    ("conv bias", ("resnets.0.conv1.bias",) * 3, "resnets.0.conv1.bias"),
    ("3x3 conv weight", ("resnets.0.conv2.weight",) * 3, "resnets.0.conv2.weight"),
    ("shortcut weight", ("conv_shortcut.weight",) * 3, "conv_shortcut.weight"),
    ("time_emb_proj weight", ("time_emb_proj.weight",) * 3, None),
    ("time-embedding linear_2 bias", ("time_embedding.linear_2.bias",) * 3, None),
    ("cross-attention to_k", ("attn2.to_k.weight",) * 3, "to_k.weight"),
    ("self-attention to_v", ("attn1.to_v.weight",) * 3, "to_v.bias"),
    ("feed-forward proj bias", ("ff.net.0.proj.bias",) * 3, None),
    ("proj_out weight", ("proj_out.weight",) * 3, "post_quant_conv.weight"),
    ("exchange convs", (None, "controlnet_down_blocks.3.weight", "control_down_blocks.3.weight"), "quant_conv.bias"),
    ("mid exchange convs", (None, "controlnet_mid_block.bias", "control_mid_block.weight"), "quant_conv.weight"),
    ("conv_out weight", ("conv_out.weight", None, "conv_out.weight"), "conv_out.weight"),
]


def _bump(net, suffix):
    if suffix is None:
        return
    hits = [p for n, p in net.named_parameters() if n.endswith(suffix)]
    assert hits, suffix
    with torch.no_grad():
        hits[0].add_(0.05)


def _vae(oracle, dev):
    from uni_renderer_amd.vae import AutoencoderKL

    c = oracle.cfg
    n = len(c["block_out_channels"])
    m = AutoencoderKL(in_channels=c["in_channels"], out_channels=c["out_channels"], latent_channels=c["latent_channels"],
                      block_out_channels=c["block_out_channels"], layers_per_block=c["layers_per_block"],
                      norm_num_groups=c["norm_num_groups"], scaling_factor=c["scaling_factor"],
                      down_block_types=("DownEncoderBlock2D",) * n, up_block_types=("UpDecoderBlock2D",) * n)
    m.load_state_dict(oracle.state_dict())
    return m.to(torch.float16).to(dev).eval()


class _Executors:
    """The four executors of one triplet and its VAE; the executor objects (and with them every cache) live across ``run``s."""

    def __init__(self, nets, vae):
        from uni_renderer_amd.fused import GroupedDualStreamStep
        from uni_renderer_amd.hoist import HoistedSamplingStep

        self.nets, self.vae = nets, vae
        self.grouped = GroupedDualStreamStep(*nets)
        self.inverse = HoistedSamplingStep(*nets, "inverse")
        self.render = HoistedSamplingStep(*nets, "render", conditioning_scale=0.5)

    @torch.no_grad()
    def run(self, x, c, ehs, ti, ta, img, z):
        out = {}
        mod = product_step(*self.nets, x, c, ehs, ti, ta)
        out["module.img"], out["module.attr"] = mod["img_pred"], mod["attr_pred"]
        grp = self.grouped(x, c, ehs, ti, ta)
        out["grouped.img"], out["grouped.attr"] = grp["img_pred"], grp["attr_pred"]
        self.inverse.prologue(x, ehs, ti)  # a fresh prologue: the hoisted half is recomputed from the current parameters
        out["inverse.attr"] = self.inverse.step(c, ta)["attr_pred"]
        self.render.prologue(c, ehs, ta)
        out["render.img"] = self.render.step(x, ti)["img_pred"]
        post = self.vae.encode(img).latent_dist
        out["vae.mean"], out["vae.logvar"] = post.mean, post.logvar
        out["vae.decode"] = self.vae.decode(z, return_dict=False)[0]
        return {k: v.clone() for k, v in out.items()}


def test_every_executor_follows_a_write_to_one_parameter(dev):
    oracle = O.build_triplet(O.TINY_CONFIG, seed=81)
    vae_o = V.build(V.TINY_VAE_CONFIG, seed=82)
    fresh = lambda: (build_product_from_oracle(*oracle, torch.float16, dev), _vae(vae_o, dev))
    nets, vae = fresh()
    g = torch.Generator().manual_seed(83)
    inputs = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=84)]
    inputs += [torch.randn(2, 3, 32, 48, generator=g).to(dev).half(), torch.randn(2, 4, 16, 24, generator=g).to(dev).half()]
    warm = _Executors(nets, vae)
    prev = warm.run(*inputs)  # every cache is warm
    for role, suffixes, vae_suffix in ROLES:
        for net, suffix in zip(nets, suffixes):
            _bump(net, suffix)
        _bump(vae, vae_suffix)
        got = warm.run(*inputs)
        nets2, vae2 = fresh()
        for a, b in zip(nets2 + [vae2], list(nets) + [vae]):
            a.load_state_dict(b.state_dict())
        want = _Executors(nets2, vae2).run(*inputs)
        for k in want:
            assert bool(torch.isfinite(want[k]).all()), (role, k)
            assert torch.equal(got[k], want[k]), (role, k, float((got[k].float() - want[k].float()).abs().max()))
        assert not torch.equal(got["grouped.img"], prev["grouped.img"]) or not torch.equal(got["grouped.attr"], prev["grouped.attr"]), role
        prev = got
