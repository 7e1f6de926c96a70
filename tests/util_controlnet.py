"""ControlNetModel oracle for the tests (reference models/controlnet.py:2530-3266, restated): a subclass of the oracle's
``AttributeEncoderModel`` -- the same trunk -- that adds diffusers' ``ControlNetConditioningEmbedding`` (eight nn.Conv2d) and
follows the reference forward: ``sample = conv_in(sample) + controlnet_cond_embedding(cond)``, down, mid, 12 + 1 zero
convs, scaling (``guess_mode``: torch.logspace(-1, 0, 13) * conditioning_scale).  fp32 on the CPU; ``oracle/`` is untouched."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from util_models import O

EMB_CHANNELS = (16, 32, 96, 256)
SD_PARAMS, TINY_PARAMS = 361_279_120, 5_739_408  # trunk 360,192,640 / 5,243,008 (in_channels = 4) + embedding 1,086,480 / 496,400


class ConditioningEmbedding(nn.Module):
    def __init__(self, out_channels, cond_channels=3, widths=EMB_CHANNELS):
        super().__init__()
        self.conv_in = nn.Conv2d(cond_channels, widths[0], 3, padding=1)
        self.blocks = nn.ModuleList()
        for a, b in zip(widths[:-1], widths[1:]):
            self.blocks.append(nn.Conv2d(a, a, 3, padding=1))
            self.blocks.append(nn.Conv2d(a, b, 3, padding=1, stride=2))
        self.conv_out = nn.Conv2d(widths[-1], out_channels, 3, padding=1)
        nn.init.zeros_(self.conv_out.weight)
        nn.init.zeros_(self.conv_out.bias)

    def forward(self, cond):
        x = F.silu(self.conv_in(cond))
        for blk in self.blocks:
            x = F.silu(blk(x))
        return self.conv_out(x)


class ControlNetOracle(O.AttributeEncoderModel):
    def __init__(self, channel_order="rgb", conditioning_channels=3, **cfg):
        super().__init__(**cfg)
        self.channel_order = channel_order
        self.controlnet_cond_embedding = ConditioningEmbedding(self.cfg["block_out_channels"][0], conditioning_channels)

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, guess_mode=False):
        if self.channel_order == "bgr":
            controlnet_cond = torch.flip(controlnet_cond, dims=[1])
        emb = self._emb(timestep, sample.shape[0])  # ref 3154: expanded to the batch
        x = self.conv_in(sample) + self.controlnet_cond_embedding(controlnet_cond)  # ref 3201-3204
        skips = (x,)
        for blk in self.down_blocks:
            x, st = blk(x, emb, encoder_hidden_states)
            skips += st
        x = self.mid_block(x, emb, encoder_hidden_states)
        res = [z(s) for s, z in zip(skips, self.controlnet_down_blocks)]
        mid = self.controlnet_mid_block(x)
        if guess_mode:  # ref 3245-3249
            scales = torch.logspace(-1, 0, len(res) + 1) * conditioning_scale
            return [r * s for r, s in zip(res, scales)], mid * scales[-1]
        return [r * conditioning_scale for r in res], mid * conditioning_scale  # ref 3251-3252


def trunk_config(cfg):
    return {k: v for k, v in cfg.items() if k not in ("out_channels", "up_block_types")}


def randomize(net, std=0.02, seed=4321):
    """The zero-initialised convs teach nothing: the embedding's conv_out and the 12 + 1 zero convs get N(0, std^2)."""
    g = torch.Generator().manual_seed(seed)
    for m in [net.controlnet_cond_embedding.conv_out] + list(net.controlnet_down_blocks) + [net.controlnet_mid_block]:
        m.weight.data = torch.randn(m.weight.shape, generator=g) * std
        m.bias.data = torch.randn(m.bias.shape, generator=g) * std


def build_oracle(cfg, seed=1234, channel_order="rgb", fp16_weights=False):
    torch.manual_seed(seed)
    net = ControlNetOracle(channel_order=channel_order, **trunk_config(cfg))
    randomize(net)
    if fp16_weights:
        for p in net.parameters():
            p.data = p.data.to(torch.float16).to(torch.float32)
    return net.eval()


def build_product(oracle, dtype=None, dev=None):
    import uni_renderer_amd as U

    net = U.ControlNetModel(controlnet_conditioning_channel_order=oracle.channel_order, **trunk_config(oracle.cfg))
    net.load_state_dict(oracle.state_dict())
    if dtype is not None:
        net = net.to(dtype)
    if dev is not None:
        net = net.to(dev)
    return net.eval().requires_grad_(False)


def make_inputs(B, latent_hw, cond_hw, cross_dim, seed=99):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, *latent_hw, generator=g)
    cond = torch.rand(B, 3, *cond_hw, generator=g)  # an image: uniform in [0, 1]
    ehs = torch.randn(B, 77, cross_dim, generator=g) * 0.5
    t = torch.randint(0, 1000, (B,), generator=g).long()
    return x, cond, ehs, t
