"""Stand-in for the diffusers (>= 0.14) ``ControlNetModel``: the UNet stand-in's own down path and mid block (sd_standin/unet.py), a small
convolutional embedding of the control image, and one 1 x 1 "zero convolution" per skip tensor of the UNet plus one for the mid block.

``diffusers`` is not installable here, so the topology is restated from the published architecture (Zhang et al. 2023, "Adding Conditional
Control to Text-to-Image Diffusion Models") with diffusers' attribute names: ``conv_in``, ``time_embedding``, ``down_blocks``, ``mid_block``,
``controlnet_cond_embedding`` (``conv_in``, ``blocks``, ``conv_out``), ``controlnet_down_blocks``, ``controlnet_mid_block``. Weights are
random-init from a seed, as in build_unet; a trained ControlNet's zero convolutions are not zero, so the default leaves them at nn's init.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from .unet import DownBlock, MidBlock, SD15_CONFIG, timestep_embedding


class ControlNetConditioningEmbedding(nn.Module):
    """Control image [B, 3, 8 h, 8 w] -> [B, block_out_channels[0], h, w]: conv_in, six blocks (three of stride 2), conv_out; SiLU after
    every convolution but the last."""

    def __init__(self, conditioning_embedding_channels, conditioning_channels=3, block_out_channels=(16, 32, 96, 256)):
        super().__init__()
        self.conv_in = nn.Conv2d(conditioning_channels, block_out_channels[0], 3, padding=1)
        self.blocks = nn.ModuleList()
        for i in range(len(block_out_channels) - 1):
            cin, cout = block_out_channels[i], block_out_channels[i + 1]
            self.blocks.append(nn.Conv2d(cin, cin, 3, padding=1))
            self.blocks.append(nn.Conv2d(cin, cout, 3, padding=1, stride=2))
        self.conv_out = nn.Conv2d(block_out_channels[-1], conditioning_embedding_channels, 3, padding=1)

    def forward(self, conditioning):
        x = F.silu(self.conv_in(conditioning))
        for blk in self.blocks:
            x = F.silu(blk(x))
        return self.conv_out(x)


class ControlNetModel(nn.Module):
    def __init__(self, sample_size=64, in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                 attention_head_dim=8, cross_attention_dim=768, norm_num_groups=32, use_linear_projection=False, conditioning_channels=3,
                 conditioning_embedding_out_channels=(16, 32, 96, 256)):
        super().__init__()
        self.in_channels = in_channels
        self.config = SimpleNamespace(sample_size=sample_size, in_channels=in_channels, block_out_channels=tuple(block_out_channels),
                                      layers_per_block=layers_per_block, attention_head_dim=attention_head_dim,
                                      cross_attention_dim=cross_attention_dim, conditioning_channels=conditioning_channels)
        nblocks = len(block_out_channels)
        heads = attention_head_dim if isinstance(attention_head_dim, (tuple, list)) else (attention_head_dim,) * nblocks
        temb_ch = block_out_channels[0] * 4
        g = norm_num_groups
        self.time_proj_dim = block_out_channels[0]
        self.time_embedding = nn.ModuleList([nn.Linear(block_out_channels[0], temb_ch), nn.Linear(temb_ch, temb_ch)])
        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(block_out_channels[0], conditioning_channels,
                                                                         conditioning_embedding_out_channels)
        self.down_blocks = nn.ModuleList()
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(block_out_channels[0], block_out_channels[0], 1)])      # conv_in's skip
        out_ch = block_out_channels[0]
        for i in range(nblocks):
            in_ch, out_ch = out_ch, block_out_channels[i]
            last = i == nblocks - 1
            self.down_blocks.append(DownBlock(in_ch, out_ch, temb_ch, layers_per_block, heads[i], cross_attention_dim, has_attn=not last,
                                              add_down=not last, groups=g, linear_proj=use_linear_projection))
            for _ in range(layers_per_block + (0 if last else 1)):          # one per skip of the block: its layers, then its downsampler
                self.controlnet_down_blocks.append(nn.Conv2d(out_ch, out_ch, 1))
        self.mid_block = MidBlock(block_out_channels[-1], temb_ch, heads[-1], cross_attention_dim, g, use_linear_projection)
        self.controlnet_mid_block = nn.Conv2d(block_out_channels[-1], block_out_channels[-1], 1)

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    @property
    def device(self):
        return self.conv_in.weight.device

    def hidden_states(self, sample, timestep, encoder_hidden_states, hint):
        """The ControlNet's encoder on `sample` with the embedded control image `hint` added behind conv_in -> (the hidden states the
        controlnet_down_blocks read, in their order; the hidden state controlnet_mid_block reads)."""
        if not torch.is_tensor(timestep):
            timestep = torch.tensor([timestep], dtype=torch.float32, device=sample.device)
        timestep = timestep.to(sample.device).reshape(-1).expand(sample.shape[0])
        temb = timestep_embedding(timestep, self.time_proj_dim).to(self.dtype)
        temb = self.time_embedding[1](F.silu(self.time_embedding[0](temb)))
        x = self.conv_in(sample.to(self.dtype)) + hint
        hs = (x,)
        for blk in self.down_blocks:
            x, outs = blk(x, temb, encoder_hidden_states)
            hs += outs
        return hs, self.mid_block(x, temb, encoder_hidden_states)

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0):
        hint = self.controlnet_cond_embedding(controlnet_cond.to(self.dtype))
        hs, mid = self.hidden_states(sample, timestep, encoder_hidden_states, hint)
        down_block_res_samples = tuple(conv(h) * conditioning_scale for conv, h in zip(self.controlnet_down_blocks, hs))
        mid_block_res_sample = self.controlnet_mid_block(mid) * conditioning_scale
        return down_block_res_samples, mid_block_res_sample


def build_controlnet(config=None, seed=1239, dtype=torch.float32, device="cpu", zero_init=False, hint_gain=1.0):
    """Random-init ControlNet with a fixed seed, as build_unet builds the UNet; the global RNG stream is left where it was. `config` is a
    UNet config (the keys a ControlNet has no use for are dropped). zero_init=True zeroes the zero convolutions, as an untrained ControlNet
    has them; the default keeps nn's init, as a trained one's are not zero. ``hint_gain`` optionally scales the weights of the eight
    convolutions of controlnet_cond_embedding, as build_unet's qk_gain scales to_q: with nn's init the embedded control image has a
    hundredth of the magnitude of conv_in(sample) and is mostly bias, so the image would hardly matter; 1.0 keeps the default init."""
    cfg = dict(SD15_CONFIG if config is None else config)
    cfg.pop("out_channels", None)
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        net = ControlNetModel(**cfg)
    finally:
        torch.random.set_rng_state(gen_state)
    if hint_gain != 1.0:
        emb = net.controlnet_cond_embedding
        with torch.no_grad():
            for conv in [emb.conv_in] + list(emb.blocks) + [emb.conv_out]:
                conv.weight.mul_(hint_gain)
    if zero_init:
        with torch.no_grad():
            for conv in list(net.controlnet_down_blocks) + [net.controlnet_mid_block]:
                conv.weight.zero_()
                conv.bias.zero_()
    return net.to(device=device, dtype=dtype).eval().requires_grad_(False)
