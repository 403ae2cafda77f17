"""Minimal AutoencoderKL stand-in: the hot path ends at the final latent (parity is checked there);
the reference only needs ``vae.decode(z).sample`` (paint_with_words/paint_with_words.py:50) and, for
img2img / inpaint, ``vae.encode(x).latent_dist.sample()`` (:461-462).

``TinyVAE`` is that minimum (what every loop test and bench.py use); ``AutoencoderKL`` below is the real Stable Diffusion DECODER topology
with random seeded weights, the module `pww_hip.vae.decode` runs on the native path; ``AutoencoderKLEncDec`` adds the real ENCODER topology
(and `encode(x).latent_dist` as the diagonal Gaussian), the module `pww_hip.vae_encode.encode` runs on the native path."""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F


class TinyVAE(nn.Module):
    def __init__(self, latent_channels=4, seed=1236):
        super().__init__()
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        try:
            self.dec = nn.Conv2d(latent_channels, 3, 3, padding=1)
            self.enc = nn.Conv2d(3, latent_channels, 8, stride=8)
        finally:
            torch.random.set_rng_state(state)
        self.requires_grad_(False)

    @property
    def dtype(self):
        return self.dec.weight.dtype

    def decode(self, z):
        x = F.interpolate(self.dec(z.to(self.dtype)), scale_factor=8.0, mode="nearest")
        return SimpleNamespace(sample=torch.tanh(x))

    def encode(self, x):
        mean = self.enc(x.to(self.dtype))
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: mean, mode=lambda: mean))


# ---- the Stable Diffusion 1.x / 2.x decoder, restated from the published architecture with the attribute names of diffusers 0.10.0 -----------
class VaeResnetBlock2D(nn.Module):
    """ResnetBlock2D without a time embedding: x + conv2(silu(norm2(conv1(silu(norm1(x)))))), a 1 x 1 shortcut where the channels change."""

    def __init__(self, in_channels, out_channels, groups=32, eps=1e-6):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, in_channels, eps=eps)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, out_channels, eps=eps)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None

    def forward(self, x, temb=None):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        if self.conv_shortcut is not None:
            x = self.conv_shortcut(x)
        return x + h


class AttentionBlock(nn.Module):
    """One head over the H W positions: x + proj_attn(softmax(q k^T / sqrt(C)) v) on group_norm(x)."""

    def __init__(self, channels, groups=32, eps=1e-6):
        super().__init__()
        self.channels = channels
        self.num_heads = 1
        self.group_norm = nn.GroupNorm(groups, channels, eps=eps)
        self.query = nn.Linear(channels, channels)
        self.key = nn.Linear(channels, channels)
        self.value = nn.Linear(channels, channels)
        self.proj_attn = nn.Linear(channels, channels)

    def forward(self, x):
        B, C, H, W = x.shape
        t = self.group_norm(x).reshape(B, C, H * W).transpose(1, 2)
        q, k, v = self.query(t), self.key(t), self.value(t)
        probs = torch.softmax((torch.bmm(q, k.transpose(1, 2)) * (C ** -0.5)).float(), dim=-1).to(q.dtype)
        out = self.proj_attn(torch.bmm(probs, v))
        return out.transpose(1, 2).reshape(B, C, H, W) + x


class VaeUpsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class VaeMidBlock(nn.Module):
    def __init__(self, channels, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock2D(channels, channels, groups, eps), VaeResnetBlock2D(channels, channels, groups, eps)])
        self.attentions = nn.ModuleList([AttentionBlock(channels, groups, eps)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class VaeUpBlock(nn.Module):
    def __init__(self, in_channels, out_channels, layers, add_upsample, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, groups, eps) for i in range(layers)])
        self.upsamplers = nn.ModuleList([VaeUpsample2D(out_channels)]) if add_upsample else None

    def forward(self, x):
        for resnet in self.resnets:
            x = resnet(x)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class VaeDecoder(nn.Module):
    def __init__(self, latent_channels, out_channels, block_out_channels, layers_per_block, groups, eps):
        super().__init__()
        rev = list(reversed(block_out_channels))        # SD: 512, 512, 256, 128
        self.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
        self.mid_block = VaeMidBlock(rev[0], groups, eps)
        self.up_blocks = nn.ModuleList([VaeUpBlock(rev[max(i - 1, 0)], ch, layers_per_block + 1, i < len(rev) - 1, groups, eps) for i, ch in enumerate(rev)])
        self.conv_norm_out = nn.GroupNorm(groups, rev[-1], eps=eps)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(rev[-1], out_channels, 3, padding=1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for block in self.up_blocks:
            x = block(x)
        return self.conv_out(self.conv_act(self.conv_norm_out(x)))


SD_VAE_CONFIG = dict(latent_channels=4, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32)


class AutoencoderKL(nn.Module):
    """The decoder of the Stable Diffusion 1.x / 2.x VAE (post_quant_conv, decoder.conv_in, .mid_block with one AttentionBlock, four up blocks of
    three resnets, .conv_norm_out / SiLU / .conv_out; every GroupNorm 32 groups, eps 1e-6), random seeded weights. `decode(z).sample` is the
    reference's only use of it. The ENCODER is not restated: `encode` keeps TinyVAE's one strided convolution so that img2img and inpainting
    run on the class; it is a stand-in, not the SD encoder."""

    def __init__(self, latent_channels=4, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32, seed=1237):
        super().__init__()
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        try:
            self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)
            self.decoder = VaeDecoder(latent_channels, out_channels, block_out_channels, layers_per_block, norm_num_groups, 1e-6)
            self.enc = nn.Conv2d(3, latent_channels, 8, stride=8)
        finally:
            torch.random.set_rng_state(state)
        self.requires_grad_(False)

    @property
    def dtype(self):
        return self.post_quant_conv.weight.dtype

    def decode(self, z):
        return SimpleNamespace(sample=self.decoder(self.post_quant_conv(z.to(self.dtype))))

    def encode(self, x):
        mean = self.enc(x.to(self.dtype))
        return SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda generator=None: mean, mode=lambda: mean))


# ---- the encoder of the same VAE, restated from the published architecture with the attribute names of diffusers 0.10.0 ---------------------
class VaeDownsample2D(nn.Module):
    """Stride 2 with the padding on the right and bottom only: the taps of output o are the inputs 2 o + {0, 1, 2}."""

    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class VaeDownBlock(nn.Module):
    def __init__(self, in_channels, out_channels, layers, add_downsample, groups, eps):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, groups, eps) for i in range(layers)])
        self.downsamplers = nn.ModuleList([VaeDownsample2D(out_channels)]) if add_downsample else None

    def forward(self, x):
        for resnet in self.resnets:
            x = resnet(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class VaeEncoder(nn.Module):
    def __init__(self, in_channels, latent_channels, block_out_channels, layers_per_block, groups, eps):
        super().__init__()
        chs = list(block_out_channels)                  # SD: 128, 256, 512, 512
        self.conv_in = nn.Conv2d(in_channels, chs[0], 3, padding=1)
        self.down_blocks = nn.ModuleList([VaeDownBlock(chs[max(i - 1, 0)], ch, layers_per_block, i < len(chs) - 1, groups, eps) for i, ch in enumerate(chs)])
        self.mid_block = VaeMidBlock(chs[-1], groups, eps)
        self.conv_norm_out = nn.GroupNorm(groups, chs[-1], eps=eps)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(chs[-1], 2 * latent_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for block in self.down_blocks:
            x = block(x)
        return self.conv_out(self.conv_act(self.conv_norm_out(self.mid_block(x))))


class DiagonalGaussian:
    """The posterior `encode` returns as `.latent_dist`: mean | logvar are the two halves of the moments, logvar clamped to [-30, 20]."""

    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator=None):
        """THE statement of how the noise is drawn: fp32 normals of the mean's shape from `generator` (None: the default generator of the
        mean's device) on the mean's device, cast to its dtype."""
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device).to(self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean


class AutoencoderKLEncDec(AutoencoderKL):
    """AutoencoderKL with the ENCODER of the Stable Diffusion 1.x / 2.x VAE as well: encoder.conv_in (3 -> 128), four down blocks of two
    resnets (128, 256, 512, 512 channels; the first three end in a stride-2 downsampler padded on the right and bottom only), .mid_block with
    one AttentionBlock, .conv_norm_out / SiLU / .conv_out (512 -> 8), quant_conv (8 -> 8, 1 x 1); `encode(x).latent_dist` is the diagonal
    Gaussian of the moments. The decoder and post_quant_conv are those of AutoencoderKL(), bit for bit: the encoder's weights come from a
    seed of their own, drawn after the parent's. The module `pww_hip.vae_encode.encode` runs on the native path."""

    def __init__(self, in_channels=3, encoder_seed=1238, **kw):
        super().__init__(**kw)
        cfg = dict(SD_VAE_CONFIG, **{k: v for k, v in kw.items() if k in SD_VAE_CONFIG})
        state = torch.random.get_rng_state()
        torch.manual_seed(encoder_seed)
        try:
            self.encoder = VaeEncoder(in_channels, cfg["latent_channels"], cfg["block_out_channels"], cfg["layers_per_block"], cfg["norm_num_groups"], 1e-6)
            self.quant_conv = nn.Conv2d(2 * cfg["latent_channels"], 2 * cfg["latent_channels"], 1)
        finally:
            torch.random.set_rng_state(state)
        self.requires_grad_(False)

    def encode(self, x):
        return SimpleNamespace(latent_dist=DiagonalGaussian(self.quant_conv(self.encoder(x.to(self.dtype)))))
