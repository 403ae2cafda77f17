"""The ControlNet fixture shared by tests/test_control_host.py, tests/test_control_kernels_gpu.py and tests/test_control_request_gpu.py (test
infrastructure): the grouped launch's problems with their fp64 reference and per-element bar, the tile walk restated for the plan test, and
the reduced UNet + ControlNet of the request tests. Nothing in here calls the code under test."""
import numpy as np
import torch

TILE_M, TILE_N = 128, 64
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}       # unit roundoff of the storage type


# ---- one problem of the grouped launch: CPU tensors rounded to the storage type, so the fp64 reference sees what the kernel sees

def problem(seed, M, K, N, dtype, hw=None, B=1):
    """h [B, K, H, W], w [N, K, 1, 1], b [N], skip [B, N, H, W] (NCHW-shaped CPU tensors of `dtype`; B H W = M), seeded per problem so that
    every problem of a table has its own weights."""
    g = torch.Generator().manual_seed(9000 + seed)
    H, W = hw if hw is not None else (1, M // B)
    assert B * H * W == M
    h = torch.randn(B, K, H, W, generator=g).to(dtype)
    w = (torch.randn(N, K, 1, 1, generator=g) / K ** 0.5).to(dtype)
    b = (0.5 * torch.randn(N, generator=g)).to(dtype)
    skip = torch.randn(B, N, H, W, generator=g).to(dtype)
    return dict(h=h, w=w, b=b, skip=skip, M=M, K=K, N=N)


def reference(p, s, with_skip=True):
    """fp64: (ref [B, N, H, W], bar-free magnitude sum_k |h||w| + |b| of the same shape)."""
    h, w, b = p["h"].double(), p["w"].double()[:, :, 0, 0], p["b"].double()
    x = torch.einsum("bkhw,nk->bnhw", h, w) + b[None, :, None, None]
    mag = torch.einsum("bkhw,nk->bnhw", h.abs(), w.abs()) + b.abs()[None, :, None, None]
    ref = float(s) * x
    if with_skip:
        ref = ref + p["skip"].double()
    return ref, mag


def bar(p, s, ref, mag, dtype):
    """The issue's bar per element: u |ref| + K 2^-23 |s| (sum_k |h||w| + |b|) -- one rounding of the result to the storage type, and the fp32
    accumulation of K products. (The fp32 scale word itself is exact in the tests: the scales are fp32 numbers.)"""
    return U[dtype] * ref.abs() + p["K"] * 2.0 ** -23 * abs(float(s)) * mag


# the thirteen-problem table of the kernel test: C over {64, 128, 256} and M over {128, 32, 8, 2}, N != K in places, the order mixed so that
# the descending-K issue order differs from the caller's
THIRTEEN = [(128, 64, 64), (128, 64, 128), (32, 128, 128), (128, 256, 64), (32, 128, 64), (8, 256, 256), (32, 64, 256), (8, 256, 128), (8, 128, 256),
            (2, 256, 256), (2, 64, 64), (2, 128, 128), (2, 256, 64)]      # (M, K, N)


# ---- the tile walk, restated from the header's text

def expected_tiles(shapes):
    """shapes: [(M, N, K)] -> the SET of (problem, m0, n0) a launch must cover, each once."""
    out = []
    for p, (M, N, K) in enumerate(shapes):
        for m0 in range(0, M, TILE_M):
            for n0 in range(0, N, TILE_N):
                out.append((p, m0, n0))
    return out


PLAN_SWEEP = [
    [(1, 64, 64)],
    [(127, 64, 64)], [(128, 64, 64)], [(129, 64, 64)],
    [(129, 192, 64)], [(300, 64, 320)],
    [(1, 64, 64), (127, 128, 64), (128, 64, 128), (129, 192, 256)],
    [(M, N, K) for M, K, N in THIRTEEN],
    # SD1.5 at 2 rows: the thirteen zero convolutions
    [(8192, 320, 320)] * 3 + [(2048, 320, 320)] + [(2048, 640, 640)] * 2 + [(512, 640, 640)] + [(512, 1280, 1280)] * 2 + [(128, 1280, 1280)] * 4,
    [(5, 64, 64)] * 16,
]


# ---- the reduced models of the request tests

REQUEST_CONFIG = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(64, 128, 128, 128), layers_per_block=1,
                      attention_head_dim=(1, 2, 2, 2), cross_attention_dim=64, norm_num_groups=8, use_linear_projection=False)
SIDE = 128          # pixels: latents of 16^2, 8^2, 4^2, 2^2


HINT_GAIN = 4.0     # build_controlnet(hint_gain=): with nn's init the embedded control image is 0.014 std against conv_in(sample)'s 7.6 and mostly bias


def control_image(seed, side=SIDE):
    """A uint8 [side, side, 3] control image: 16 x 16 pixel blocks of seeded random colours (two seeds give uncorrelated images)."""
    rng = np.random.RandomState(700 + seed)
    blocks = rng.rand(side // 16, side // 16, 3)
    return (np.kron(blocks, np.ones((16, 16, 1))) * 255).round().astype(np.uint8)


def color_map(side=SIDE):
    """An RGB color map of `side` pixels with the colours of pww_cases.RUNNER_CONTEXT in quadrants (uint8 [side, side, 3])."""
    import pww_cases as cases
    colors = list(cases.RUNNER_CONTEXT)
    rgb = np.zeros((side, side, 3), dtype=np.uint8)
    half = side // 2
    for i, (y, x) in enumerate(((0, 0), (0, half), (half, 0), (half, half))):
        rgb[y:y + half, x:x + half] = colors[i % len(colors)]
    return rgb


PROMPT = "realistic photo of a dog, cat, tree, with beautiful sky, on sandy ground"
STEPS, GUIDANCE, CAP = 3, 7.5, 1e-2          # CAP: the project's fp16 bar on the final latent's rel-L2 (bench.py, config 3)


def build_request_tools(device, dtype=torch.float16, nets=1):
    """((vae, unet, text_encoder, tokenizer, scheduler), [ControlNets]): the reduced stand-ins in channels_last memory, seeded."""
    from sd_standin import build_unet, build_controlnet, HashTokenizer, TinyTextEncoder, TinyVAE, LMSDiscreteScheduler
    unet = build_unet(REQUEST_CONFIG, seed=1234, dtype=dtype, device=device, qk_gain=2.0).to(memory_format=torch.channels_last)
    text = TinyTextEncoder(REQUEST_CONFIG["cross_attention_dim"], seed=1235).to(device=device, dtype=dtype)
    vae = TinyVAE(4, seed=1236).to(device=device, dtype=dtype)
    sch = LMSDiscreteScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000)
    cnets = [build_controlnet(REQUEST_CONFIG, seed=1239 + k, dtype=dtype, device=device, hint_gain=HINT_GAIN).to(memory_format=torch.channels_last)
             for k in range(nets)]
    return (vae, unet, text, HashTokenizer(), sch), cnets
