"""Region strength on the GPU: the three launches of libpww_hip_hold.so bit for bit against their restatements, whole img2img loops with a
hold in the three modes against the oracle loop, the two consequences of the definition (equal strengths are the plain call; an s = 0 region
comes back as the init latent), and hipGraph mode keeping its one graph.

Expected values never come from the code under test: the launches are restated in numpy fp32 (tests/hold_cases.py), and the loop is
tests/hold_cases.py::oracle_hold_loop -- the oracle's img2img loop with the restated hold behind every scheduler step -- whose final latents
are recorded in tests/golden/hold_oracle.npz (tests/test_hold_host.py holds the record to fresh runs, and checks that the plain loop lies
0.94 rel-L2 away from the loop that keeps half of the image, against caps of 1e-2 (fp16) and 5e-2 (bf16))."""
import importlib

import numpy as np
import pytest
import torch
from PIL import Image

import hold_cases as H
import pww_cases as cases
from gpu_util import install_unfused, uninstall_all, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
THETAS = (0.0, 0.125, 0.375, 0.5, 1.0, 1.5)         # k / 8 (S == theta occurs and releases), nothing held, everything held


# ---- the three launches

def _apply_check(gpu_device, n, C, hw, offset=0):
    """Every (theta, a, b) of one shape; offset = 1: the same values in views that start one element into their buffers (4-byte aligned)."""
    from pww_hip import ops
    x, x0, z, S = H.apply_inputs(n, C, hw)

    def dev(a):
        buf = torch.zeros(a.size + offset, dtype=torch.float32, device=gpu_device)
        view = buf[offset:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16
        return view
    d0, dz, dS = dev(x0), dev(z), dev(S)
    for theta in THETAS:
        for a, b in H.APPLY_AB:
            dx = dev(x)
            got = ops.hold_apply(dx, d0, dz, dS, theta, a, b)
            assert got.data_ptr() == dx.data_ptr()                                     # in place
            want = H.apply(x, x0, z, S, theta, a, b)
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (n, C, hw, theta, a, b)
            held = S < np.float32(theta)
            if theta == 0.0:
                assert not held.any() and np.array_equal(want, x, equal_nan=True)      # nothing changes
            if theta == 1.5:
                assert held.all() and np.isfinite(want).all()                          # everything is held: the NaN and the infs are gone
            if theta == 0.375:
                # planted in held pixels (S = 0, 1/8, 2/8): overwritten; planted in released pixels (S = 6/8, 7/8, 1): untouched
                assert np.isfinite(want[0, 0, :3]).all() and np.isnan(want[0, C - 1, 6]) and np.isinf(want[0, C - 1, 7:9]).all()
            if theta == 0.5:
                assert held[0, 3] and not held[0, 4]                                   # S = 4 / 8 = theta releases
    assert np.array_equal(d0.cpu().numpy(), x0) and np.array_equal(dz.cpu().numpy(), z) and np.array_equal(dS.cpu().numpy(), S)      # read only


@pytest.mark.parametrize("shape", H.APPLY_CASES, ids=["x".join(map(str, s)) for s in H.APPLY_CASES])
def test_hold_apply_bit_for_bit(gpu_device, shape):
    _apply_check(gpu_device, *shape)


def test_hold_apply_on_unaligned_views(gpu_device):
    _apply_check(gpu_device, 1, 4, 64, offset=1)


def test_hold_apply_takes_a_latent_and_checks_its_arguments(gpu_device):
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    x, x0, z, S = (torch.from_numpy(a).to(gpu_device) for a in H.apply_inputs(2, 4, 64))
    got = ops.hold_apply(x.view(2, 4, 8, 8).clone(), x0.view(2, 4, 8, 8), z.view(2, 4, 8, 8), S.view(2, 8, 8), 0.5, 0.6, 0.8)
    assert np.array_equal(got.cpu().numpy().reshape(2, 4, 64), H.apply(*(t.cpu().numpy() for t in (x, x0, z, S)), 0.5, 0.6, 0.8), equal_nan=True)
    for bad, match in (((x.half(), x0, z, S), "float32"), ((x, x0[:1], z, S), "does not go"), ((x, x0, z, S[:, :32]), "does not go"),
                       ((x.transpose(0, 1), x0.transpose(0, 1), z.transpose(0, 1), S), "does not go"), ((x[:, :, ::2], x0[:, :, ::2], z[:, :, ::2], S[:, ::2]), "contiguous"),
                       ((x, x0.cpu(), z, S), "HIP device")):
        with pytest.raises(PwwHipError, match=match):
            ops.hold_apply(*bad, 0.5, 1.0, 1.0)
    with pytest.raises(PwwHipError, match="finite"):
        ops.hold_apply(x, x0, z, S, float("nan"), 1.0, 1.0)


@pytest.mark.parametrize("size", H.MAP_SIZES, ids=["%dx%d" % s for s in H.MAP_SIZES])
def test_strength_map_bit_for_bit(gpu_device, size):
    from pww_hip import ops
    Hh, W = size
    rgb = H.map_rgb(Hh, W, H.COLORS8)
    dev = torch.from_numpy(rgb).to(gpu_device)
    for K in (1, 8):
        for s0 in (0.5, 0.0, 1.0):
            got = ops.hold_strength_map(dev, H.COLORS8[:K], H.STRENGTHS8[:K], s0)
            want = H.strength_map(rgb, H.COLORS8[:K], H.STRENGTHS8[:K], s0)
            assert got.dtype == torch.float32 and tuple(got.shape) == (Hh // 8, W // 8) and np.array_equal(got.cpu().numpy(), want), (K, s0)
            assert want.min() >= 0 and want.max() <= 1
    assert len(np.unique(want)) > 8                                                      # blocks with mixed colours: the map is no step function
    # a colour that is absent from the map: the base strength everywhere
    got = ops.hold_strength_map(dev, [(9, 9, 9)], [1.0], 0.3)
    assert np.array_equal(got.cpu().numpy(), np.full((Hh // 8, W // 8), np.float32(0.3)))
    # a map of one colour: that colour's strength everywhere, whatever else is named
    one = H.map_rgb(Hh, W, H.COLORS8, single=H.COLORS8[5])
    got = ops.hold_strength_map(torch.from_numpy(one).to(gpu_device), H.COLORS8, H.STRENGTHS8, 0.5)
    assert np.array_equal(got.cpu().numpy(), H.strength_map(one, H.COLORS8, H.STRENGTHS8, 0.5))
    assert np.allclose(got.cpu().numpy(), H.STRENGTHS8[5], atol=1e-7)
    # with a feather: the two more launches, in place on the map
    got = ops.hold_strength_map(dev, H.COLORS8, H.STRENGTHS8, 0.5, 2.0)
    assert np.array_equal(got.cpu().numpy(), H.strength_map(rgb, H.COLORS8, H.STRENGTHS8, 0.5, 2.0))


@pytest.mark.parametrize("shape", H.FEATHER_CASES, ids=["%dx%d" % s for s in H.FEATHER_CASES])
def test_feather_bit_for_bit(gpu_device, shape):
    from pww_hip import ops
    g = torch.Generator().manual_seed(shape[0] * shape[1])
    plane = (torch.randint(0, 65, shape, generator=g).float() / 64)
    plane[0, :3] = torch.tensor([0.0, 1.0, 1.0])
    plane[-1, -2:] = 1.0
    dev = plane.to(gpu_device)
    for sigma in H.FEATHER_SIGMAS:
        got = ops.hold_feather(dev, sigma).cpu().numpy()
        want = H.feather(plane.numpy(), sigma)
        assert np.array_equal(got, want), (shape, sigma)
        assert got.min() >= 0.0 and got.max() <= 1.0                                    # a normalised mean of values in [0, 1]
        assert not np.array_equal(got, plane.numpy())
    assert torch.equal(dev.cpu(), plane)                                                # the input plane is read only
    assert np.array_equal(ops.hold_feather(torch.ones(shape, device=gpu_device), 8.0).cpu().numpy(), np.ones(shape, dtype=np.float32))


# ---- whole loops

def _set_mode(mode):
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    return pww_mod, old


def _hip_loop(tools, device, mode, name=None, fused=True, steps=H.STEPS, keep=None, **kw):
    """paint_with_words as img2img on the inputs of loop `name`, with its region strengths (keywords override them); the global generator is
    seeded like the oracle loop seeds it. keep: a dict that receives the x0 and z the request was made of."""
    import paint_with_words as pw
    from pww_hip import sampler as S
    rgb, init, region_strength, strength, sigma, canvas = H.loop_inputs(name)
    pww_mod, old = _set_mode(mode)
    orig_install, orig_held = S.install, pww_mod._held_images
    if not fused:
        S.install = install_unfused        # calibration path: same driver, attention as unfused torch ops
    if keep is not None:
        def held(*a, **k):
            out = orig_held(*a, **k)
            keep["init"], keep["noise"] = out[2].clone(), out[3].clone()
            return out
        pww_mod._held_images = held
    args = dict(strength=strength, region_strength=region_strength, region_strength_feather=sigma)
    if canvas:
        args.update(canvas_window=H.WINDOW, canvas_stride=H.STRIDE)
    args.update(kw)
    try:
        torch.manual_seed(H.SEED)
        return pw.paint_with_words(color_context=dict(cases.RUNNER_CONTEXT), color_map_image=Image.fromarray(rgb), input_prompt=cases.RUNNER_PROMPT,
                                   num_inference_steps=steps, guidance_scale=H.GUIDANCE, seed=0, device=str(device), weight_function=cases.weight_fn_runner,
                                   preloaded_utils=tools, return_latents=True, init_image=Image.fromarray(init), **args).clone()
    finally:
        S.install, pww_mod._held_images = orig_install, orig_held
        pww_mod.DEFAULT_MODE = old
        if not fused:
            uninstall_all()


@pytest.fixture(scope="module")
def oracle_latents():
    return H.recorded()


_UNFUSED = {}


def _unfused_drift(gpu_device, oracle_latents, dtype, name):
    """rel-L2 of the unfused torch path -- the same driver and the same hold launch, attention as torch ops in `dtype` -- against the oracle
    loop, once per (dtype, loop)."""
    if (dtype, name) not in _UNFUSED:
        tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=H.QK_GAIN)
        try:
            _UNFUSED[dtype, name] = rel_l2(_hip_loop(tools, gpu_device, "eager", name, fused=False), oracle_latents[name])
        finally:
            uninstall_all()
    return _UNFUSED[dtype, name]


@pytest.mark.parametrize("name", [n for n in H.LOOPS if n != "plain"])
@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
@DTYPES
def test_tiny_hold_loop_vs_oracle(gpu_device, oracle_latents, dtype, mode, name):
    d0 = _unfused_drift(gpu_device, oracle_latents, dtype, name)
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=H.QK_GAIN)
    try:
        lat = _hip_loop(tools, gpu_device, mode, name)
    finally:
        uninstall_all()
    d = rel_l2(lat, oracle_latents[name])
    print(f"hold loop {name} {dtype} {mode}: rel-L2 hip {d:.3e} unfused-torch {d0:.3e}")
    assert tuple(lat.shape) == tuple(oracle_latents[name].shape) and lat.dtype == torch.float32
    assert d <= H.CAP[dtype]
    assert d <= H.UNFUSED_SLACK[0] * d0 + H.UNFUSED_SLACK[1]


@DTYPES
def test_the_plain_call_lies_outside_the_cap(gpu_device, oracle_latents, dtype):
    """The plain img2img call at the largest strength lands on the plain oracle loop and far from the loop that keeps half of the image: the
    caps above would not pass a build that ignored the strengths."""
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=H.QK_GAIN)
    try:
        plain = _hip_loop(tools, gpu_device, "graph", "plain")
    finally:
        uninstall_all()
    d_keep, d_plain = rel_l2(plain, oracle_latents["half_keep"]), rel_l2(plain, oracle_latents["plain"])
    print(f"plain img2img {dtype}: vs the half_keep oracle loop {d_keep:.3e}, vs the plain oracle loop {d_plain:.3e}")
    assert d_keep > 4 * max(H.CAP.values()) > H.CAP[dtype]
    assert d_plain <= {torch.float16: 2e-2, torch.bfloat16: 1e-1}[dtype]          # the plain loop's own caps (tests/test_loop_gpu.py)


# ---- the two consequences of the definition

@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
def test_equal_strengths_are_the_plain_call(gpu_device, mode):
    """T = 8, s = 0.5: every named strength equal to `strength`, and a named colour that does not occur in the map, are torch.equal to the
    plain img2img call of the same mode after the same torch.manual_seed -- nothing is ever held, and the steps are the same.
    (The stock PyTorch-ROCm convolutions of the UNet are not repeatable run to run by default -- DESIGN.md: two identical calls agree to
    ~5e-3 -- so the plain call is not torch.equal to ITSELF then; with torch.backends.cudnn.deterministic, a stock setting, it is, which the
    test asserts first. Measured without the setting: plain vs plain 4.9e-3, equal strengths vs plain 4.8e-3 rel-L2.)"""
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=H.QK_GAIN)
    stock = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        plain = _hip_loop(tools, gpu_device, mode, "half_keep", strength=0.5, region_strength=None)
        again = _hip_loop(tools, gpu_device, mode, "half_keep", strength=0.5, region_strength=None)
        equal = _hip_loop(tools, gpu_device, mode, "half_keep", strength=0.5, region_strength={H.A: 0.5, "#%02x%02x%02x" % H.B: 0.5})
        absent = _hip_loop(tools, gpu_device, mode, "half_keep", strength=0.5, region_strength={(1, 2, 3): 0.25})
        moved = _hip_loop(tools, gpu_device, mode, "half_keep", strength=0.5, region_strength={H.A: 0.25})
    finally:
        torch.backends.cudnn.deterministic = stock
        uninstall_all()
    print(f"equal strengths {mode}: plain vs plain again equal={torch.equal(plain, again)}, vs equal strengths {rel_l2(equal, plain):.3e}, "
          f"vs an absent colour {rel_l2(absent, plain):.3e}, vs another strength {rel_l2(moved, plain):.3e}")
    assert torch.equal(again, plain)                                                 # the yardstick is repeatable
    assert torch.equal(equal, plain)
    assert torch.equal(absent, plain)
    assert rel_l2(moved, plain) > 4e-2                                               # and a strength that differs shows


@pytest.mark.parametrize("mode", ["eager", "graph"])
@DTYPES
def test_the_kept_region_is_the_init_latent(gpu_device, dtype, mode):
    """half_keep: the left half has s = 0, feather 0 and whole 8 x 8 blocks -- it comes back as x0, bit for bit; the rest has moved."""
    tools = cases.build_tools("tiny", dtype=dtype, device=gpu_device, qk_gain=H.QK_GAIN)
    keep = {}
    try:
        lat = _hip_loop(tools, gpu_device, mode, "half_keep", keep=keep)
    finally:
        uninstall_all()
    x0 = keep["init"]
    assert x0.dtype == torch.float32 and tuple(x0.shape) == tuple(lat.shape) == (1, 4, 8, 8)
    assert torch.equal(lat[..., :4], x0[..., :4])
    assert rel_l2(lat[..., 4:], x0[..., 4:]) > 0.1
    # and x0 is the oracle's, up to the VAE's type: four roundings (image, weight, sum, output) of unit roundoff 2^-11 / 2^-8
    assert rel_l2(x0, H.init_latent("half_keep")) <= {torch.float16: 4 * 2.0 ** -11, torch.bfloat16: 4 * 2.0 ** -8}[dtype]


# ---- hipGraph mode keeps its one graph

def test_graph_captures(gpu_device):
    tools = cases.build_tools("tiny", dtype=torch.float16, device=gpu_device, qk_gain=H.QK_GAIN)
    try:
        plain = _hip_loop(tools, gpu_device, "graph", "plain")
        sampler = tools[1]._pww_samplers[(id(tools[4]), "graph")]
        assert sampler._graphed.captures == 1 and len(sampler._graphed.graphs) == 1            # one capture for all steps
        a = _hip_loop(tools, gpu_device, "graph", "half_keep")
        assert sampler._graphed.captures == 1                                                  # the hold launch is outside the graph: replayed
        b = _hip_loop(tools, gpu_device, "graph", "half_keep", region_strength={H.A: 0.25, H.D: 0.5}, region_strength_feather=1.0)
        assert sampler._graphed.captures == 1                                                  # another strength dict, a feather: replayed
        a_eager = _hip_loop(tools, gpu_device, "eager", "half_keep")
        assert rel_l2(a, a_eager) <= 2e-2 and rel_l2(a, plain) > 4e-2 and rel_l2(a, b) > 4e-2
    finally:
        uninstall_all()

