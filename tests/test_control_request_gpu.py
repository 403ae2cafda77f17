"""ControlNet requests on the GPU: paint_with_words / paint_with_words_batch with a control image beside the colour map, 3 steps on the
reduced UNet + ControlNet of tests/control_cases.py (64 / 128 / 128 / 128 channels, 128 x 128 pixels: the grouped launch sees M = rows x
{256, 64, 16, 4}), under torch.backends.cudnn.deterministic as tests/test_hold_gpu.py runs its bitwise comparisons.

Measured on MI355X (fp16, final-latent rel-L2; profiles/control.md, section 3): the figures each test prints."""
import importlib

import pytest
import torch
from PIL import Image

import control_cases as CC
import pww_cases as cases
from gpu_util import uninstall_all, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def deterministic():
    stock = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = stock
    uninstall_all()


def _mode(mode):
    pww_mod = importlib.import_module("paint_with_words.paint_with_words")
    old, pww_mod.DEFAULT_MODE = pww_mod.DEFAULT_MODE, mode
    return pww_mod, old


def _run(tools, device, mode, batch=None, seed=3, **kw):
    """paint_with_words (batch=None) or paint_with_words_batch (batch = the seeds) -> the final latents."""
    import paint_with_words as pw
    pww_mod, old = _mode(mode)
    common = dict(num_inference_steps=CC.STEPS, guidance_scale=CC.GUIDANCE, device=str(device), weight_function=cases.weight_fn_runner,
                  preloaded_utils=tools, return_latents=True)
    common.update(kw)
    cmap = Image.fromarray(CC.color_map())
    try:
        if batch is None:
            return pw.paint_with_words(dict(cases.RUNNER_CONTEXT), cmap, CC.PROMPT, seed=seed, **common).clone()
        return pw.paint_with_words_batch(dict(cases.RUNNER_CONTEXT), cmap, CC.PROMPT, list(batch), **common).clone()
    finally:
        pww_mod.DEFAULT_MODE = old


def _sampler(tools, mode):
    pww_mod, old = _mode(mode)
    try:
        return pww_mod._sampler_for(tools[1], tools[4])
    finally:
        pww_mod.DEFAULT_MODE = old


A, B = CC.control_image(1), CC.control_image(2)


def test_the_keywords_are_accepted_and_the_control_image_steers(gpu_device):
    """Without the feature this call is a TypeError. txt2img and img2img; the result depends on the image and on the scale."""
    tools, (net,) = CC.build_request_tools(gpu_device)
    plain = _run(tools, gpu_device, "folded")
    a = _run(tools, gpu_device, "folded", controlnet=net, control_image=Image.fromarray(A))
    b = _run(tools, gpu_device, "folded", controlnet=net, control_image=B, controlnet_conditioning_scale=1.0)
    half = _run(tools, gpu_device, "folded", controlnet=net, control_image=torch.from_numpy(A).permute(2, 0, 1).float() / 255, controlnet_conditioning_scale=0.5)
    print("control vs none %.3e, image A vs B %.3e, scale 1 vs 0.5 %.3e" % (rel_l2(a, plain), rel_l2(a, b), rel_l2(a, half)))
    assert a.dtype == torch.float32 and tuple(a.shape) == (1, 4, 16, 16) and bool(torch.isfinite(a).all())
    assert rel_l2(a, plain) > 4 * CC.CAP and rel_l2(a, b) > CC.CAP and rel_l2(a, half) > CC.CAP
    init = Image.fromarray(cases.synthetic_init_image()).resize((CC.SIDE, CC.SIDE))
    torch.manual_seed(11)
    i_plain = _run(tools, gpu_device, "folded", init_image=init, strength=0.8)
    torch.manual_seed(11)
    i_ctl = _run(tools, gpu_device, "folded", init_image=init, strength=0.8, controlnet=net, control_image=A)
    print("img2img: control vs none %.3e" % rel_l2(i_ctl, i_plain))
    assert bool(torch.isfinite(i_ctl).all()) and rel_l2(i_ctl, i_plain) > CC.CAP


@pytest.mark.parametrize("mode", ["eager", "folded", "graph"])
def test_the_native_route_against_the_stock_sequence(gpu_device, mode, monkeypatch):
    from pww_hip import controlnet as CN
    tools, (net,) = CC.build_request_tools(gpu_device)
    monkeypatch.setenv("PWW_CONTROL", "force")
    CN.reset_stats()
    native = _run(tools, gpu_device, mode, controlnet=net, control_image=A)
    st = CN.stats()
    assert st["grouped_launches"] == st["evaluations"] > 0 and st["stock_zero_convs"] == 0 and st["declined"] == 0
    monkeypatch.setenv("PWW_CONTROL", "0")
    CN.reset_stats()
    stock = _run(tools, gpu_device, mode, controlnet=net, control_image=A)
    st = CN.stats()
    assert st["grouped_launches"] == 0 and st["stock_zero_convs"] == 9 * st["evaluations"] > 0
    d = rel_l2(native, stock)
    print("native vs PWW_CONTROL=0, %s: final-latent rel-L2 %.3e" % (mode, d))
    assert d <= CC.CAP


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_scale_zero_and_an_empty_window_are_the_uncontrolled_call_bit_for_bit(gpu_device, mode):
    tools, (net,) = CC.build_request_tools(gpu_device)
    plain = _run(tools, gpu_device, mode)
    again = _run(tools, gpu_device, mode)
    zero = _run(tools, gpu_device, mode, controlnet=net, control_image=A, controlnet_conditioning_scale=0.0)
    empty = _run(tools, gpu_device, mode, controlnet=net, control_image=A, control_guidance_start=0.5, control_guidance_end=0.5)
    on = _run(tools, gpu_device, mode, controlnet=net, control_image=A)
    print("%s: plain vs plain equal=%s, scale 0 vs plain %.3e, empty window vs plain %.3e, control vs plain %.3e"
          % (mode, torch.equal(plain, again), rel_l2(zero, plain), rel_l2(empty, plain), rel_l2(on, plain)))
    assert torch.equal(again, plain)                                    # the yardstick is repeatable
    assert torch.equal(zero, plain)
    assert torch.equal(empty, plain)
    assert rel_l2(on, plain) > 4 * CC.CAP


def test_a_window_in_graph_mode_equals_the_window_in_folded_mode(gpu_device):
    tools, (net,) = CC.build_request_tools(gpu_device)
    kw = dict(controlnet=net, control_image=A, control_guidance_start=0.0, control_guidance_end=0.5)
    plain_g, plain_f = _run(tools, gpu_device, "graph"), _run(tools, gpu_device, "folded")
    graph = _run(tools, gpu_device, "graph", **kw)
    folded = _run(tools, gpu_device, "folded", **kw)
    full = _run(tools, gpu_device, "folded", controlnet=net, control_image=A)
    print("window [0, 0.5]: graph vs folded %.3e (plain graph vs plain folded %.3e), window vs full %.3e, window vs none %.3e"
          % (rel_l2(graph, folded), rel_l2(plain_g, plain_f), rel_l2(folded, full), rel_l2(folded, plain_f)))
    assert torch.equal(graph, folded)
    assert rel_l2(folded, full) > CC.CAP and rel_l2(folded, plain_f) > CC.CAP      # the window is neither the whole schedule nor nothing


def test_graph_mode_captures_once_and_replays_another_image_and_scale(gpu_device):
    from pww_hip import controlnet as CN
    tools, (net,) = CC.build_request_tools(gpu_device)
    first = _run(tools, gpu_device, "graph", controlnet=net, control_image=A, controlnet_conditioning_scale=1.0)
    sampler = _sampler(tools, "graph")
    assert sampler._graphed.captures == 1
    CN.reset_stats()
    second = _run(tools, gpu_device, "graph", controlnet=net, control_image=B, controlnet_conditioning_scale=0.6, control_guidance_end=0.7)
    st = CN.stats()
    assert sampler._graphed.captures == 1                                # replayed: copy into the static tensors, fill the scale words
    assert st["hint_embeddings"] == 1 and st["evaluations"] == CC.STEPS == st["grouped_launches"] and st["stock_zero_convs"] == 0
    fresh_tools, (fresh_net,) = CC.build_request_tools(gpu_device)
    fresh = _run(fresh_tools, gpu_device, "graph", controlnet=fresh_net, control_image=B, controlnet_conditioning_scale=0.6, control_guidance_end=0.7)
    print("replayed vs a fresh sampler %.3e, first vs second request %.3e" % (rel_l2(second, fresh), rel_l2(first, second)))
    assert torch.equal(second, fresh)
    assert rel_l2(first, second) > CC.CAP
    plain = _run(tools, gpu_device, "graph")                             # the uncontrolled call has another signature: a capture of its own
    assert sampler._graphed.captures == 2 and bool(torch.isfinite(plain).all())


def test_stats_one_grouped_launch_per_net_and_evaluation(gpu_device):
    from pww_hip import controlnet as CN
    tools, (net,) = CC.build_request_tools(gpu_device)
    CN.reset_stats()
    _run(tools, gpu_device, "folded", controlnet=net, control_image=A)
    st = CN.stats()
    assert st["requests"] == 1 and st["hint_embeddings"] == 1 and st["evaluations"] == CC.STEPS
    assert st["grouped_launches"] == CC.STEPS and st["grouped_problems"] == 9 * CC.STEPS and st["stock_zero_convs"] == 0
    assert st["declined"] == 0 and st["decline_reasons"] == {} and st["skipped_steps"] == 0
    CN.reset_stats()
    _run(tools, gpu_device, "eager", controlnet=net, control_image=A, control_guidance_end=0.5)
    st = CN.stats()                                                      # eager: two batch-1 evaluations per step, inside the window only
    assert st["evaluations"] == 2 == st["grouped_launches"] and st["skipped_steps"] == 2 and st["hint_embeddings"] == 1 and st["stock_zero_convs"] == 0


def test_a_batch_gives_every_image_its_own_hint(gpu_device):
    tools, (net,) = CC.build_request_tools(gpu_device)
    ab = _run(tools, gpu_device, "graph", batch=[3, 4], controlnet=net, control_image=[A, B])
    ba = _run(tools, gpu_device, "graph", batch=[3, 4], controlnet=net, control_image=[B, A])
    single = _run(tools, gpu_device, "graph", seed=3, controlnet=net, control_image=A)
    d, moved = rel_l2(ab[:1], single), rel_l2(ab[:1], ba[:1])
    print("batch (A, B) image 0 vs the single call with A %.3e, vs the batch (B, A) %.3e" % (d, moved))
    assert tuple(ab.shape) == (2, 4, 16, 16) and d <= CC.CAP and moved > 4 * CC.CAP


def test_two_controlnets_run(gpu_device):
    from pww_hip import controlnet as CN
    tools, (n1, n2) = CC.build_request_tools(gpu_device, nets=2)
    CN.reset_stats()
    both = _run(tools, gpu_device, "folded", controlnet=[n1, n2], control_image=[A, B], controlnet_conditioning_scale=[1.0, 0.5])
    st = CN.stats()
    assert st["grouped_launches"] == 2 * CC.STEPS and st["hint_embeddings"] == 2 and st["stock_zero_convs"] == 0 and st["declined"] == 0
    one = _run(tools, gpu_device, "folded", controlnet=n1, control_image=A)
    off = _run(tools, gpu_device, "folded", controlnet=[n1, n2], control_image=[A, B], controlnet_conditioning_scale=[1.0, 0.0])
    print("two nets vs the first alone %.3e; the second at scale 0 vs the first alone: equal=%s" % (rel_l2(both, one), torch.equal(off, one)))
    assert bool(torch.isfinite(both).all()) and rel_l2(both, one) > CC.CAP
    assert torch.equal(off, one)                                         # the second launch at scale 0 hands the first's outputs through


def test_region_prompts_with_control_every_row_has_its_images_hint(gpu_device):
    tools, (net,) = CC.build_request_tools(gpu_device)
    colors = list(cases.RUNNER_CONTEXT)
    regions = {colors[0]: "a fluffy cat on a sofa", colors[1]: ("a golden retriever", 0.8, None)}
    kw = dict(controlnet=net, region_prompts=regions)
    ab = _run(tools, gpu_device, "graph", batch=[3, 4], control_image=[A, B], **kw)
    ba = _run(tools, gpu_device, "graph", batch=[3, 4], control_image=[B, A], **kw)
    single = _run(tools, gpu_device, "graph", seed=3, control_image=A, **kw)
    d, moved = rel_l2(ab[:1], single), rel_l2(ab[:1], ba[:1])
    print("region prompts: batch (A, B) image 0 vs the single call with A %.3e, vs the batch (B, A) %.3e" % (d, moved))
    assert d <= CC.CAP and moved > 4 * CC.CAP
    eager = _run(tools, gpu_device, "eager", seed=3, control_image=A, **kw)
    print("region prompts: eager vs graph %.3e" % rel_l2(eager, single))
    assert rel_l2(eager, single) <= CC.CAP


def test_the_untaken_combinations_raise(gpu_device):
    from pww_hip import controlnet as CN
    from pww_hip._lib import PwwHipError
    from sd_standin import build_controlnet
    tools, (net,) = CC.build_request_tools(gpu_device)
    with pytest.raises(ValueError, match="canvas_window"):
        _run(tools, gpu_device, "folded", controlnet=net, control_image=A, canvas_window=64)
    with pytest.raises(ValueError, match="same size"):
        _run(tools, gpu_device, "folded", controlnet=net, control_image=A[:64])
    with pytest.raises(ValueError, match="layout"):
        _run(tools, gpu_device, "folded", controlnet=build_controlnet(CC.REQUEST_CONFIG, device=gpu_device), control_image=A)          # fp32
    with pytest.raises(PwwHipError, match="HIP device"):
        _run(tools, gpu_device, "folded", controlnet=build_controlnet(CC.REQUEST_CONFIG, dtype=torch.float16), control_image=A)        # on the CPU
    sampler = _sampler(tools, "folded")
    request = CN.ControlRequest([net], [torch.zeros(1, 3, CC.SIDE, CC.SIDE)], [1.0])
    lat = torch.zeros(1, 4, 16, 16, device=gpu_device)
    with pytest.raises(ValueError, match="inpainting"):
        sampler.sample({}, {}, lat, [], 7.5, cases.weight_fn_runner, extra_channels=torch.zeros(1, 5, 16, 16, device=gpu_device), control=request)
