"""The grouped ControlNet-residual launch (libpww_hip_control.so through ops.control_residuals) against an fp64 reference, fp16 and bf16.

The bar per element is derived, not tuned (tests/control_cases.py::bar): u |ref| + K 2^-23 |s| (sum_k |h||w| + |b|), u = 2^-8 (bf16) or 2^-11
(fp16) -- one rounding of the result plus fp32 accumulation. No case may be skipped or declined: each asserts through
pww_hip.controlnet.stats() that the grouped kernel ran."""
import pytest
import torch
import torch.nn as nn

import control_cases as CC

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _nhwc(t, device):
    return t.to(device).contiguous(memory_format=torch.channels_last) if t.shape[2] * t.shape[3] > 1 and t.shape[1] > 1 else _rows_nhwc(t, device)


def _rows_nhwc(t, device):
    """A [B, C, H, W] tensor whose memory is [B H W][C] whatever sizes are 1 (the allocator's channels_last strides are ambiguous there)."""
    B, C, H, W = t.shape
    return t.to(device).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _conv(p, device):
    conv = nn.Conv2d(p["K"], p["N"], 1).to(device=device, dtype=p["w"].dtype).requires_grad_(False)
    conv.weight.copy_(p["w"])
    conv.bias.copy_(p["b"])
    return conv


def _word(s, device):
    return torch.tensor([float(s)], dtype=torch.float32, device=device)


def _launch(problems, s, device, with_skip=True, skips=None, outs=None, word=None):
    """ops.control_residuals on the problems, with the launch counted."""
    from pww_hip import ops, controlnet
    hs = [_nhwc(p["h"], device) for p in problems]
    convs = [_conv(p, device) for p in problems]
    if with_skip and skips is None:
        skips = [_nhwc(p["skip"], device) for p in problems]
    word = _word(s, device) if word is None else word
    assert ops.control_takes(hs, convs, word, skips, outs)
    before = controlnet.stats()
    got = ops.control_residuals(hs, convs, word, skips=skips, outs=outs)
    after = controlnet.stats()
    assert after["grouped_launches"] == before["grouped_launches"] + 1 and after["grouped_problems"] == before["grouped_problems"] + len(problems)
    assert after["declined"] == before["declined"]
    return got, (hs, convs, skips, word)


def _check(problems, got, s, dtype, with_skip=True):
    worst = 0.0
    for p, out in zip(problems, got):
        assert out.dtype == dtype and tuple(out.shape) == tuple(p["skip"].shape)
        ref, mag = CC.reference(p, s, with_skip)
        err, lim = (out.double().cpu() - ref).abs(), CC.bar(p, s, ref, mag, dtype)
        ratio = float((err / lim.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= lim).all()), "M %d K %d N %d: error / bar = %.3f" % (p["M"], p["K"], p["N"], ratio)
    return worst


@DTYPES
def test_one_row_one_tile(gpu_device, dtype):
    problems = [CC.problem(1, 1, 64, 64, dtype)]
    got, _ = _launch(problems, 0.75, gpu_device)
    print("M 1 K 64 N 64 %s: worst error / bar %.3f" % (dtype, _check(problems, got, 0.75, dtype)))


@DTYPES
def test_m_tail_and_three_column_tiles(gpu_device, dtype):
    problems = [CC.problem(2, 129, 64, 192, dtype)]
    got, _ = _launch(problems, 1.25, gpu_device)
    print("M 129 K 64 N 192 %s: worst error / bar %.3f" % (dtype, _check(problems, got, 1.25, dtype)))


@DTYPES
def test_thirteen_problems_each_with_its_own_weights(gpu_device, dtype):
    problems = [CC.problem(10 + i, M, K, N, dtype, B=2) for i, (M, K, N) in enumerate(CC.THIRTEEN)]
    got, _ = _launch(problems, 0.5, gpu_device)
    print("thirteen problems %s: worst error / bar %.3f" % (dtype, _check(problems, got, 0.5, dtype)))
    # a wrong (problem, tile) mapping would put another problem's product here: far outside the bar
    a, b = problems[0], problems[10]
    assert (a["M"], a["K"]) != (b["M"], b["K"]) or not torch.equal(a["w"], b["w"])


@DTYPES
def test_skip_rows_are_slices_of_a_wider_tensor(gpu_device, dtype):
    """channels_last views: the skip is a channel slice of a wider channels_last tensor (row pitch 192 + 64), the hidden state too, and the
    output goes into a slice of a third."""
    p = CC.problem(3, 2 * 5 * 7, 128, 192, dtype, hw=(5, 7), B=2)
    wide_skip = torch.zeros(2, 256, 5, 7, dtype=dtype, device=gpu_device).contiguous(memory_format=torch.channels_last)
    wide_skip[:, 64:] = p["skip"].to(gpu_device)
    wide_h = torch.zeros(2, 192, 5, 7, dtype=dtype, device=gpu_device).contiguous(memory_format=torch.channels_last)
    wide_h[:, :128] = p["h"].to(gpu_device)
    wide_out = torch.full((2, 320, 5, 7), 3.0, dtype=dtype, device=gpu_device).contiguous(memory_format=torch.channels_last)
    from pww_hip import ops, controlnet
    word, conv = _word(0.6, gpu_device), _conv(p, gpu_device)
    before = controlnet.stats()["grouped_launches"]
    got = ops.control_residuals([wide_h[:, :128]], [conv], word, skips=[wide_skip[:, 64:]], outs=[wide_out[:, 64:256]])
    assert controlnet.stats()["grouped_launches"] == before + 1
    assert got[0].data_ptr() == wide_out[:, 64:256].data_ptr()                              # nothing is copied
    _check([p], got, 0.6, dtype)
    assert bool((wide_out[:, :64] == 3.0).all()) and bool((wide_out[:, 256:] == 3.0).all())      # the neighbours of the slice are untouched
    assert torch.equal(wide_skip[:, 64:].cpu(), p["skip"])                                   # read only


@DTYPES
def test_out_may_alias_its_skip(gpu_device, dtype):
    problems = [CC.problem(4, 129, 128, 64, dtype), CC.problem(5, 8, 64, 128, dtype)]
    skips = [_nhwc(p["skip"], gpu_device) for p in problems]
    got, _ = _launch(problems, 0.9, gpu_device, skips=skips, outs=skips)
    assert all(g.data_ptr() == s.data_ptr() for g, s in zip(got, skips))
    _check(problems, got, 0.9, dtype)


@DTYPES
def test_without_a_skip(gpu_device, dtype):
    problems = [CC.problem(6, 130, 192, 64, dtype), CC.problem(7, 3, 64, 64, dtype)]
    got, _ = _launch(problems, -1.5, gpu_device, with_skip=False)
    _check(problems, got, -1.5, dtype, with_skip=False)


@DTYPES
def test_scale_zero_returns_the_skip_bit_for_bit(gpu_device, dtype):
    problems = [CC.problem(8, 129, 64, 128, dtype), CC.problem(9, 2, 128, 64, dtype)]
    problems[0]["skip"][0, 0, 0, :4] = torch.tensor([-0.0, 0.0, float("inf"), -1.0]).to(dtype)      # a signed zero and an infinity pass through
    problems[1]["h"][0, 0, 0, 0] = float("inf")                                                    # ... and so does a skip beside a non-finite h
    got, _ = _launch(problems, 0.0, gpu_device)
    for p, out in zip(problems, got):
        assert torch.equal(out.cpu().view(torch.int16), p["skip"].view(torch.int16))


@DTYPES
def test_the_same_launch_follows_the_scale_word(gpu_device, dtype):
    """The scale is read from the device word when the launch runs: the launch captured into a hipGraph and replayed after the word is
    rewritten gives the new scale's result; two replays with one word are bit-equal."""
    from pww_hip import ops, controlnet
    problems = [CC.problem(20 + i, M, K, N, dtype) for i, (M, K, N) in enumerate([(129, 64, 64), (8, 128, 128)])]
    hs = [_nhwc(p["h"], gpu_device) for p in problems]
    convs = [_conv(p, gpu_device) for p in problems]
    skips = [_nhwc(p["skip"], gpu_device) for p in problems]
    word = _word(0.5, gpu_device)
    before = controlnet.stats()["grouped_launches"]
    outs = ops.control_residuals(hs, convs, word, skips=skips)          # (warm-up in front of the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.control_residuals(hs, convs, word, skips=skips, outs=outs)
    assert controlnet.stats()["grouped_launches"] == before + 2
    graph.replay()
    _check(problems, outs, 0.5, dtype)
    first = [o.clone() for o in outs]
    graph.replay()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))          # bitwise repeatable
    word.fill_(-2.0)
    graph.replay()
    _check(problems, outs, -2.0, dtype)
    word.zero_()
    graph.replay()
    assert all(torch.equal(o.view(torch.int16), s.view(torch.int16)) for o, s in zip(outs, skips))


@DTYPES
def test_two_launches_are_bit_equal(gpu_device, dtype):
    problems = [CC.problem(30 + i, M, K, N, dtype, B=2) for i, (M, K, N) in enumerate(CC.THIRTEEN)]
    a, _ = _launch(problems, 0.7, gpu_device)
    b, _ = _launch(problems, 0.7, gpu_device)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_what_the_library_would_refuse_is_declined(gpu_device):
    from pww_hip import ops
    from pww_hip._lib import PwwHipError
    p = CC.problem(40, 8, 64, 64, torch.float16)
    h, conv, skip, word = _nhwc(p["h"], gpu_device), _conv(p, gpu_device), _nhwc(p["skip"], gpu_device), _word(1.0, gpu_device)
    assert ops.control_takes([h], [conv], word, [skip])
    odd = nn.Conv2d(64, 96, 1).to(device=gpu_device, dtype=torch.float16)
    nchw = p["h"].to(gpu_device).contiguous()
    for bad in (([h] * 17, [conv] * 17, word, None), ([h], [odd], word, None), ([nchw.expand(1, 64, 1, 8)[:, :, :, ::2]], [conv], word, None),
                ([h], [conv], word.cpu(), None), ([h], [conv], word.half(), None), ([h.float()], [conv], word, None), ([h], [conv], word, [skip[:, :32]]),
                ([h], [nn.Conv2d(64, 64, 3, padding=1).to(device=gpu_device, dtype=torch.float16)], word, None)):
        assert not ops.control_takes(*bad)
        with pytest.raises(PwwHipError, match="control_residuals"):
            ops.control_residuals(bad[0], bad[1], bad[2], skips=bad[3])
