"""Per-token cross-attention maps from the fused attention path.

The reference keeps `attention_scores.softmax(dim=-1)` as an ordinary tensor inside inj_forward
(paint_with_words/paint_with_words.py:112-114), so a user who tunes `weight_function` and the region strengths can look at
where each prompt token's attention went. The fused kernels never write that tensor. While a recorder is active

    with pww_hip.record_attention_maps() as rec:
        paint_with_words(...)
    maps = rec.maps()

every cross-attention call over the prompt tokens is followed by one pww_cross_attn_probs launch (ops.attention_probs) with the same
q / k / map / coefficient inputs, which adds the head-averaged probabilities of the conditional rows into one fp32 accumulator per token
count (or per layer). Nothing here is on the hot path: the recorder is host bookkeeping, AttentionMaps is torch / PIL on finished buffers.
"""
import contextlib
import math
import threading

import torch
import torch.nn.functional as F

from . import ops
from ._lib import PwwHipError

_tls = threading.local()


def active():
    """The recorder of the calling thread's `record_attention_maps()` block, or None."""
    return getattr(_tls, "recorder", None)


@contextlib.contextmanager
def record_attention_maps(per_layer=False):
    """Record the cross-attention maps of every request issued inside the block by this thread (paint_with_words,
    paint_with_words_batch, paint_with_words_inpaint, the pipeline classes, PwWSampler.sample). per_layer: one accumulator per
    cross-attention layer instead of one per token count. Not nestable; single-device only."""
    if active() is not None:
        raise PwwHipError("record_attention_maps() is already active on this thread (it does not nest)")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise PwwHipError("record_attention_maps() does not cover pww_hip.dist: the process group has world size %d > 1"
                          % torch.distributed.get_world_size())
    rec = AttentionRecorder(per_layer=per_layer)
    _tls.recorder = rec
    try:
        yield rec
    finally:
        _tls.recorder = None


class _ChunkedPrompt(list):
    """The framed ids of a prompt encoded in several chunks (a list, like a one-chunk prompt's entry) + its unframed content ids."""

    def __init__(self, token_ids, content_ids, per):
        super().__init__(token_ids)
        self.content, self.per = list(content_ids), per


class AttentionRecorder:
    """Host side of the recording mode: owns the accumulators, counts the contributions per accumulator (layers x UNet evaluations), and
    is what attention._attention finds under the ATTN_RECORDER key of a conditional context dict."""

    def __init__(self, per_layer=False):
        self.per_layer = bool(per_layer)
        self.images = None        # recorded images per request (fixed by the first request / launch)
        self.latent_hw = None
        self.row = 0              # eager mode: the image the next batch-1 UNet call belongs to
        self.muted = False        # hipGraph warm-up pass: accumulators are allocated, nothing is launched or counted
        self.counts = {}          # accumulator key -> contributions per image
        self.tokenizer = None
        self.prompts = []         # token id lists, one per conditioned prompt of the request(s)
        self._live = {}           # key -> fp32 [images, N, M] accumulator the launches add into
        self._done = {}           # key -> sum of finished hipGraph-mode requests (their accumulators belong to the sampler)
        self._meta = {}           # key -> (N, M, order of first appearance)
        self._trace = None        # capture pass: key -> launches per UNet evaluation
        self._static_meta = None  # hipGraph mode: the sampler's record of its static accumulators (a later recorder only replays: it never sees the calls)

    # -- what the sampler calls -------------------------------------------------------------------
    def begin_request(self, images, latent_hw=None, static=None):
        """A request of `images` images starts. static: the sampler's {"bufs": key -> accumulator, "meta": key -> (N, M, order)} of static
        accumulators (hipGraph mode: captured launches hold their addresses); they are zeroed here, before the first replay."""
        if self.images is not None and self.images != images:
            raise PwwHipError("one recorder serves requests of one batch size (%d images so far, now %d)" % (self.images, images))
        self.images, self.row = int(images), 0
        if latent_hw is not None:
            self.latent_hw = (int(latent_hw[0]), int(latent_hw[1]))
        if static is not None:
            self._live, self._static_meta = static["bufs"], static["meta"]
            self._meta.update(static["meta"])
            for buf in self._live.values():
                buf.zero_()

    def end_request(self, static=False):
        self.row = 0
        if static:                # the static accumulators serve the next request: keep this one's sums
            for key, buf in self._live.items():
                self._done[key] = buf.clone() if key not in self._done else self._done[key] + buf
            self._live, self._static_meta = {}, None

    def begin_trace(self):
        self._trace = {}

    def end_trace(self):
        trace, self._trace = self._trace, None
        return trace

    def replayed(self, trace):
        for key, n in trace.items():
            self.counts[key] = self.counts.get(key, 0) + n

    def note_prompt(self, tokenizer, token_ids, content_ids=None):
        """token_ids: the prompt's key columns (77 k framed ids). content_ids: with a prompt encoded in several chunks, its unframed ids --
        phrases are matched on them and mapped to columns like the weight maps' (conditioning.framed_column)."""
        self.tokenizer = tokenizer
        self.prompts.append(list(token_ids) if content_ids is None else _ChunkedPrompt(token_ids, content_ids, tokenizer.model_max_length - 2))

    # -- what the attention plug calls ------------------------------------------------------------
    def target(self, attn, B, N, M, cond_rows, device):
        """-> (accumulator rows to add into, images) for one cross-attention call, or None while muted. cond_rows: the first so many of the
        B rows are the conditional ones of a CFG-folded batch (0: all of them)."""
        images = int(cond_rows) if cond_rows else int(B)
        if self.images is None:
            self.images = images
        if self.row + images > self.images:
            raise PwwHipError("attention call of %d recorded images does not fit the recorder's %d" % (images, self.images))
        key = ("layer", id(attn)) if self.per_layer else N
        buf = self._live.get(key)
        if buf is None or tuple(buf.shape) != (self.images, N, M) or buf.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise PwwHipError("attention-map accumulators must exist before hipGraph capture")
            buf = self._live[key] = ops.probs_buffer(self.images, N, M, device)
        if key not in self._meta:
            self._meta[key] = (N, M, len(self._meta))
        if self._static_meta is not None:
            self._static_meta.setdefault(key, self._meta[key])
        if self.muted:
            return None
        if self.row == 0:
            tally = self._trace if self._trace is not None else self.counts
            tally[key] = tally.get(key, 0) + 1
        return buf[self.row:self.row + images], images

    # -- results ----------------------------------------------------------------------------------
    def maps(self):
        entries = []
        for key, (N, M, order) in sorted(self._meta.items(), key=lambda kv: kv[1][2]):
            total = None
            for t in (self._done.get(key), self._live.get(key)):
                if t is not None:
                    total = t.clone() if total is None else total + t
            if total is not None and self.counts.get(key, 0) > 0:
                entries.append((N, total, self.counts[key]))
        return AttentionMaps(entries, latent_hw=self.latent_hw, tokenizer=self.tokenizer, prompts=self.prompts)


def _grid_of(N, latent_hw):
    """(h, w) of a layer with N tokens: the latent grid halved (rounding up, like the UNet's stride-2 convolutions) until it has N cells;
    without a latent size, a square."""
    if latent_hw is not None:
        h, w = latent_hw
        for _ in range(8):
            if h * w == N:
                return h, w
            h, w = (h + 1) // 2, (w + 1) // 2
    r = math.isqrt(N)
    if r * r == N:
        return r, r
    raise PwwHipError("cannot tell the grid of a layer with %d tokens (latent size %s)" % (N, latent_hw))


class AttentionMaps:
    """Finished attention maps. entries: [(N, fp32 [images, N, M] SUM of contributions, number of contributions)] -- one per token count,
    or one per layer (`layers`). Values are means over layers, UNet evaluations and heads of the softmax probabilities."""

    def __init__(self, entries, latent_hw=None, tokenizer=None, prompts=()):
        if not entries:
            raise PwwHipError("no cross-attention call was recorded")
        self._entries = [(int(N), t, int(c)) for N, t, c in entries]
        self._latent_hw = latent_hw
        self.tokenizer, self.prompts = tokenizer, list(prompts)
        self.resolutions = {N: _grid_of(N, latent_hw) for N, _, _ in self._entries}
        self.counts = {}
        for N, _, c in self._entries:
            self.counts[N] = self.counts.get(N, 0) + c

    @property
    def layers(self):
        """One AttentionMaps per recorded accumulator (per layer with record_attention_maps(per_layer=True)), in call order."""
        return [AttentionMaps([e], self._latent_hw, self.tokenizer, self.prompts) for e in self._entries]

    @property
    def count(self):
        return sum(self.counts.values())

    def raw(self, N):
        """[images, h, w, M]: mean over the layers of N tokens and the UNet evaluations."""
        parts = [t for n, t, _ in self._entries if n == N]
        if not parts:
            raise KeyError(N)
        total = parts[0] if len(parts) == 1 else torch.stack(parts).sum(0)
        h, w = self.resolutions[N]
        return (total / self.counts[N]).reshape(total.shape[0], h, w, total.shape[2])

    def tokens(self, size=None):
        """[images, M, H, W]: every resolution resized bilinearly to `size` (default: the largest recorded), averaged with the
        resolutions' contribution counts as weights."""
        if size is None:
            size = max(self.resolutions.values(), key=lambda hw: hw[0] * hw[1])
        size = (int(size[0]), int(size[1]))
        acc = None
        for N in self.resolutions:
            m = self.raw(N).permute(0, 3, 1, 2)
            if tuple(m.shape[-2:]) != size:
                m = F.interpolate(m, size=size, mode="bilinear", align_corners=False)
            m = m * float(self.counts[N])
            acc = m if acc is None else acc + m
        return acc / float(self.count)

    def columns(self, text, image=0):
        """Prompt positions of `text` in image `image`'s prompt: the tokenizer span search conditioning._parse_regions /
        _column_lists use for the color_context phrases."""
        if self.tokenizer is None or not self.prompts:
            raise PwwHipError("no prompt was recorded with these maps (phrase lookup needs the request's tokenizer and prompt)")
        ids = list(self.tokenizer(text, max_length=self.tokenizer.model_max_length, truncation=True)["input_ids"][1:-1])
        toks = self.prompts[image if len(self.prompts) > 1 else 0]
        L = len(ids)
        if isinstance(toks, _ChunkedPrompt):
            from .conditioning import framed_column
            inner = toks.content
            cols = sorted({framed_column(c, toks.per) for i in range(len(inner)) if L and inner[i:i + L] == ids for c in range(i, min(i + L, len(inner)))})
        else:
            cols = sorted({c for i in range(len(toks)) if L and toks[i:i + L] == ids for c in range(i, i + L)})
        if not cols:
            raise PwwHipError("phrase %r does not occur in the prompt" % (text,))
        return cols

    def phrase(self, text, size=None):
        """[images, H, W]: mean of tokens() over the prompt positions of `text`."""
        t = self.tokens(size)
        return torch.stack([t[i, self.columns(text, i)].mean(0) for i in range(t.shape[0])])

    def to_pil(self, text, size=None):
        """One 8-bit greyscale PIL image per recorded image: phrase(text), min-max normalised."""
        from PIL import Image
        out = []
        for m in self.phrase(text, size).float().cpu():
            lo, hi = float(m.min()), float(m.max())
            m = (m - lo) / (hi - lo) if hi > lo else torch.zeros_like(m)
            out.append(Image.fromarray((m * 255.0).round().clamp(0, 255).to(torch.uint8).numpy(), mode="L"))
        return out
