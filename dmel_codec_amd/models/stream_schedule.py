"""Frontier / window arithmetic of the streaming encoder (models/codec_lit_modules.py: StreamingEncoder).  Pure integer code -- no
torch, no GPU: which mel frames, which WaveNet level frontiers and which tokens become final once `k` samples of a stream have
arrived, and how the last step (the stream's end is known) differs.

The stack is non-causal, so a token needs right context before its id can equal the one `encode()` gives it on the finished clip:

    token j   <- encoder features  [F j - quant_left, F j + quant_right]          (quantiser: strided convs + ConvNeXt blocks)
    feature t <- mel frames        [t - sum(dilations), t + sum(dilations)]       (WaveNet: one k = 3 dilated conv per block)
    frame t   <- samples           [t hop - pad, t hop - pad + n_fft)             (STFT, reflected at the signal's own ends only)

so token j is final as soon as `token_ready_samples(j)` samples have arrived -- or the stream ends.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Mapping, Optional, Sequence, Tuple


def quantizer_context(downsample_factor: Sequence[int], dw_kernel: int = 7) -> Tuple[int, int]:
    """(left, right): token j of DownsampleFiniteScalarQuantize.encode depends on the input frames [F j - left, F j + right], F the
    product of the factors.  Walked back through the layers: each stage is Conv1d(kernel = stride = f) followed by a ConvNeXt block whose
    only mixing over time is a depthwise conv of `dw_kernel` taps (LayerNorm, the pointwise convs and the FSQ act per position).
    Factors (2, 2), k = 7: [0, 0] -> [-3, 3] -> [-6, 7] -> [-9, 10] -> [-18, 21]."""
    lo = hi = 0
    half = (dw_kernel - 1) // 2
    for f in reversed(list(downsample_factor)):
        lo, hi = lo - half, hi + half            # ConvNeXt block at this rate
        lo, hi = lo * f, hi * f + f - 1          # Conv1d(kernel_size = f, stride = f)
    return -lo, hi


@dataclass(frozen=True)
class EncodeGeometry:
    hop: int
    n_fft: int
    dilations: Tuple[int, ...]
    downsample_factor: Tuple[int, ...] = (2, 2)
    dw_kernel: int = 7

    @property
    def pad(self) -> int:
        return (self.n_fft - self.hop) // 2

    @property
    def factor(self) -> int:
        f = 1
        for v in self.downsample_factor:
            f *= v
        return f

    @property
    def quant_context(self) -> Tuple[int, int]:
        return quantizer_context(self.downsample_factor, self.dw_kernel)

    @property
    def encoder_context(self) -> int:
        return sum(self.dilations)

    def frames_ready(self, k: int) -> int:
        """frames whose every sample is among the first k of an unfinished stream (no right reflection can be involved)"""
        need = self.n_fft - self.pad
        return 0 if k < need else (k - need) // self.hop + 1

    def total_frames(self, length: int) -> int:
        """frames of a finished clip of `length` samples: 1 + (length + 2 pad - n_fft) // hop = length // hop"""
        padded = length + 2 * self.pad
        return 0 if padded < self.n_fft else 1 + (padded - self.n_fft) // self.hop

    def token_ready_samples(self, j: int, total: Optional[int] = None) -> int:
        """number of samples after which token j is final: its right context complete, or the stream (of `total` samples) over"""
        t = self.factor * j + self.quant_context[1] + self.encoder_context          # last mel frame token j depends on
        k = t * self.hop - self.pad + self.n_fft
        return k if total is None else min(k, total)

    @property
    def lookahead_samples(self) -> int:
        """samples behind the first sample of token j (sample F j hop) that must have arrived before token j is final"""
        return self.token_ready_samples(0)


@dataclass(frozen=True)
class EncodeStep:
    samples: int                      # samples received so far
    final: bool
    frames: Tuple[int, int]           # mel frames [a, b) to compute now
    prev: Tuple[int, ...]             # WaveNet level frontiers before / after the step (absolute frames, levels 0 .. L)
    next: Tuple[int, ...]
    tokens: Tuple[int, int]           # tokens [a, b) that become final now
    quant_window: Tuple[int, int]     # feature frames [lo, hi) the quantiser runs on for them (lo a multiple of the factor)
    total_length: int                 # -1 until the stream's end is known


class EncodeSchedule:
    """The streaming encoder's counters.  step(n, final) accounts for n more samples and says what to compute."""

    def __init__(self, geo: EncodeGeometry):
        self.geo = geo
        self.samples = 0
        self.frames = 0
        self.levels: List[int] = [0] * (len(geo.dilations) + 1)
        self.tokens = 0
        self.finished = False

    def step(self, n: int, final: bool = False) -> EncodeStep:
        if self.finished:
            raise RuntimeError("stream already finished")
        if n < 0:
            raise ValueError("negative sample count")
        g = self.geo
        self.samples += n
        f_new = g.total_frames(self.samples) if final else g.frames_ready(self.samples)
        f_new = max(f_new, self.frames)
        nxt = [f_new]
        for l, d in enumerate(g.dilations):
            # mid-stream a level stays `dilation` columns behind its input; at the end the zero padding is the real one
            nxt.append(f_new if final else max(self.levels[l + 1], nxt[-1] - d))
        ready = nxt[-1]                                   # encoder features [0, ready) exist
        left, right = g.quant_context
        F = g.factor
        if final:
            j_new = f_new
            for f in g.downsample_factor:                 # every strided conv floors: (T // 2) // 2
                j_new //= f
        else:
            j_new = max(self.tokens, (ready - right - 1) // F + 1 if ready > right else 0)
        lo_tok = max(0, self.tokens - (left + F - 1) // F)
        st = EncodeStep(samples=self.samples, final=final, frames=(self.frames, f_new), prev=tuple(self.levels), next=tuple(nxt),
                        tokens=(self.tokens, j_new), quant_window=(lo_tok * F, ready),
                        total_length=self.samples if final else -1)
        self.frames, self.levels, self.tokens = f_new, nxt, j_new
        self.finished = final
        return st

    def state(self) -> dict:
        """the counters as plain Python values -- nothing derived from the geometry: what a snapshot of a session carries"""
        return dict(samples=self.samples, frames=self.frames, levels=list(self.levels), tokens=self.tokens, finished=self.finished)

    @classmethod
    def from_state(cls, geo: EncodeGeometry, state: Mapping) -> "EncodeSchedule":
        """the schedule that returns, for every later step(n, final), the step the one state() was taken from returns"""
        sc = cls(geo)
        sc.levels = _state_levels(state, len(geo.dilations) + 1)
        sc.samples, sc.frames, sc.tokens, sc.finished = int(state["samples"]), int(state["frames"]), int(state["tokens"]), bool(state["finished"])
        return sc


def _state_levels(state: Mapping, depth: int) -> List[int]:
    levels = [int(v) for v in state["levels"]]
    if len(levels) != depth:
        raise ValueError(f"a state of {len(levels)} level frontiers for a schedule of {depth}: the depth of the WaveNet differs")
    return levels


def encode_need_from(geo: EncodeGeometry, last_level: int, tokens: int) -> int:
    """The oldest column an encode slot still reads when a step starts from the frontier `last_level` of the last WaveNet level and
    `tokens` released tokens: the next block window reaches max(dilations) behind the last level, the quantiser's window starts its
    left context in front of the next token (EncodeStep.quant_window[0])."""
    left, _ = geo.quant_context
    F = geo.factor
    return max(0, min(last_level - max(geo.dilations), max(0, tokens - (left + F - 1) // F) * F))


def encode_live_window(sched: EncodeSchedule) -> Tuple[int, int]:
    """[lo, hi) in absolute frames: the columns of an encode slot a later step reads -- exactly what a re-base in front of the next push
    would keep (EncodeSessions._rebase) -- up to the newest mel frame."""
    lo = encode_need_from(sched.geo, sched.levels[-1], sched.tokens)
    return lo, max(lo, sched.frames)


def session_rows(slots: int, steps: Mapping[int, EncodeStep], origins: Sequence[int]) -> Tuple[List[int], List[int], List[int]]:
    """A pool of independent streams (EncodeSessions) holds one EncodeSchedule per slot; one step of the pool hands the encoder one
    (prev, next) row per slot (dmel_wavenet_stream_step_items).  steps: slot -> this step's EncodeStep of every slot that takes part;
    origins[slot]: the absolute frame in column 0 of that slot's buffers.  Returns (prev, next, origin): prev / next are `slots` rows of
    L + 1 frontiers, flattened row-major and relative to the slot's own origin; origin has one entry per slot.  A slot without a step is
    idle: a row of zeros (next == prev on every level), origin 0."""
    if not steps:
        raise ValueError("no step to make rows of")
    width = len(next(iter(steps.values())).prev)
    prev, nxt, org = [0] * (slots * width), [0] * (slots * width), [0] * slots
    for slot, st in steps.items():
        if not 0 <= slot < slots:
            raise ValueError(f"slot {slot} out of range")
        if len(st.prev) != width or len(st.next) != width:
            raise ValueError("steps of different depth")
        o = origins[slot]
        if o < 0 or o > min(st.prev):
            raise ValueError(f"slot {slot}: origin {o} is behind a frontier that is still in use")
        prev[slot * width:(slot + 1) * width] = [p - o for p in st.prev]
        nxt[slot * width:(slot + 1) * width] = [p - o for p in st.next]
        org[slot] = o
    return prev, nxt, org


# ---------------------------------------------------------------------------------------------------- the decode side
@dataclass(frozen=True)
class DecodeGeometry:
    """What the frontier arithmetic of an incremental decode depends on: mel frames per token, the decoder WaveNet's dilations, the
    vocoder's context in frames on each side (0: mel only) and the quantiser's context in tokens on each side."""
    factor: int
    dilations: Tuple[int, ...]
    voc_halo: int = 0
    quant_halo_tokens: int = 4

    @property
    def decoder_context(self) -> int:
        return sum(self.dilations)

    @property
    def max_dilation(self) -> int:
        return max(self.dilations) if self.dilations else 1

    @property
    def hold_frames(self) -> int:
        """frames between the oldest column a later step still reads and the newest frame received, at most, in front of a push: the
        quantiser holds back H tokens, the last level runs sum(dilations) behind the condition, and behind the last level the next
        block window reaches max(dilations) back and the vocoder window 2 voc_halo (emitted is voc_halo behind, its window another)"""
        return self.quant_halo_tokens * self.factor + self.decoder_context + max(self.max_dilation, 2 * self.voc_halo)


@dataclass(frozen=True)
class DecodeStep:
    tokens: int                       # tokens received so far
    final: bool
    need_from: int                    # oldest column this and every later step reads: min(prev[L] - maxdil, emitted - voc_halo), >= 0
    upto: int                         # tokens * factor: the buffers must hold the absolute frames [need_from, upto)
    tok_window: Tuple[int, int]       # tokens [lo, hi) the quantiser decodes now (lo == hi: nothing)
    tok_keep_from: int                # oldest token a later window reads: the carried token tail starts here
    z: Tuple[int, int]                # condition / level-0 frames [a, b) written now, cropped from the window's output
    prev: Tuple[int, ...]             # decoder level frontiers before / after the WaveNet step (prev == next: no step)
    next: Tuple[int, ...]
    emit: Tuple[int, int]             # mel frames [a, b) handed out now
    voc_window: Tuple[int, int]       # mel frames [lo, hi) the vocoder runs on for them (lo == hi: nothing to vocode)


class DecodeSchedule:
    """The counters StreamingDecoder._push_eager keeps inline (models/codec_lit_modules.py), as a pure class: step(n, final) accounts for n
    more tokens and says what to compute.  Time is in mel frames, absolute.

        condition   z_valid -> all frames if final, else (tokens - H) * factor: the quantiser's last H tokens wait for right context
        level l     next[l] = max(prev[l], next[l - 1] - dilation[l - 1]); the total on the final step (the zero padding is real then)
        emitted     -> prev[L] - voc_halo (prev[L] if final or mel only)

    As in StreamingDecoder the WaveNet step is skipped -- and the frontiers stay where they are -- while the last level cannot advance."""

    def __init__(self, geo: DecodeGeometry):
        self.geo = geo
        self.tokens = 0
        self.z_valid = 0
        self.levels: List[int] = [0] * (len(geo.dilations) + 1)
        self.emitted = 0
        self.tok_origin = 0
        self.finished = False

    @property
    def need_from(self) -> int:
        g = self.geo
        return max(0, min(self.levels[-1] - g.max_dilation, self.emitted - g.voc_halo))

    def step(self, n: int, final: bool = False) -> DecodeStep:
        if self.finished:
            raise RuntimeError("stream already finished")
        if n < 0:
            raise ValueError("negative token count")
        g = self.geo
        f, H = g.factor, g.quant_halo_tokens
        need_from = self.need_from
        self.tokens += n
        total = self.tokens * f
        z_new = total if final else max(self.z_valid, (self.tokens - H) * f)
        tok_window = (0, 0)
        z = (self.z_valid, self.z_valid)
        if z_new > self.z_valid:
            tok_window = (max(0, self.z_valid // f - H), self.tokens)
            z = (self.z_valid, z_new)
            self.z_valid = z_new
            self.tok_origin = max(self.tok_origin, self.z_valid // f - H)
        nxt = [self.z_valid]
        for l, d in enumerate(g.dilations):
            nxt.append(self.z_valid if final else max(self.levels[l + 1], nxt[-1] - d))
        prev = tuple(self.levels)
        if final or nxt[-1] > self.levels[-1]:
            self.levels = nxt
        ready = self.levels[-1]
        e_new = ready if (final or g.voc_halo == 0) else max(self.emitted, ready - g.voc_halo)
        voc = (0, 0)
        if g.voc_halo and e_new > self.emitted:
            voc = (max(0, self.emitted - g.voc_halo), min(ready, e_new + g.voc_halo))
        st = DecodeStep(tokens=self.tokens, final=final, need_from=need_from, upto=total, tok_window=tok_window,
                        tok_keep_from=self.tok_origin, z=z, prev=prev, next=tuple(self.levels), emit=(self.emitted, e_new), voc_window=voc)
        self.emitted = e_new
        self.finished = final
        return st

    def state(self) -> dict:
        """the counters as plain Python values -- nothing derived from the geometry: what a snapshot of a session carries"""
        return dict(tokens=self.tokens, z_valid=self.z_valid, levels=list(self.levels), emitted=self.emitted, tok_origin=self.tok_origin,
                    finished=self.finished)

    @classmethod
    def from_state(cls, geo: DecodeGeometry, state: Mapping) -> "DecodeSchedule":
        """the schedule that returns, for every later step(n, final), the step the one state() was taken from returns"""
        sc = cls(geo)
        sc.levels = _state_levels(state, len(geo.dilations) + 1)
        sc.tokens, sc.z_valid, sc.emitted = int(state["tokens"]), int(state["z_valid"]), int(state["emitted"])
        sc.tok_origin, sc.finished = int(state["tok_origin"]), bool(state["finished"])
        return sc


def decode_live_window(sched) -> Tuple[int, int]:
    """[lo, hi) in absolute frames: the columns of a decode slot a later step reads -- from the schedule's need_from, which is what a
    re-base in front of the next push would keep (decode_rebase; an EarlyDecodeSchedule with a fade keeps one frame more), to the
    condition frontier, behind which nothing has been written.  sched: a DecodeSchedule or an EarlyDecodeSchedule."""
    z_valid = sched.exact.z_valid if isinstance(sched, EarlyDecodeSchedule) else sched.z_valid
    lo = sched.need_from
    return lo, max(lo, z_valid)


def decode_capacity(geo: DecodeGeometry, max_push_tokens: int, extra_hold: int = 0) -> int:
    """Columns of a decode slot's state buffers.  In front of a push a slot holds at most geo.hold_frames columns that are still read
    (+ extra_hold: the one frame more a cross-fading session keeps, EarlyDecodeSchedule(fade_frames=1)); the push adds
    max_push_tokens * factor.  Four pushes of room instead of one, rounded up to 32, so that a slot that pushes the maximum every time
    is re-based (decode_rebase) once in four pushes and one that pushes less, less often."""
    if max_push_tokens <= 0:
        raise ValueError("max_push_tokens must be positive")
    return (geo.hold_frames + extra_hold + 4 * max_push_tokens * geo.factor + 31) // 32 * 32


def decode_rebase(origin: int, st: DecodeStep, cap: int) -> int:
    """The absolute frame column 0 of a slot's buffers holds after making room for step `st`: unchanged while [origin, st.upto) fits
    `cap` columns, else the oldest column still needed."""
    if st.upto - origin <= cap:
        return origin
    if st.upto - st.need_from > cap:
        raise RuntimeError(f"{st.upto - st.need_from} columns do not fit the capacity {cap}: a push beyond max_push_tokens")
    return st.need_from


def decode_session_rows(slots: int, steps: Mapping[int, DecodeStep], origins: Sequence[int]) -> Tuple[List[int], List[int], List[int]]:
    """session_rows for decode steps: one (prev, next) row per slot, relative to the slot's own origin; a slot without a step, or whose
    step runs no WaveNet step, is idle (a row of zeros, origin 0)."""
    live = {s: st for s, st in steps.items() if st.next != st.prev}
    if not live:
        raise ValueError("no step to make rows of")
    return session_rows(slots, live, origins)


@dataclass(frozen=True)
class EarlyDecodeStep:
    """One step of a decode session that emits with bounded look-ahead: the committed DecodeStep, untouched, and what is computed on a
    fork of the committed state (the shadow row) to hand out frames whose right context has not arrived.  Frames are absolute."""
    step: DecodeStep                  # what the exact schedule does with this push: the committed row runs it as it always did
    emit: Tuple[int, int]             # mel frames [a, b) handed out now; b may lie ahead of step.next[-1]
    shadow: bool                      # the emitted frames come from the shadow row (else from the committed one, and nothing is forked)
    prev: Tuple[int, ...]             # the shadow row: from the committed frontiers in front of this step ...
    next: Tuple[int, ...]             # ... to `upto` on every level, a final-style row (prev == next: no shadow step)
    fork: Tuple[int, int]             # columns [lo, hi) the shadow reads from committed state: copied from the committed row
    tok_window: Tuple[int, int]       # tokens [lo, hi) the quantiser decodes now, for the committed and the shadow row alike
    z: Tuple[int, int]                # condition / level-0 frames [a, b) written to the shadow row: from the committed frontier to `upto`
    voc_window: Tuple[int, int]       # mel frames [lo, hi) the vocoder runs on, hi the window's own end (lo == hi: nothing to vocode)
    fade: int = 0                     # frames in front of emit[0] the vocoder window also renders (a cross-fading session: 1)

    @property
    def need_from(self) -> int:
        return max(0, self.step.need_from - self.fade)

    @property
    def upto(self) -> int:
        return self.step.upto


class EarlyDecodeSchedule:
    """A DecodeSchedule that hands frames out at most `lookahead` frames behind the newest one received.  The committed counters are a
    DecodeSchedule's, stepped exactly as an exact session steps them; on top of them `emitted` runs ahead of the last level:

        non-final   emitted -> max(emitted, the exact schedule's frontier, tokens * factor - lookahead)
        final       emitted -> tokens * factor, from the committed row (its final step is the true end: no shadow)

    When the third term wins, the frames come from the shadow row: a copy of the committed columns [fork) stepped from the committed
    frontiers to the newest frame on every level, as if the stream ended here.  With lookahead >= geo.hold_frames it never wins:
    every step is the exact schedule's, range for range.  The columns the shadow and its vocoder window read start at or behind the
    committed step's need_from, so decode_rebase and decode_capacity hold as they are.

    `lookahead` may change between steps (set_lookahead): the rule above is applied with the value of the moment.  What has left
    never comes back, so raising it only pauses emission until tokens * factor - lookahead passes `emitted`; every piece is still a
    crop of the prefix decode, and from a step with lookahead >= geo.hold_frames on the third term never wins again.

    fade_frames = 1 is the schedule of a session that cross-fades its audio pieces (utils/crossfade.py): the last samples of the frame
    in front of the emitted frontier are rendered again by the next decode, so the vocoder window starts one frame earlier,
    [emitted - voc_halo - 1, ...), and with it the fork window; need_from moves one frame back so that no re-base drops that
    column (the early frontier is never behind the exact one, so the widened window is at most one frame behind the exact
    need_from), and the capacity is decode_capacity(geo, max_push_tokens, extra_hold=1).  The wrapped DecodeSchedule is untouched."""

    def __init__(self, geo: DecodeGeometry, lookahead: int, fade_frames: int = 0):
        if fade_frames not in (0, 1):
            raise ValueError("fade_frames is 0 or 1: a cross-fade is at most one mel frame long")
        self.geo, self.fade_frames = geo, int(fade_frames)
        self.set_lookahead(lookahead)
        self.exact = DecodeSchedule(geo)
        self.emitted = 0

    def set_lookahead(self, lookahead: int) -> None:
        """the look-ahead of every later step"""
        if int(lookahead) < 0:
            raise ValueError("lookahead_frames must be >= 0")
        self.lookahead = int(lookahead)

    @property
    def tokens(self) -> int:
        return self.exact.tokens

    @property
    def finished(self) -> bool:
        return self.exact.finished

    @property
    def need_from(self) -> int:
        return max(0, self.exact.need_from - self.fade_frames)

    def step(self, n: int, final: bool = False) -> EarlyDecodeStep:
        g, ex = self.geo, self.exact
        z_before = ex.z_valid
        st = ex.step(n, final)
        T, e_prev, e_exact = st.upto, self.emitted, st.emit[1]
        e_new = T if final else max(e_prev, e_exact, T - self.lookahead)
        shadow = not final and e_new > max(e_prev, e_exact)
        halo, fade = g.voc_halo, self.fade_frames
        v_lo = max(0, e_prev - halo - fade)               # the vocoder window's first frame
        idle = (0, 0)
        if shadow:
            lo = min([st.prev[l + 1] - d for l, d in enumerate(g.dilations)] + [e_prev - halo - fade])
            lo = max(0, min(lo, ex.z_valid))
            row = dict(prev=st.prev, next=(T,) * len(st.prev), fork=(lo, ex.z_valid),
                       tok_window=(max(0, z_before // g.factor - g.quant_halo_tokens), st.tokens), z=(ex.z_valid, T),
                       voc_window=(v_lo, T) if halo else idle)
        else:
            ready = st.next[-1]
            row = dict(prev=st.prev, next=st.prev, fork=idle, tok_window=st.tok_window, z=(ex.z_valid, ex.z_valid),
                       voc_window=(v_lo, min(ready, e_new + halo)) if halo and e_new > e_prev else idle)
        self.emitted = e_new
        return EarlyDecodeStep(step=st, emit=(e_prev, e_new), shadow=shadow, fade=fade, **row)

    def state(self) -> dict:
        """the look-ahead of the moment, the fade, the early frontier and the wrapped exact schedule's counters, as plain values"""
        return dict(lookahead=self.lookahead, fade_frames=self.fade_frames, emitted=self.emitted, exact=self.exact.state())

    @classmethod
    def from_state(cls, geo: DecodeGeometry, state: Mapping) -> "EarlyDecodeSchedule":
        """the schedule that returns, for every later step(n, final), the step the one state() was taken from returns"""
        sc = cls(geo, int(state["lookahead"]), fade_frames=int(state["fade_frames"]))
        sc.exact = DecodeSchedule.from_state(geo, state["exact"])
        sc.emitted = int(state["emitted"])
        return sc


# ---------------------------------------------------------------------------------------------------- streaming sample-rate conversion
def resample_width(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> int:
    """half width of the windowed sinc in input samples (orig, new already divided by their gcd): torchaudio's
    `_get_sinc_resample_kernel`, as utils/resample.py: sinc_resample_bank evaluates it"""
    return int(math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)))


@dataclass(frozen=True)
class ResampleStep:
    samples: int                      # input samples received so far
    final: bool
    outputs: Tuple[int, int]          # output samples [a, b) that become final now
    reads: Tuple[int, int]            # input samples [lo, hi) they read inside the signal (lo == hi: none)
    keep_from: int                    # oldest input sample a later output still reads: the tail carried to the next step starts here
    total_length: int                 # -1 until the stream's end is known


class ResampleSchedule:
    """The counters of a streamed polyphase resampler (utils/resample.py: StreamResampler).  With down / up = orig / new in lowest terms,
    output o = n up + p (phase p of group n) reads the inputs [n down - width, n down + width + down), zero outside the signal.

    Mid-stream, after k input samples, group n is final once its last tap has arrived: n down + width + down - 1 < k, so
    groups_ready(k) = (k - width - down) // down + 1 for k >= width + down, else 0, and whole groups are emitted:
    outputs_ready(k) = up * groups_ready(k).  When the stream ends at length L the rest is emitted up to ceil(up L / down), the
    whole-clip output length, with zeros behind the end.

    Carried: the next group to emit, n = emitted / up, reads from n down - width, and nothing later reads in front of that.  Group n is
    not ready, so k < n down + width + down: the tail [n down - width, k) is shorter than kw = 2 width + down samples -- `width` of left
    context, and less than width + down of a group whose right context is still arriving.

    Latency: output m (0-based count m + 1) is final after samples_needed(m + 1) = ceil((m + 1) / up) down + width input samples, which is
    at most width + down source samples behind that output's own position m down / up: the latency the resampler adds."""

    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        if orig_freq <= 0 or new_freq <= 0:
            raise ValueError("Original frequency and desired frequecy should be positive")
        g = math.gcd(int(orig_freq), int(new_freq))
        self.down, self.up = int(orig_freq) // g, int(new_freq) // g
        self.width = resample_width(self.down, self.up, lowpass_filter_width, rolloff)
        self.kw = 2 * self.width + self.down
        self.samples = 0
        self.emitted = 0
        self.finished = False

    # -- pure functions of the rates --------------------------------------------------------------------------------
    def outputs_ready(self, k: int) -> int:
        """outputs whose every tap is among the first k samples of an unfinished stream (whole groups)"""
        need = self.width + self.down
        return 0 if k < need else ((k - need) // self.down + 1) * self.up

    def samples_needed(self, m: int) -> int:
        """inverse: the smallest k with outputs_ready(k) >= m"""
        return 0 if m <= 0 else -(-m // self.up) * self.down + self.width

    def total_outputs(self, length: int) -> int:
        """outputs of a finished clip of `length` samples: ceil(new * length / orig)"""
        return -(-self.up * length // self.down)

    def first_read(self, o: int) -> int:
        """oldest input sample output o reads (may be negative: zero padding)"""
        return (o // self.up) * self.down - self.width

    @property
    def max_tail(self) -> int:
        """the carried tail is always shorter than this"""
        return self.kw

    @property
    def tail_start(self) -> int:
        return max(0, self.first_read(self.emitted))

    # -- the stream ---------------------------------------------------------------------------------------------------
    def step(self, n: int, final: bool = False) -> ResampleStep:
        if self.finished:
            raise RuntimeError("stream already finished")
        if n < 0:
            raise ValueError("negative sample count")
        self.samples += n
        k = self.samples
        o_new = self.total_outputs(k) if final else self.outputs_ready(k)
        o_new = max(o_new, self.emitted)
        lo = hi = 0
        if o_new > self.emitted:
            lo = max(0, self.first_read(self.emitted))
            hi = max(lo, min(k, self.first_read(o_new - 1) + self.kw))
        st = ResampleStep(samples=k, final=final, outputs=(self.emitted, o_new), reads=(lo, hi),
                          keep_from=k if final else min(k, max(0, self.first_read(o_new))), total_length=k if final else -1)
        self.emitted = o_new
        self.finished = final
        return st

    def state(self) -> dict:
        """the counters as plain Python values -- nothing derived from the rates: what a snapshot of a session carries"""
        return dict(samples=self.samples, emitted=self.emitted, finished=self.finished)

    @classmethod
    def from_state(cls, rates: Tuple[int, int], state: Mapping) -> "ResampleSchedule":
        """rates: (orig_freq, new_freq).  The schedule that returns, for every later step(n, final), the step the one state() was
        taken from returns.  A state that no schedule of these rates can be in (outputs that are not whole groups) is refused."""
        sc = cls(int(rates[0]), int(rates[1]))
        sc.samples, sc.emitted, sc.finished = int(state["samples"]), int(state["emitted"]), bool(state["finished"])
        if sc.samples < 0 or sc.emitted < 0 or (not sc.finished and sc.emitted != sc.outputs_ready(sc.samples)):
            raise ValueError(f"a resampler state of {sc.emitted} outputs after {sc.samples} samples: not a state of {rates[0]} -> {rates[1]} Hz")
        return sc


def resample_max_outputs(orig_freq: int, new_freq: int, n: int) -> int:
    """The largest number of outputs one step of at most `n` samples can release, from any state a ResampleSchedule of this rate pair
    can be in: what the rows of a pool of resamplers (utils/resample.py: SessionResampler) and of the pools behind it are sized by.

    Mid-stream whole groups are released.  After k samples groups_ready(k) = (k - width) // down for k >= width + down (else 0) of them
    are out, and floor((k + n - width) / down) - floor((k - width) / down) <= n // down + 1: at most (n // down + 1) * up outputs.
    The final step flushes up to total_outputs(k + n) = ceil(up (k + n) / down).  With k = width + q down + r, 0 <= r < down, q up
    outputs are out already (fewer than `width` samples: none, and the flush is shorter still), which leaves
    ceil(up (width + r + n) / down), largest at r = down - 1.  That covers the mid-stream case as well (width >= 1), so it is the
    bound."""
    if n < 0:
        raise ValueError("negative sample count")
    sc = ResampleSchedule(orig_freq, new_freq)
    mid = (n // sc.down + 1) * sc.up
    last = sc.total_outputs(n + sc.width + sc.down - 1)
    return max(mid, last)


def resample_session_rows(slots: int, steps: Mapping[int, ResampleStep], s0: Sequence[int],
                          fill: Sequence[int]) -> Tuple[List[int], List[int], List[int], List[int], List[int]]:
    """session_rows for a pool of resamplers: the per-item tables of dmel_resample_window_items_f32.  steps: slot -> this step's
    ResampleStep of every slot that takes part; the slot's row holds the absolute samples [s0[slot], s0[slot] + fill[slot]), this
    step's chunk included.  Returns (s0, n_valid, o0, n_out, total_length), one entry per slot.  A slot without a step, or whose step
    releases no output, is idle: n_out 0 (and zeros, length unknown).  A step that reads outside its row is refused here, with the
    slot's name, before the library has to."""
    rs0, nv, o0, n_out, total = [0] * slots, [0] * slots, [0] * slots, [0] * slots, [-1] * slots
    for slot, st in steps.items():
        if not 0 <= slot < slots:
            raise ValueError(f"slot {slot} out of range")
        a, b = st.outputs
        if b <= a:
            continue
        lo, hi = st.reads
        if hi > lo and not (s0[slot] <= lo and hi <= s0[slot] + fill[slot]):
            raise ValueError(f"slot {slot}: outputs [{a}, {b}) read samples [{lo}, {hi}), the row holds "
                             f"[{s0[slot]}, {s0[slot] + fill[slot]})")
        rs0[slot], nv[slot], o0[slot], n_out[slot], total[slot] = s0[slot], fill[slot], a, b - a, st.total_length
    return rs0, nv, o0, n_out, total
