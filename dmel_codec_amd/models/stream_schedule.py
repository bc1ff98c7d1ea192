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

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple


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
