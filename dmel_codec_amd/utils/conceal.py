"""The packet-loss concealment rule of encode sessions opened with conceal= (models/stream_sessions.py: EncodeSessions), on the host:
the config, the per-session state, the scan over samples, the report a caller reads, and the map from lost wire frames to damaged
codec-rate samples.  The pool's kernel (dmel_conceal_items) is held to scan() bit for bit; only conceal_items(), the launch at the
end, needs a GPU.

RTP does not deliver every packet.  A caller that pushes nothing for a lost packet lets the session's timeline slip; one that pushes
zeros puts a pair of clicks into the encoder and an end of speech into every detector.  This rule is what a telephony front end
does instead: pitch waveform repetition, per session, on the session's samples at the codec's rate, as f32, behind the convert,
downmix and resample launches and in front of everything else.  It adds no latency: no sample is held back, the samples of a lost
range are re-written in place from the session's own recent output, and the first good samples behind it are cross-faded in.

Precision: everything is fp32, every operation is rounded on its own (no fused multiply-add), the divisions are the IEEE ones.  One
summation order for everything: sum8 as utils/echo.py defines it.  The float parameters reach the rule as fp32 values computed once
on the host: floor and eps as they are, rD = fp32(1 / D) (0 where D = 0) and rF = fp32(1 / (F + 1)), the divisions in float64,
rounded once.

Lengths, in samples at the codec's rate, from the config's milliseconds by cfg.samples(rate) (rounded to the nearest; W to the
nearest multiple of 8):  W the correlation window, [Pmin, Pmax] the lag range, H the repetition at full level, D the linear fade to
zero behind it, F the cross-fade into the first good samples.  Refused: W + Pmax > RING, H + D + Pmax > RING, Pmin < 8,
Pmin > Pmax, F < 1, W < 8.  RING = 4096.

State of a session: one row of ROW_WORDS = 16 + RING = 4112 4-byte words.  A zeroed row is a fresh session.

    0  T        int32   samples seen                               7   runs     int32   onsets
    1  phase    int32   0 good, 1 lost, 2 recovering               8   muted    int32   lost samples that were written as 0
    2  t0       int32   the onset: T at the run's first sample     9   longest  int32   the longest run that has ended
    3  P        int32   the period of the run, 0 = none            10  run      int32   length of the open or the last run
    4  k        int32   samples since the onset                    11  q        fp32    score of the last search (0: none ran)
    5  rec      int32   recovery samples left                      12  e0       fp32    window energy of the last search
    6  lost     int32   lost samples                               13 .. 15     reserved, kept at 0
    16 .. 4112  ring[4096]  fp32: the session's OUTPUT sample y[t] at word 16 + t mod RING

A call takes n samples and `ranges`: sorted, disjoint, non-touching [lo, hi) positions inside the n samples whose content is to be
ignored.  Per sample t, in order:

    a lost sample, first of a run (phase != 1) -- the onset:  t0 = T, k = 0, P = 0, run = 0, runs += 1, q = e0 = 0, phase = 1.
        The search runs only if T >= W + Pmax:  a[i] = ring[t0 - W + i], i = 0 .. W - 1;  e0 = sum8(a * a).  If e0 >= floor, for
        every lag p in [Pmin, Pmax]:  b[i] = ring[t0 - W + i - p];  c = sum8(a * b);  e = sum8(b * b);
        q(p) = c > 0 ? (c * c) / (e + eps) : 0  (a product, a sum, a division).  P is the lag of the largest q, the lowest lag of
        equal ones, and 0 if that q is 0; q is that largest value.  The argmax is over the VALUES q, never over cross-multiplied
        comparisons: it is a total order, so the order of the reduction cannot matter.
    the synthetic sample s(k):  0 if P == 0 or k >= H + D (the zero branch);  else v = ring[t0 - P + (k mod P)], and s = v for
        k < H, else u = (float)(k - H) * rD;  g = 1.0f - u;  s = g * v.  Reads lie in front of t0, writes at or behind it; the config
        checks keep the ring from lapping a word that is still read.
    a lost sample:  y = s(k);  k += 1;  lost += 1;  run += 1;  muted += 1 if y came from the zero branch.
    a good sample behind a run (phase == 1):  longest = max(longest, run);  phase = 2;  rec = F.
    a good sample while rec > 0:  i = F - rec;  w = (float)(i + 1) * rF;  d = x - s(k);  m = w * d;  y = s(k) + m;  k += 1;
        rec -= 1;  at rec == 0, phase = 0.  A lost sample during recovery is a new onset, searched on the ring as it then is.
    any other good sample:  y = x, bit for bit.
    always:  ring[T mod RING] = y;  T += 1.

A run that reaches the end of a call stays open (phase 1) and continues if the next call's first range starts at 0.  Everything
the rule reads is in the row, so the result cannot depend on how samples and ranges were cut into calls.

THE DEFAULTS ARE CHECKED ON SYNTHETIC SIGNALS ONLY (table-periodic noise and a harmonic voiced-like signal with vibrato, tremolo
and noise: tests/test_conceal_cpu.py) and are not tuned on speech or on lines.  The rule follows ITU-T G.711 Appendix I in spirit
and claims no conformance.  There is no overlap-add into the last good samples in front of a run: that needs 3.75 ms of delay and
this option adds none, so a run may begin with a small step.  The pitch buffer does not grow to 2 or 3 periods in a long run: one
period is repeated until the fade ends.  The counters are int32; nothing checks for their overflow (2^31 samples at 24 kHz are
24.8 hours).  NaN input is outside the contract.  Not served: jitter buffers, reordering, FEC / RED, comfort noise."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from ..models.stream_schedule import ResampleSchedule
from .echo import _sum8_even, sum8

HEADER_WORDS = 16
RING = 4096
ROW_WORDS = HEADER_WORDS + RING                        # 4112
MAX_RANGES = 16                                        # lost ranges one slot of a launch takes
TABLE_WORDS = 16 + 2 * MAX_RANGES                      # 4-byte words of table scratch per slot of dmel_conceal_items
I_T, I_PHASE, I_T0, I_P, I_K, I_REC, I_LOST, I_RUNS, I_MUTED, I_LONGEST, I_RUN, I_Q, I_E0 = range(13)
SILENCE = {"f32": 0.0, "s16": 0, "ulaw": 0xFF, "alaw": 0xD5}            # what a pool puts in the place of a lost frame, per wire format
_MASK = RING - 1
_MS = ("window_ms", "min_period_ms", "max_period_ms", "hold_ms", "fade_ms", "recover_ms")


@dataclasses.dataclass(frozen=True)
class ConcealConfig:
    """Plain values; see the module for what each does.  The defaults are checked on synthetic signals only."""
    window_ms: float = 20.0                            # W: the correlation window
    min_period_ms: float = 2.5                         # Pmin: 400 Hz
    max_period_ms: float = 15.0                        # Pmax: 66.7 Hz
    hold_ms: float = 10.0                              # H: repetition at full level
    fade_ms: float = 50.0                              # D: linear fade to zero behind it
    recover_ms: float = 5.0                            # F: cross-fade into the first good samples
    floor: float = 1e-4                                # window energy below which nothing is repeated
    eps: float = 1e-12

    def __post_init__(self):
        f32 = np.finfo(np.float32)
        for name in _MS + ("floor", "eps"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
            object.__setattr__(self, name, float(v))
        for name in ("floor", "eps"):
            v = getattr(self, name)
            if v != 0 and not float(f32.tiny) <= v <= float(f32.max):       # what the kernel computes with is the fp32 value
                raise ValueError(f"{name} = {v!r} is no normal fp32 number")
        if not self.eps > 0.0:
            raise ValueError(f"eps must be > 0, got {self.eps!r}")

    def samples(self, sample_rate: int) -> Tuple[int, int, int, int, int, int]:
        """(W, Pmin, Pmax, H, D, F) at `sample_rate`; ValueError where the rate or a length does not fit"""
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:      # in front of the cache: 24000.0 == 24000
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        return _samples(self, sample_rate)

    def fparams(self, sample_rate: int) -> Tuple[float, float, float, float]:
        """(floor, eps, rD, rF) as the fp32 values scan and dmel_conceal_items compute with"""
        return _fparams(self, sample_rate)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "ConcealConfig":
        return cls(**dict(d))


def check_lengths(W: int, Pmin: int, Pmax: int, H: int, D: int, F: int) -> None:
    """the bounds of the module on the lengths, as dmel_conceal_items refuses them"""
    if W < 8 or W % 8:
        raise ValueError(f"a correlation window of {W} samples: expected a multiple of 8, at least 8")
    if Pmin < 8 or Pmin > Pmax:
        raise ValueError(f"a lag range of [{Pmin}, {Pmax}] samples: expected 8 <= Pmin <= Pmax")
    if W + Pmax > RING:
        raise ValueError(f"a window of {W} samples and a longest period of {Pmax} exceed the ring of {RING}")
    if H < 0 or D < 0 or H + D + Pmax > RING:
        raise ValueError(f"a hold of {H}, a fade of {D} and a longest period of {Pmax} samples exceed the ring of {RING}")
    if F < 1:
        raise ValueError(f"a recovery of {F} samples: expected at least 1")


@functools.lru_cache(maxsize=64)
def _samples(config: ConcealConfig, sample_rate: int) -> Tuple[int, int, int, int, int, int]:
    near = lambda ms: int(math.floor(ms * sample_rate / 1000.0 + 0.5))
    W = 8 * int(math.floor(config.window_ms * sample_rate / 8000.0 + 0.5))
    out = (W,) + tuple(near(getattr(config, name)) for name in _MS[1:])
    check_lengths(*out)
    return out


@functools.lru_cache(maxsize=64)
def _fparams(config: ConcealConfig, sample_rate: int) -> Tuple[float, float, float, float]:
    """a pool asks for them on every step"""
    _, _, _, _, D, F = config.samples(sample_rate)
    return tuple(float(np.float32(v)) for v in (config.floor, config.eps, 1.0 / D if D else 0.0, 1.0 / (F + 1)))


def as_config(conceal) -> Optional[ConcealConfig]:
    """what open(conceal=) takes: None / False -> None, True -> the defaults, a ConcealConfig -> itself"""
    if conceal is None or conceal is False:
        return None
    if conceal is True:
        return ConcealConfig()
    if isinstance(conceal, ConcealConfig):
        return conceal
    raise ValueError(f"conceal must be None, a bool or a ConcealConfig, got {type(conceal).__name__}")


def fresh_state() -> torch.Tensor:
    """(4112,) int32 zeros: the state of a session that has seen no sample"""
    return torch.zeros(ROW_WORDS, dtype=torch.int32)


def _check_state(state: torch.Tensor) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (ROW_WORDS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {ROW_WORDS} words, got {tuple(state.shape)} {state.dtype}")


def check_ranges(ranges, n: int) -> List[Tuple[int, int]]:
    """sorted, disjoint, non-touching, non-empty [lo, hi) inside [0, n], at most MAX_RANGES of them -> a list of int pairs"""
    out: List[Tuple[int, int]] = []
    for r in ranges:
        lo, hi = (int(v) for v in r)
        if not 0 <= lo < hi <= n:
            raise ValueError(f"the range [{lo}, {hi}) is empty or no part of {n} samples")
        if out and lo <= out[-1][1]:
            raise ValueError(f"the range [{lo}, {hi}) is not behind [{out[-1][0]}, {out[-1][1]}) with a gap: ranges are sorted and do not touch")
        out.append((lo, hi))
    if len(out) > MAX_RANGES:
        raise ValueError(f"{len(out)} lost ranges in one call, at most {MAX_RANGES}")
    return out


def _synth(ring: np.ndarray, t0: int, P: int, k0: int, m: int, H: int, D: int, rD: np.float32) -> np.ndarray:
    """s(k0 .. k0 + m), every source read before any of the samples is written"""
    s = np.zeros(m, dtype=np.float32)
    live = 0 if P == 0 else max(0, min(m, H + D - k0))                       # the samples in front of the zero branch
    if live:
        k = k0 + np.arange(live, dtype=np.int64)
        v = ring[(t0 - P + k % P) & _MASK]
        u = (k - H).astype(np.float32) * rD
        g = np.float32(1.0) - u
        s[:live] = np.where(k < H, v, g * v)
    return s


def scan(x, ranges, config: ConcealConfig, state: Optional[torch.Tensor] = None,
         sample_rate: int = 24000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """x: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0, at `sample_rate`; ranges: the lost [lo, hi) of this call
    (check_ranges); state: what an earlier call returned (None: fresh) -> (y (n,) fp32: the concealed samples, state after the
    samples, periods (R,) int32, scores (R,) fp32) over the R onsets of the call.  No argument is modified.  Any cut of samples and
    ranges into calls gives the bits of one call."""
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"samples must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    W, Pmin, Pmax, H, D, F = config.samples(sample_rate)
    floor, eps, rD, rF = (np.float32(v) for v in config.fparams(sample_rate))
    n = int(x.shape[0])
    ranges = check_ranges(ranges, n)
    if state is None:
        state = fresh_state()
    _check_state(state)
    words = state.clone().numpy()
    fl = words.view(np.float32)
    y = x.copy()
    periods, scores = [], []
    if n == 0:                                                               # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(y), torch.from_numpy(words), torch.zeros(0, dtype=torch.int32), torch.zeros(0)
    T, phase, t0, P, k, rec, lost, runs, muted, longest, run = (int(words[i]) for i in range(I_RUN + 1))
    q, e0 = np.float32(fl[I_Q]), np.float32(fl[I_E0])
    ring = fl[HEADER_WORDS:]

    def put(at: int, ys: np.ndarray) -> None:                                # ring[(T + i) mod RING] = ys[i]; the newest RING of them count
        ys, at = ys[-RING:], at + max(0, ys.shape[0] - RING)
        ring[(at + np.arange(ys.shape[0], dtype=np.int64)) & _MASK] = ys

    pos = 0
    for lo, hi in ranges + [(n, n)]:
        if pos < lo:                                                         # a good stretch [pos, lo)
            if phase == 1:
                longest, phase, rec = max(longest, run), 2, F
            r = min(rec, lo - pos) if phase == 2 else 0
            if r:
                s = _synth(ring, t0, P, k, r, H, D, rD)
                w = np.arange(F - rec + 1, F - rec + 1 + r).astype(np.float32) * rF
                d = x[pos:pos + r] - s
                m = w * d
                y[pos:pos + r] = s + m
                k, rec = k + r, rec - r
                if rec == 0:
                    phase = 0
            put(T, y[pos:lo])
            T, pos = T + (lo - pos), lo
        if lo == hi:
            break
        if phase != 1:                                                       # the onset
            t0, k, P, run, runs, phase = T, 0, 0, 0, runs + 1, 1
            q, e0 = np.float32(0.0), np.float32(0.0)
            if T >= W + Pmax:
                h = ring[(t0 - W - Pmax + np.arange(W + Pmax, dtype=np.int64)) & _MASK]
                a = h[Pmax:]
                e0 = sum8(a * a)
                if e0 >= floor:
                    B = np.lib.stride_tricks.sliding_window_view(h, W)[Pmax - Pmin::-1][:Pmax - Pmin + 1]    # row j: the lag Pmin + j
                    c = _sum8_even(a[None, :] * B)
                    e = _sum8_even(B * B)
                    with np.errstate(over="ignore", invalid="ignore"):
                        qs = np.where(c > 0, (c * c) / (e + eps), np.float32(0.0)).astype(np.float32)
                    j = int(np.argmax(qs))                                   # the first of equal ones: the lowest lag
                    q = np.float32(qs[j])
                    P = Pmin + j if q > 0 else 0
            periods.append(P), scores.append(q)
        m = hi - lo
        y[lo:hi] = _synth(ring, t0, P, k, m, H, D, rD)
        muted += m if P == 0 else max(0, k + m - max(k, H + D))
        put(T, y[lo:hi])
        k, lost, run, T, pos = k + m, lost + m, run + m, T + m, hi
    words[:I_RUN + 1] = (T, phase, t0, P, k, rec, lost, runs, muted, longest, run)
    fl[I_Q], fl[I_E0] = q, e0
    return (torch.from_numpy(y), torch.from_numpy(words), torch.from_numpy(np.array(periods, dtype=np.int32)),
            torch.from_numpy(np.array(scores, dtype=np.float32)))


def damaged(lost_wire_ranges, orig: int, new: int) -> List[Tuple[int, int]]:
    """the ranges of samples at the rate `new` that lost wire frames [lo, hi) at the rate `orig` damage, sorted, touching and
    overlapping ones merged.  At one rate: the wire ranges themselves.  Through the resampler (utils/resample.py): every output
    whose filter window reads at least one lost frame -- with ResampleSchedule's counters, the outputs of every group g whose
    window [g down - width, g down + width + down) meets [lo, hi).  No such output had been released when the first lost frame
    arrived (its window was not complete), so the ranges never reach behind what a session has already released; they may reach
    beyond the end of a stream that ends early."""
    pairs = sorted((int(lo), int(hi)) for lo, hi in lost_wire_ranges)
    if any(lo < 0 or hi < lo for lo, hi in pairs):
        raise ValueError(f"lost wire ranges must be [lo, hi) with 0 <= lo <= hi, got {pairs}")
    pairs = [p for p in pairs if p[1] > p[0]]
    if int(orig) != int(new):
        sc = ResampleSchedule(int(orig), int(new))
        # the first group whose window ends behind lo; the first one whose window begins at or behind hi
        pairs = [(max(0, (lo - sc.width - sc.down) // sc.down + 1) * sc.up, -(-(hi + sc.width) // sc.down) * sc.up) for lo, hi in pairs]
    out: List[Tuple[int, int]] = []
    for lo, hi in pairs:
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


@dataclasses.dataclass(frozen=True)
class ConcealReport:
    """What a caller reads of a session's concealment, built from the header of its state row.  Samples are samples at the codec's
    rate.

        lost_samples       samples inside lost ranges;  muted_samples: those of them written as 0 (no period found, a young or a
                           silent session, or behind the fade)
        runs               lost runs so far (onsets);  longest_run: the longest of them, the open one included
        open               whether the last sample seen was lost
        period, score      of the last search: the lag repeated (0: none) and its normalised correlation energy
        total_samples      samples seen;  lost_ratio: lost_samples / total_samples (0.0 before the first sample)
    """
    lost_samples: int
    runs: int
    longest_run: int
    muted_samples: int
    open: bool
    period: int
    score: float
    total_samples: int
    lost_ratio: float
    sample_rate: int = 24000

    def samples(self, seconds: float) -> int:
        """a duration in samples at the codec's rate, rounded to the nearest"""
        return int(math.floor(float(seconds) * self.sample_rate + 0.5))

    def seconds(self, samples: Optional[int] = None) -> float:
        """a count of samples (default: lost_samples) in seconds"""
        return (self.lost_samples if samples is None else int(samples)) / self.sample_rate


def report(state: torch.Tensor, sample_rate: int = 24000) -> ConcealReport:
    """the report of a state row, or of its first 16 words (any device -- one copy to the host)"""
    row = state[:HEADER_WORDS].cpu()
    w, f = [int(v) for v in row.tolist()], [float(v) for v in row.view(torch.float32).tolist()]
    is_open = w[I_PHASE] == 1
    return ConcealReport(lost_samples=w[I_LOST], runs=w[I_RUNS], longest_run=max(w[I_LONGEST], w[I_RUN]) if is_open else w[I_LONGEST],
                         muted_samples=w[I_MUTED], open=is_open, period=w[I_P], score=f[I_Q], total_samples=w[I_T],
                         lost_ratio=w[I_LOST] / w[I_T] if w[I_T] > 0 else 0.0, sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def conceal_items(samples: torch.Tensor, first: Sequence[int], n_new: Sequence[int], ranges: Sequence[Sequence[Tuple[int, int]]],
                  configs: Sequence[Optional[ConcealConfig]], state: torch.Tensor, out_period: torch.Tensor, out_score: torch.Tensor,
                  sample_rate: int = 24000, table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_conceal_items).  samples: (S, width) fp32 CUDA with contiguous columns; slot s takes
    the n_new[s] samples at columns [first[s], first[s] + n_new[s]) of its row through the rule, ranges[s] (relative to first[s])
    lost, and re-writes IN PLACE the lost ranges and the recovery stretches behind them (0 samples: the slot is idle, its rows are
    not touched, configs[s] may be None); no other column is written.  state: (S, 4112) int32, contiguous, updated in place;
    out_period: (S, pitch) int32, out_score: (S, pitch) fp32, contiguous, pitch >= len(ranges[s]) for every s; the words behind the
    onsets a row had are not written.  table: int32 device scratch of 48 * S words a caller that conceals every step keeps
    (default: allocated here).  Runs on the current stream."""
    _lib.require_cuda(samples, "samples")
    if samples.ndim != 2 or samples.dtype != torch.float32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be an fp32 tensor (S, width) with contiguous columns, got {tuple(samples.shape)} {samples.dtype}")
    S, width = (int(v) for v in samples.shape)
    dev = samples.device
    if len(first) != S or len(n_new) != S or len(ranges) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} offsets, counts, range lists and configs, got {len(first)}, {len(n_new)}, {len(ranges)} "
                         f"and {len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, ROW_WORDS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {ROW_WORDS}) on {dev}")
    for t, name, dt in ((out_period, "out_period", torch.int32), (out_score, "out_score", torch.float32)):
        if t.dtype != dt or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {dt} tensor ({S}, pitch) on {dev}")
    if out_period.shape[1] != out_score.shape[1]:
        raise ValueError("out_period and out_score must have one pitch")
    nr, rg, ip, fp = [], [], [], []
    for s in range(S):
        n, f = int(n_new[s]), int(first[s])
        if n < 0 or (n and not 0 <= f <= width - n):
            raise ValueError(f"slot {s}: columns [{f}, {f + n}) are no part of a row of {width} samples")
        if n and configs[s] is None:
            raise ValueError(f"slot {s} has {n} samples and no config")
        cfg = configs[s] if n else None
        mine = check_ranges(ranges[s], n) if n else []
        nr.append(len(mine))
        rg += [v for r in mine for v in r] + [0] * (2 * (MAX_RANGES - len(mine)))
        ip += cfg.samples(sample_rate) if cfg else (0,) * 6
        fp += cfg.fparams(sample_rate) if cfg else (0.0,) * 4
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    I64 = C.c_int64 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_conceal_items(samples.data_ptr(), samples.stride(0), S, I64(*[int(v) for v in first]),
                                                 I64(*[int(v) for v in n_new]), (C.c_int32 * S)(*nr),
                                                 (C.c_int32 * (2 * MAX_RANGES * S))(*rg), (C.c_int32 * (6 * S))(*ip),
                                                 (C.c_float * (4 * S))(*fp), state.data_ptr(), ROW_WORDS, out_period.data_ptr(),
                                                 out_score.data_ptr(), int(out_period.shape[1]), table.data_ptr(), _lib.stream_ptr()),
                   "conceal_items")
