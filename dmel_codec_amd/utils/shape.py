"""The reply-shaping rule of decode sessions opened with shape= in pools built with shape=True (models/stream_sessions.py:
DecodeSessions.set_gain / stop), on the host: the config, the requests and their segments, the per-session state row, the scan over
samples, and the report a caller reads.  The pool's kernel (dmel_shape_items) is held to scan() bit for bit; only shape_items(), the
launch at the end, needs a GPU.

The rule acts on z, the session's float stream at the vocoder's rate as it leaves the tone splice: speech, cross-faded where the
session fades, with tones spliced in.  Positions are absolute sample indices of z.  Three things happen to it, in this order: a
commanded gain that ramps between requests, a block look-ahead limiter, and an end of stream that fades instead of clicks.

COMMANDED GAIN c[i].  A session starts at initial_gain.  A REQUEST is (P, g1, ramp): from sample P the gain moves to g1 over `ramp`
samples, 0 <= g1 <= max_gain, 0 <= ramp <= 16384, anchors P do not decrease (equal anchors: the later request wins).  plan() turns
the requests into SEGMENTS (P, g0, g1, ramp), where g0 is the value the trajectory so far has at P, computed in fp32 with the
formula below -- so a request may interrupt an earlier ramp.  Sample i belongs to the last segment with P <= i (initial_gain, or
the base gain, in front of the first), and with k = i - P:

    k <  ramp:   d = g1 - g0;   m = d * RAMP[k];   c = g0 + m        (separately rounded fp32 operations, no fused multiply-add)
    k >= ramp:   c = g1                                              (exactly)

RAMP = ramp_table(ramp), RAMP[k] = fp32(0.5 - 0.5 cos(pi (k + 0.5) / ramp)), computed in float64 and rounded once: the table
definition of utils/tones.py.  At most 8 segments of a slot are live in one launch; live() folds what is finished into a base
gain, which is exact because a finished ramp sits on g1.

GAINED SAMPLE.  v = z * c, one rounded operation.

LIMITER (limit=True).  Blocks are N consecutive samples of v, counted from the session's first sample (block_samples=None: 5 ms,
(rate + 100) // 200; 32 <= N <= 1024).  Per completed block b, p_b = max |v| over the block:

    t_b = p_b > ceiling ? ceiling / p_b : 1.0f                  (the IEEE fp32 division)
    u = 1.0f - s_{b-1};   u = release * u;   r = s_{b-1} + u
    s_b = min(t_b, r)                                           (s_{-1} = 1.0f)
    n_b = min(s_{b-1}, s_b)                                     (the gain at the start of block b)

Block b leaves when block b + 1 is complete.  Sample i of the block, four rounded operations and the product:

    d = n_{b+1} - n_b;   u = fp32(i + 1) * rN;   m = d * u;   gi = n_b + m;   y = v * gi          (rN = fp32(1 / N))
    y >  ceiling: y =  ceiling, clamped += 1;      y < -ceiling: y = -ceiling, clamped += 1

WHY |y| <= ceiling.  Both nodes of block b are at most s_b: n_b = min(s_{b-1}, s_b) <= s_b and n_{b+1} = min(s_b, s_{b+1}) <= s_b.
gi lies between the nodes (u is in (0, 1]), up to rounding, and s_b <= t_b, so |v| gi <= p_b t_b <= ceiling up to rounding.
The clamp can only catch that rounding excess, and `clamped` counts it; the bound itself holds for every finite input because of
the clamp.

The session's audio therefore runs between N and 2 N - 1 samples behind z and leaves in whole blocks.  On the session's last step
(final) everything held leaves: the open block's peak is taken over the samples it has, it counts as a completed block,
n_{last+1} = s_last, and the total length is kept.  emitted() gives the count of a step from integers alone.

limit=False: no delay, nothing held.  y = clamp(v), clamped samples counted.  With gain 1.0 and |z| <= ceiling the output is z bit for
bit.

END.  A session may carry an end sample E (DecodeSessions.stop sets it behind a request (now, 0, ramp)): z is cut at E, the step
that reaches it is the session's last, and the hold is flushed as above.

State of a session: a row of HEADER = 16 4-byte words and, with the limiter, 2 N - 1 floats: the held samples of v, oldest first.

    0  s          fp32   s of the last completed block            7  c_now     fp32   c of the last sample taken
    1  node       fp32   n of the held whole block (else s)       8  s_min     fp32   the smallest s so far
    2  open_peak  fp32   max |v| of the open block                9  limited   int32  blocks with p > ceiling
    3  hold       int32  samples held, 0 .. 2 N - 1               10 clamped   int32
    4  blocks     int32  completed blocks                         11 peak_in   fp32   max |z|
    5  in         int32  samples of z taken                       12 peak_out  fp32   max |y|
    6  out        int32  samples handed out                       13 .. 15     reserved, kept at 0

A zeroed row is the fresh state: while in == 0, s, node and s_min read as 1.0f whatever the row holds, and a step writes them back.
The words of the hold behind the held samples are kept at 0, so rows compare as wholes.  The held samples, open_peak and the fill
are carried, so the result cannot depend on how the stream was cut into pushes.

THE DEFAULTS (ceiling 0.98, release 0.1 per block, max_gain 4.0) ARE CHECKED ON SYNTHETIC SIGNALS ONLY (sines, noise with a burst,
single spikes: tests/test_shape_cpu.py) and are not tuned on speech.  The counters are int32; nothing checks for their overflow.
NaN and infinite input are outside the contract.  Not served: loudness (LUFS) targets, multiband or sample-accurate sliding-window
limiting, gain on the mel."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from . import tones

HEADER = 16
MIN_BLOCK, MAX_BLOCK = 32, 1024
MAX_RAMP = 16384
MAX_SEGMENTS = 8                                       # live segments of a slot in one launch
SEG_WORDS = 5                                          # start (relative to the first new sample), ramp, ramp_off, g0, g1
FPARAMS = 5                                            # ceiling, release, rN, base gain, max_gain
TABLE_WORDS = 64                                       # 4-byte words of table scratch per slot of dmel_shape_items
PASS_SAMPLES, PASS_BLOCKS = 4096, 63                   # what one pass of the kernel's workgroup emits from LDS
I_S, I_NODE, I_OPEN, I_HOLD, I_BLOCKS, I_IN, I_OUT, I_C, I_SMIN, I_LIMITED, I_CLAMPED, I_PEAK_IN, I_PEAK_OUT = range(13)
_FLOATS = ("ceiling", "release", "max_gain", "initial_gain")

Request = Tuple[int, float, int]                       # (P, g1, ramp)
Segment = Tuple[int, float, float, int]                # (P, g0, g1, ramp)


def default_block(rate: int) -> int:
    """5 ms in samples of `rate`, rounded to the nearest"""
    return (int(rate) + 100) // 200


def ramp_table(n: int) -> np.ndarray:
    """(n,) fp32, read-only: tones' table definition, for n in [0, 16384]"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= MAX_RAMP:
        raise ValueError(f"a gain ramp has 0 .. {MAX_RAMP} samples, got {n!r}")
    return tones._ramp(int(n))


@dataclasses.dataclass(frozen=True)
class ShapeConfig:
    """Plain values; see the module for what each does.  block_samples: None for 5 ms at the rate the shaper runs at.  The defaults
    are checked on synthetic signals only."""
    block_samples: Optional[int] = None
    limit: bool = True
    ceiling: float = 0.98
    release: float = 0.1
    max_gain: float = 4.0
    initial_gain: float = 1.0

    def __post_init__(self):
        n = self.block_samples
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not MIN_BLOCK <= n <= MAX_BLOCK):
            raise ValueError(f"block_samples must be None or an integer in [{MIN_BLOCK}, {MAX_BLOCK}], got {n!r}")
        if not isinstance(self.limit, bool):
            raise ValueError(f"limit must be a bool, got {self.limit!r}")
        for name in _FLOATS:
            v = getattr(self, name)
            zero_ok = name == "initial_gain"
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (v == 0 and not zero_ok):
                raise ValueError(f"{name} must be a finite number {'>= 0' if zero_ok else '> 0'}, got {v!r}")
            object.__setattr__(self, name, float(v))
        if self.release > 1.0:
            raise ValueError(f"release must be in (0, 1], got {self.release!r}")
        if self.initial_gain > self.max_gain:
            raise ValueError(f"initial_gain {self.initial_gain!r} must lie in [0, max_gain] = [0, {self.max_gain!r}]")
        f32 = np.finfo(np.float32)
        for name in _FLOATS:
            v = getattr(self, name)
            if v != 0 and not float(f32.tiny) <= v <= float(f32.max):       # what the kernel computes with is the fp32 value
                raise ValueError(f"{name} = {v!r} is no normal fp32 number")

    def block(self, rate: int) -> int:
        """N at `rate`; ValueError where the rate or the block does not fit"""
        if isinstance(rate, bool) or not isinstance(rate, int) or rate <= 0:
            raise ValueError(f"rate must be a positive integer, got {rate!r}")
        n = default_block(rate) if self.block_samples is None else self.block_samples
        if not MIN_BLOCK <= n <= MAX_BLOCK:
            raise ValueError(f"a block of {n} samples at {rate} Hz is outside [{MIN_BLOCK}, {MAX_BLOCK}]: set block_samples")
        return n

    def state_words(self, rate: int) -> int:
        """4-byte words of a session's state row: the header, and 2 N - 1 held samples with the limiter"""
        return HEADER + (2 * self.block(rate) - 1 if self.limit else 0)

    def fparams(self, rate: int) -> Tuple[float, ...]:
        """(ceiling, release, rN, initial_gain, max_gain) as the fp32 values scan and dmel_shape_items compute with"""
        return _fparams(self, rate)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "ShapeConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _fparams(config: ShapeConfig, rate: int) -> Tuple[float, ...]:
    n = config.block(rate)
    return tuple(float(np.float32(v)) for v in (config.ceiling, config.release, 1.0 / n, config.initial_gain, config.max_gain))


def as_config(shape) -> Optional[ShapeConfig]:
    """what open(shape=) takes: None / False -> None, True -> the defaults, a ShapeConfig -> itself"""
    if shape is None or shape is False:
        return None
    if shape is True:
        return ShapeConfig()
    if isinstance(shape, ShapeConfig):
        return shape
    raise ValueError(f"shape must be None, a bool or a ShapeConfig, got {type(shape).__name__}")


# ---------------------------------------------------------------------------------------------------- the commanded gain
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_request(request, config: ShapeConfig, after: int = 0) -> Request:
    """(P, g1, ramp) as plain values, g1 rounded to fp32; ValueError outside the bounds of the module.  after: the smallest anchor
    allowed (an earlier request's)"""
    try:
        P, g1, ramp = request
    except (TypeError, ValueError):
        raise ValueError(f"a request is (P, g1, ramp), got {request!r}") from None
    if not _is_int(P) or not after <= P < 2 ** 31:
        raise ValueError(f"a request's anchor must be an integer in [{after}, 2^31) (anchors do not decrease), got {P!r}")
    if isinstance(g1, bool) or not isinstance(g1, (int, float, np.floating)) or not math.isfinite(g1) or not 0 <= g1 <= config.max_gain:
        raise ValueError(f"a request's gain must be a finite number in [0, max_gain] = [0, {config.max_gain!r}], got {g1!r}")
    if not _is_int(ramp) or not 0 <= ramp <= MAX_RAMP:
        raise ValueError(f"a request's ramp must be an integer in [0, {MAX_RAMP}] samples, got {ramp!r}")
    return int(P), float(np.float32(g1)), int(ramp)


def gain_at(segments: Sequence[Segment], base: float, i: int) -> np.float32:
    """c[i] of a trajectory: the last segment with P <= i (the base gain in front of the first), in fp32"""
    seg = None
    for sg in segments:
        if sg[0] <= i:
            seg = sg
    if seg is None:
        return np.float32(base)
    P, g0, g1, ramp = seg
    k = i - P
    if k >= ramp:
        return np.float32(g1)
    d = np.float32(g1) - np.float32(g0)
    m = d * ramp_table(ramp)[k]
    return np.float32(g0) + m


def extend(segments: Sequence[Segment], base: float, request: Request) -> Segment:
    """the segment a checked request becomes behind `segments`: g0 is what the trajectory so far has at its anchor"""
    P, g1, ramp = request
    return (P, float(gain_at(segments, base, P)), g1, ramp)


def plan(requests: Sequence[Request], config: ShapeConfig) -> List[Segment]:
    """all requests of a session, in order -> its segments"""
    segs, after = [], 0
    for r in requests:
        r = check_request(r, config, after)
        segs.append(extend(segs, config.initial_gain, r))
        after = r[0]
    return segs


def live(segments: Sequence[Segment], base: float, pos: int) -> Tuple[List[Segment], float]:
    """what samples at and behind `pos` still need: the segments that can be the last one with P <= i for some i >= pos, and the
    base gain in front of them.  A segment that has finished at `pos` and is not followed by one that has begun is folded into the
    base: it sits on g1."""
    a = -1
    for k, sg in enumerate(segments):
        if sg[0] <= pos:
            a = k
    if a < 0:
        return list(segments), float(base)
    P, _, g1, ramp = segments[a]
    if P + ramp <= pos:
        return list(segments[a + 1:]), float(g1)
    return list(segments[a:]), float(base)


def commanded(segments: Sequence[Segment], base: float, pos: int, n: int) -> np.ndarray:
    """(n,) fp32: c[pos .. pos + n)"""
    c = np.full(n, np.float32(base), dtype=np.float32)
    for P, g0, g1, ramp in segments:                    # in order: a later segment overwrites from its anchor on
        a = max(P - pos, 0)
        if a >= n:
            continue
        k = np.arange(a + pos - P, n + pos - P, dtype=np.int64)
        g0f, g1f = np.float32(g0), np.float32(g1)
        out = np.full(n - a, g1f, dtype=np.float32)
        inside = k < ramp
        if inside.any():
            d = g1f - g0f
            m = d * ramp_table(ramp)[k[inside]]
            out[inside] = g0f + m
        c[a:] = out
    return c


# ---------------------------------------------------------------------------------------------------- the scan
def emitted(fill: int, n_new: int, N: int, final: bool, limit: bool = True) -> int:
    """samples a step hands out: fill: the samples the session holds (the row's `hold`, 0 .. 2 N - 1), n_new: the samples of z the
    step takes.  Whole blocks but the newest completed one; everything on the last step; n_new without the limiter."""
    total = int(fill) + int(n_new)
    if final or not limit:
        return total
    return max(0, total // int(N) - 1) * int(N)


def completed(fill: int, n_new: int, N: int, final: bool, limit: bool = True) -> int:
    """blocks a step completes: what a row of out_peak / out_gain must take"""
    if not limit:
        return 0
    N, total = int(N), int(fill) + int(n_new)
    return total // N + (1 if final and total % N else 0) - (1 if fill >= N else 0)


def fresh_state(config: ShapeConfig, rate: int) -> torch.Tensor:
    """int32 zeros of config.state_words(rate): the state of a session that has taken no sample"""
    return torch.zeros(config.state_words(rate), dtype=torch.int32)


def scan(z, requests: Sequence[Request], config: ShapeConfig, rate: int, end: Optional[int] = None,
         state: Optional[torch.Tensor] = None, final: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """z: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0, at `rate`, the samples behind those `state` has taken;
    requests: ALL requests of the session so far, [(P, g1, ramp), ...] at absolute positions; end: E, or None; state: what an
    earlier call returned (None: fresh); final: these are the session's last samples -> (y fp32: the samples handed out, state
    after the step, block_peaks (B,) fp32, block_gains (B,) fp32: p_b and s_b of the B blocks the step completed).  Neither z nor
    state is modified.  Any cut of the samples gives the bits of one call.  n == 0 without final (and without reaching E) is an
    idle step: the state comes back as it is."""
    x = z.numpy() if isinstance(z, torch.Tensor) else np.asarray(z)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"z must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    N, limit = config.block(rate), config.limit
    ceiling, release, rN, g_init, _ = (np.float32(v) for v in config.fparams(rate))
    words_n = config.state_words(rate)
    if state is None:
        state = fresh_state(config, rate)
    if state.dtype != torch.int32 or tuple(state.shape) != (words_n,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {words_n} words, got {tuple(state.shape)} {state.dtype}")
    words = state.clone().numpy()
    fl = words.view(np.float32)
    pos, hold = int(words[I_IN]), int(words[I_HOLD])
    if not 0 <= hold <= (2 * N - 1 if limit else 0):
        raise ValueError(f"the state holds {hold} samples, which a block of {N} does not allow")
    n = int(x.shape[0])
    if end is not None:
        if not _is_int(end) or end < pos:
            raise ValueError(f"end = {end!r} lies in front of the {pos} samples the session has taken")
        if pos + n >= end:
            n, final = end - pos, True
            x = x[:n]
    none = torch.zeros(0, dtype=torch.float32)
    if n == 0 and not final:
        return none.clone(), torch.from_numpy(words), none.clone(), none.clone()
    segs, base = live(plan(requests, config), config.initial_gain, pos)
    fresh = pos == 0
    s, node, s_min = (np.float32(1.0),) * 3 if fresh else (np.float32(fl[k]) for k in (I_S, I_NODE, I_SMIN))
    blocks, limited, clamped = (int(words[k]) for k in (I_BLOCKS, I_LIMITED, I_CLAMPED))
    peak_in, peak_out, open_peak = (np.float32(fl[k]) for k in (I_PEAK_IN, I_PEAK_OUT, I_OPEN))
    c = commanded(segs, base, pos, n)
    v = x * c
    if n:
        peak_in = max(peak_in, np.float32(np.abs(x).max()))
        fl[I_C] = c[-1]
    peaks, gains = [], []
    if not limit:
        y, new_hold = v, v[:0]
    else:
        L = np.concatenate([fl[HEADER:HEADER + hold].copy(), v])
        M = L.shape[0]
        done = M // N + (1 if final and M % N else 0)
        nodes = {0: node} if hold >= N else {}
        for j in range(1 if hold >= N else 0, done):
            p = np.float32(np.abs(L[j * N:(j + 1) * N]).max())
            t = ceiling / p if p > ceiling else np.float32(1.0)
            u = np.float32(1.0) - s
            u = release * u
            r = s + u
            sb = min(t, r)
            nodes[j], s = min(s, sb), sb
            s_min = min(s_min, sb)
            limited += int(p > ceiling)
            blocks += 1
            peaks.append(p), gains.append(sb)
        if final:
            nodes[done], leave = s, done
        else:
            leave = max(0, done - 1)
        n_out = emitted(hold, n, N, final)
        y = np.empty(n_out, dtype=np.float32)
        u = np.arange(1, N + 1, dtype=np.float32) * rN
        for j in range(leave):
            vs = L[j * N:min((j + 1) * N, M)]
            d = nodes[j + 1] - nodes[j]
            gi = nodes[j] + d * u[:vs.shape[0]]
            y[j * N:j * N + vs.shape[0]] = vs * gi
        new_hold = L[n_out:]
        node = nodes[leave] if new_hold.shape[0] >= N else s
        open_peak = np.float32(np.abs(L[done * N:]).max()) if M > done * N and not final else np.float32(0.0)
    over, under = y > ceiling, y < -ceiling
    clamped += int(over.sum()) + int(under.sum())
    y = np.where(over, ceiling, np.where(under, -ceiling, y)).astype(np.float32)
    if y.shape[0]:
        peak_out = max(peak_out, np.float32(np.abs(y).max()))
    fl[I_S], fl[I_NODE], fl[I_OPEN], fl[I_SMIN], fl[I_PEAK_IN], fl[I_PEAK_OUT] = s, node, open_peak, s_min, peak_in, peak_out
    words[I_HOLD], words[I_BLOCKS], words[I_LIMITED], words[I_CLAMPED] = new_hold.shape[0], blocks, limited, clamped
    words[I_IN], words[I_OUT] = pos + n, int(words[I_OUT]) + y.shape[0]
    if limit:
        fl[HEADER:HEADER + new_hold.shape[0]] = new_hold
        words[HEADER + new_hold.shape[0]:] = 0
    return (torch.from_numpy(y), torch.from_numpy(words), torch.from_numpy(np.array(peaks, dtype=np.float32)),
            torch.from_numpy(np.array(gains, dtype=np.float32)))


@dataclasses.dataclass(frozen=True)
class ShapeReport:
    """What a caller reads of a session's shaper, built from the header of its state row.

        samples_in, samples_out   samples of z taken, samples handed out (the difference is held: N .. 2 N - 1 with the limiter)
        gain, gain_db             the commanded gain at the last sample taken (initial_gain before the first)
        limiter, limiter_min      s of the last completed block and the smallest s so far (1.0: the limiter has not acted)
        limited_blocks, blocks    completed blocks whose peak exceeded the ceiling; completed blocks
        clamped                   samples that met the ceiling behind the limiter (rounding excess), or instead of it
        peak_in, peak_out         the largest |z| taken and the largest |y| handed out
    """
    samples_in: int
    samples_out: int
    gain: float
    gain_db: float
    limiter: float
    limiter_min: float
    limited_blocks: int
    blocks: int
    clamped: int
    peak_in: float
    peak_out: float
    block: int = 120
    rate: int = 24000


def _db(v: float) -> float:
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def report(state: torch.Tensor, block: int = 120, rate: int = 24000, initial_gain: float = 1.0) -> ShapeReport:
    """the report of a state row or of its header (any device -- one copy to the host)"""
    row = state[:HEADER].cpu()
    w, f = [int(v) for v in row.tolist()], [float(v) for v in row.view(torch.float32).tolist()]
    fresh = w[I_IN] == 0
    gain = float(np.float32(initial_gain)) if fresh else f[I_C]
    return ShapeReport(samples_in=w[I_IN], samples_out=w[I_OUT], gain=gain, gain_db=_db(gain), limiter=1.0 if fresh else f[I_S],
                       limiter_min=1.0 if fresh else f[I_SMIN], limited_blocks=w[I_LIMITED], blocks=w[I_BLOCKS], clamped=w[I_CLAMPED],
                       peak_in=f[I_PEAK_IN], peak_out=f[I_PEAK_OUT], block=int(block), rate=int(rate))


# ---------------------------------------------------------------------------------------------------- the launch
def ramp_arena(lengths, dev) -> Tuple[torch.Tensor, Dict[int, int]]:
    """the ramp tables of `lengths` back to back on `dev` -> (arena, {length: offset})"""
    off, at = {}, 0
    for n in sorted({int(n) for n in lengths if n}):
        off[n], at = at, at + n
    arena = np.concatenate([ramp_table(n) for n in off] + [np.zeros(1, np.float32)])
    return torch.from_numpy(arena).to(dev), off


def shape_items(src: Sequence[Optional[torch.Tensor]], dst: Sequence[Optional[torch.Tensor]], configs: Sequence[Optional[ShapeConfig]],
                segments: Sequence[Sequence[Segment]], base: Sequence[float], pos: Sequence[int], hold: Sequence[int],
                final: Sequence[bool], state: torch.Tensor, out_peak: torch.Tensor, out_gain: torch.Tensor, rate: int,
                ramps: Optional[torch.Tensor] = None, ramp_off: Optional[Dict[int, int]] = None,
                table: Optional[torch.Tensor] = None) -> List[int]:
    """all slots of a step in ONE launch (dmel_shape_items) -> the samples each slot's dst received.  Slot s takes the samples of
    src[s] (a 1-D fp32 CUDA tensor with contiguous samples, or None for none) as z[pos[s] ...], with the live segments
    segments[s] (absolute anchors; at most 8) over the base gain base[s], and writes emitted(hold[s], n, N, final[s]) samples to
    dst[s] (another buffer than src[s]; at least that long; None where nothing can leave).  hold[s]: the samples the slot's row holds
    (what the caller tracks from emitted()).  A slot with no samples that is not final is idle: its rows are not touched and
    configs[s] may be None.  state: (S, pitch) int32, contiguous, pitch >= configs[s].state_words(rate), updated in place;
    out_peak / out_gain: (S, pitch) fp32, contiguous, pitch >= completed(...) of every slot.  ramps, ramp_off: the arena with the
    table of every ramp length the segments use and {length: offset} (default: built here); table: int32 device scratch of
    64 * S words a caller that shapes every step keeps.  Runs on the current stream."""
    S = len(src)
    if S == 0:
        raise ValueError("no slot to shape")
    if not (len(dst) == len(configs) == len(segments) == len(base) == len(pos) == len(hold) == len(final) == S):
        raise ValueError(f"{S} slots need {S} of every per-slot argument")
    _lib.require_cuda(state, "state")
    dev = state.device
    if state.dtype != torch.int32 or state.ndim != 2 or state.shape[0] != S or not state.is_contiguous():
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, pitch) on {dev}")
    for t, name in ((out_peak, "out_peak"), (out_gain, "out_gain")):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous fp32 tensor ({S}, pitch) on {dev}")
    if out_peak.shape[1] != out_gain.shape[1]:
        raise ValueError("out_peak and out_gain must have one pitch")
    if ramp_off is None or ramps is None:
        ramps, ramp_off = ramp_arena([sg[3] for sl in segments for sg in sl], dev)
    sp, dp, cap, n_new, flags, blocks, fp, counts, words, out = [], [], [], [], [], [], [], [], [], []
    for s in range(S):
        x, d, cfg = src[s], dst[s], configs[s]
        for t, name in ((x, "src"), (d, "dst")):
            if t is not None and (t.dtype != torch.float32 or t.ndim != 1 or (t.shape[0] > 1 and t.stride(0) != 1) or t.device != dev):
                raise ValueError(f"slot {s}: {name} must be a 1-D fp32 tensor of contiguous samples on {dev}")
        n = 0 if x is None else int(x.shape[0])
        idle = n == 0 and not final[s]
        if not idle and cfg is None:
            raise ValueError(f"slot {s} takes part and has no config")
        segs = [] if idle else list(segments[s])
        if len(segs) > MAX_SEGMENTS:
            raise ValueError(f"slot {s}: {len(segs)} live segments, at most {MAX_SEGMENTS}")
        sp.append(x.data_ptr() or None if n else None)
        dp.append(d.data_ptr() or None if d is not None and d.shape[0] else None)
        cap.append(0 if d is None else int(d.shape[0]))
        n_new.append(n)
        flags.append((1 if final[s] else 0) | (2 if cfg is not None and cfg.limit else 0))
        blocks.append(cfg.block(rate) if cfg else 0)
        f = cfg.fparams(rate) if cfg else (0.0,) * FPARAMS
        fp += [f[0], f[1], f[2], float(np.float32(base[s])) if cfg else 0.0, f[4]]
        counts.append(len(segs))
        for k in range(MAX_SEGMENTS):
            if k < len(segs):
                P, g0, g1, ramp = segs[k]
                if ramp and ramp not in ramp_off:
                    raise ValueError(f"slot {s}: segment {k}: no ramp table of {ramp} samples in the arena")
                bits = np.array([g0, g1], dtype=np.float32).view(np.int32)
                start = max(int(P) - int(pos[s]), -(1 << 30))            # a ramp that began long ago has finished: any such start will do
                words += [start, int(ramp), ramp_off[ramp] if ramp else 0, int(bits[0]), int(bits[1])]
            else:
                words += [0] * SEG_WORDS
        out.append(0 if idle else emitted(hold[s], n, blocks[-1], bool(final[s]), cfg.limit))
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    P, I64, I32 = C.c_void_p * S, C.c_int64 * S, C.c_int32 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_shape_items(P(*dp), I64(*cap), P(*sp), I64(*n_new), I64(*[int(h) for h in hold]), I32(*flags),
                                               I32(*blocks), (C.c_float * (FPARAMS * S))(*fp), I32(*counts),
                                               (C.c_int32 * (SEG_WORDS * MAX_SEGMENTS * S))(*words), S, ramps.data_ptr(),
                                               int(ramps.numel()), state.data_ptr(), int(state.shape[1]), out_peak.data_ptr(),
                                               out_gain.data_ptr(), int(out_peak.shape[1]), table.data_ptr(), _lib.stream_ptr()),
                   "shape_items")
    return out
