"""The input level rule of encode sessions opened with level= (models/stream_sessions.py: EncodeSessions), on the host: the config,
the per-session state, the scan over samples, and the report a caller reads.  The pool's kernel (dmel_level_items) is held to
scan() bit for bit; only level_items(), the launch at the end, needs a GPU.

Training clips are peak-normalised to 0.95 each (dataset.peak_normalize); a live session cannot do that, because its peak lies in the
future.  This rule is what a telephony front end has in its place: a causal block AGC with a meter, on the session's samples at the
codec's rate, as f32, behind the convert, downmix and resample launches, whatever the wire was.  It adds no latency: no sample is
held back, and the samples are re-written in place.

Blocks: N = block_samples samples each (None: 10 ms, (sample_rate + 50) // 100: 240 at 24 kHz, 80 at 8 kHz; 32 <= N <= 4096),
consecutive, counted from the session's first sample at the codec's rate.  The float parameters reach the rule as fp32 values
computed once on the host: the fields as they are, emin = fp32(target_peak / max_gain) (the division in float64, rounded once) and
rN = fp32(1 / N).

Per sample x at position i (0-based) of the open block, whose start gain is ga and whose end gain is gb, each a separately rounded
fp32 operation, no fused multiply-add:

    d = gb - ga;   u = fp32(i + 1) * rN;   m = d * u;   gi = ga + m;   y = x * gi
    y >  ceiling: y =  ceiling, clamped += 1;      y < -ceiling: y = -ceiling, clamped += 1
    open_peak = max(open_peak, |x|)                (of the RAW sample)
    peak_out  = max(peak_out,  |y|)

Per completed block, in block order, p = open_peak its raw peak:

    peak_in = max(peak_in, p)
    not locked:   p >= gate: env = p, locked = 1        (acquire: the first block that is not silence sets the envelope)
    locked:       p < gate and p < env: held += 1       (hold: silence does not pump the gain up)
                  else k = (p >= env) ? attack : release;  t = p - env;  t = k * t;  env = env + t      (three rounded operations)
    g = locked ? min(max(target_peak / max(env, emin), min_gain), max_gain) : initial_gain              (the IEEE fp32 division)
    ga = gb;  gb = g;  open_peak = 0;  fill = 0;  blocks += 1
    out_peak[b] = p,  out_gain[b] = g                   (g is the gain the NEXT block ramps to)

While locked == 0, ga and gb read as initial_gain whatever the row holds, so a zeroed row is the fresh state; a call with samples
writes the values it read back (a row that has seen samples holds initial_gain in both words until it locks).

State of a session: STATE_WORDS = 16 4-byte words.

    0  env        fp32        4  peak_in    fp32         8   locked    int32
    1  ga         fp32        5  peak_out   fp32         9   held      int32
    2  gb         fp32        6  fill       int32        10  clamped   int32
    3  open_peak  fp32        7  blocks     int32        11 .. 15      reserved, kept at 0

open_peak and fill are carried, so the result cannot depend on how the stream was cut into pushes.

THE DEFAULTS ARE CHECKED ON SYNTHETIC SIGNALS ONLY (sines, noise with a burst: tests/test_level_cpu.py) and are not tuned on speech.
A loud onset after a quiet stretch is gained with the old gain for up to two blocks -- the block it arrives in and the ramp of the
next one -- and is clamped at `ceiling` meanwhile: the price of zero latency.  The clamped samples are counted in `clamped`.  The
counters are int32; nothing checks for their overflow (2^31 blocks of 10 ms are 248 days).  NaN input is outside the contract.
Not served: look-ahead limiting, RMS or loudness (LUFS) metering."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

STATE_WORDS = 16
MIN_BLOCK, MAX_BLOCK = 32, 4096
TABLE_WORDS = 16                                       # 4-byte words of table scratch per slot of dmel_level_items
PASS_SAMPLES, PASS_BLOCKS = 4096, 64                   # what one pass of the kernel's workgroup takes through LDS
I_ENV, I_GA, I_GB, I_OPEN, I_PEAK_IN, I_PEAK_OUT, I_FILL, I_BLOCKS, I_LOCKED, I_HELD, I_CLAMPED = range(11)
_FLOATS = ("target_peak", "max_gain", "min_gain", "attack", "release", "gate", "ceiling", "initial_gain")


def default_block(sample_rate: int) -> int:
    """10 ms in samples of `sample_rate`, rounded to the nearest"""
    return (int(sample_rate) + 50) // 100


def pass_blocks(block: int) -> int:
    """the blocks of `block` samples one pass of the kernel covers (a launch with more turns its pass loop again)"""
    return max(1, min(PASS_BLOCKS, PASS_SAMPLES // int(block)))


@dataclasses.dataclass(frozen=True)
class LevelConfig:
    """Plain values; see the module for what each does.  block_samples: None for 10 ms at the rate the leveller runs at.  The
    defaults are checked on synthetic signals only."""
    block_samples: Optional[int] = None
    target_peak: float = 0.5
    max_gain: float = 31.6                             # 30 dB
    min_gain: float = 0.1                              # -20 dB
    attack: float = 1.0
    release: float = 0.02
    gate: float = 0.003                                # -50 dBFS
    ceiling: float = 1.0
    initial_gain: float = 1.0

    def __post_init__(self):
        n = self.block_samples
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not MIN_BLOCK <= n <= MAX_BLOCK):
            raise ValueError(f"block_samples must be None or an integer in [{MIN_BLOCK}, {MAX_BLOCK}], got {n!r}")
        for name in _FLOATS:
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (v == 0 and name != "gate"):
                raise ValueError(f"{name} must be a finite number {'>= 0' if name == 'gate' else '> 0'}, got {v!r}")
            object.__setattr__(self, name, float(v))
        for name in ("attack", "release"):
            if getattr(self, name) > 1.0:
                raise ValueError(f"{name} must be in (0, 1], got {getattr(self, name)!r}")
        if not self.min_gain <= self.initial_gain <= self.max_gain:
            raise ValueError(f"initial_gain {self.initial_gain!r} must lie in [min_gain, max_gain] = [{self.min_gain!r}, {self.max_gain!r}]")
        f32 = np.finfo(np.float32)
        for name, v in [(k, getattr(self, k)) for k in _FLOATS] + [("target_peak / max_gain", self.target_peak / self.max_gain)]:
            if v != 0 and not float(f32.tiny) <= v <= float(f32.max):       # what the kernel compares with is the fp32 value
                raise ValueError(f"{name} = {v!r} is no normal fp32 number")

    def block(self, sample_rate: int) -> int:
        """N at `sample_rate`; ValueError where the rate or the block does not fit"""
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        n = default_block(sample_rate) if self.block_samples is None else self.block_samples
        if not MIN_BLOCK <= n <= MAX_BLOCK:
            raise ValueError(f"a block of {n} samples at {sample_rate} Hz is outside [{MIN_BLOCK}, {MAX_BLOCK}]: set block_samples")
        return n

    def fparams(self, sample_rate: int) -> Tuple[float, ...]:
        """(initial_gain, target_peak, emin, min_gain, max_gain, attack, release, gate, ceiling, rN) as the fp32 values scan and
        dmel_level_items compute with"""
        return _fparams(self, sample_rate)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "LevelConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _fparams(config: LevelConfig, sample_rate: int) -> Tuple[float, ...]:
    """a pool asks for them on every step"""
    n = config.block(sample_rate)
    return tuple(float(np.float32(v)) for v in (config.initial_gain, config.target_peak, config.target_peak / config.max_gain,
                                                config.min_gain, config.max_gain, config.attack, config.release, config.gate,
                                                config.ceiling, 1.0 / n))


def as_config(level) -> Optional[LevelConfig]:
    """what open(level=) takes: None / False -> None, True -> the defaults, a LevelConfig -> itself"""
    if level is None or level is False:
        return None
    if level is True:
        return LevelConfig()
    if isinstance(level, LevelConfig):
        return level
    raise ValueError(f"level must be None, a bool or a LevelConfig, got {type(level).__name__}")


def fresh_state() -> torch.Tensor:
    """(16,) int32 zeros: the state of a session that has seen no sample"""
    return torch.zeros(STATE_WORDS, dtype=torch.int32)


def _check_state(state: torch.Tensor) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (STATE_WORDS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {STATE_WORDS} words, got {tuple(state.shape)} {state.dtype}")


def scan(samples, config: LevelConfig, state: Optional[torch.Tensor] = None,
         sample_rate: int = 24000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """samples: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0, at `sample_rate`; state: what an earlier call
    returned (None: fresh) -> (y (n,) fp32: the levelled samples, state after the samples, block_peaks (B,) fp32, block_gains (B,)
    fp32) over the B blocks the samples completed.  Neither `samples` nor `state` is modified.  Any split of the samples gives the
    bits of one call."""
    x = samples.numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"samples must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    N = config.block(sample_rate)
    g0, target, emin, gmin, gmax, attack, release, gate, ceiling, rN = (np.float32(v) for v in config.fparams(sample_rate))
    if state is None:
        state = fresh_state()
    _check_state(state)
    words = state.clone().numpy()
    fl = words.view(np.float32)
    n = int(x.shape[0])
    y = np.empty(n, dtype=np.float32)
    if n == 0:                                                               # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(y), torch.from_numpy(words), torch.zeros(0), torch.zeros(0)
    fill, blocks, locked, held, clamped = (int(words[k]) for k in (I_FILL, I_BLOCKS, I_LOCKED, I_HELD, I_CLAMPED))
    if not 0 <= fill < N:
        raise ValueError(f"the state's open block holds {fill} samples, which is no part of a block of {N}")
    env, open_peak, peak_in, peak_out = (np.float32(fl[k]) for k in (I_ENV, I_OPEN, I_PEAK_IN, I_PEAK_OUT))
    ga, gb = (np.float32(fl[I_GA]), np.float32(fl[I_GB])) if locked else (g0, g0)
    ramp = np.arange(1, N + 1, dtype=np.float32) * rN                         # u of every position of a block
    peaks, gains = [], []
    at = 0
    while at < n:
        m = min(N - fill, n - at)
        xs = x[at:at + m]
        d = gb - ga
        gi = ga + d * ramp[fill:fill + m]                                    # numpy rounds the product, then the sum
        ys = xs * gi
        over, under = ys > ceiling, ys < -ceiling
        clamped += int(over.sum()) + int(under.sum())
        ys = np.where(over, ceiling, np.where(under, -ceiling, ys))
        y[at:at + m] = ys
        open_peak = max(open_peak, np.float32(np.abs(xs).max()))
        peak_out = max(peak_out, np.float32(np.abs(ys).max()))
        at, fill = at + m, fill + m
        if fill < N:
            break
        p = open_peak
        peak_in = max(peak_in, p)
        if not locked:
            if p >= gate:
                env, locked = p, 1
        elif p < gate and p < env:
            held += 1
        else:
            k = attack if p >= env else release
            t = p - env
            t = k * t
            env = env + t
        g = min(max(target / max(env, emin), gmin), gmax) if locked else g0
        ga, gb, open_peak, fill = gb, g, np.float32(0.0), 0
        blocks += 1
        peaks.append(p), gains.append(g)
    fl[I_ENV], fl[I_GA], fl[I_GB], fl[I_OPEN], fl[I_PEAK_IN], fl[I_PEAK_OUT] = env, ga, gb, open_peak, peak_in, peak_out
    words[I_FILL:I_CLAMPED + 1] = (fill, blocks, locked, held, clamped)
    return (torch.from_numpy(y), torch.from_numpy(words), torch.from_numpy(np.array(peaks, dtype=np.float32)),
            torch.from_numpy(np.array(gains, dtype=np.float32)))


@dataclasses.dataclass(frozen=True)
class LevelReport:
    """What a caller reads of a session's leveller, built from its state row.  Blocks are blocks of `block` samples at the codec's
    rate.

        gain, gain_db      the gain the open block ramps to (initial_gain until the leveller has locked)
        envelope, locked   the tracked input peak; whether a block at or above the gate has been seen
        peak_in            the largest raw |x| of the completed blocks;  peak_in_dbfs: 20 log10 of it (-inf for silence)
        peak_out           the largest |y| handed to the encoder, the open block's samples included
        clamped            samples that met the ceiling;  held_blocks: blocks of silence that left the envelope alone
        blocks             whole blocks seen;  total_samples: samples seen, the open block's included
    """
    gain: float
    gain_db: float
    envelope: float
    locked: bool
    peak_in: float
    peak_in_dbfs: float
    peak_out: float
    clamped: int
    held_blocks: int
    blocks: int
    total_samples: int
    block: int = 240
    sample_rate: int = 24000

    def samples(self, b: int) -> int:
        """the first sample of block b"""
        return int(b) * self.block

    def seconds(self, b: int) -> float:
        return int(b) * self.block / self.sample_rate


def _db(v: float) -> float:
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def report(state: torch.Tensor, block: int = 240, sample_rate: int = 24000, initial_gain: float = 1.0) -> LevelReport:
    """the report of a state row (any device -- one copy to the host); block: N of the session's config at its rate;
    initial_gain: the config's, which a row that has not locked reads as its gain"""
    row = state.cpu()
    w, f = [int(v) for v in row.tolist()], [float(v) for v in row.view(torch.float32).tolist()]
    locked = bool(w[I_LOCKED])
    gain = f[I_GB] if locked else float(np.float32(initial_gain))
    return LevelReport(gain=gain, gain_db=_db(gain), envelope=f[I_ENV], locked=locked, peak_in=f[I_PEAK_IN], peak_in_dbfs=_db(f[I_PEAK_IN]),
                       peak_out=f[I_PEAK_OUT], clamped=w[I_CLAMPED], held_blocks=w[I_HELD], blocks=w[I_BLOCKS],
                       total_samples=w[I_BLOCKS] * int(block) + w[I_FILL], block=int(block), sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def max_blocks(n_new: int, block: int) -> int:
    """the most blocks n_new samples can complete, whatever the open block holds: what a row of out_peak / out_gain must take"""
    return (int(n_new) + int(block) - 1) // int(block)


def level_items(samples: torch.Tensor, first: Sequence[int], n_new: Sequence[int], configs: Sequence[Optional[LevelConfig]],
                state: torch.Tensor, out_peak: torch.Tensor, out_gain: torch.Tensor, sample_rate: int = 24000,
                table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_level_items).  samples: (S, width) fp32 CUDA with contiguous columns; slot s levels
    the n_new[s] samples at columns [first[s], first[s] + n_new[s]) of its row IN PLACE (0: the slot is idle, its rows are not
    touched, configs[s] may be None); no other column is written.  state: (S, 16) int32, contiguous, updated in place; out_peak /
    out_gain: (S, pitch) fp32, contiguous, pitch >= max_blocks(n_new[s], N) for every s; the words behind the blocks a row completed
    are not written.  table: int32 device scratch of 16 * S words a caller that levels every step keeps (default: allocated here).
    Runs on the current stream."""
    _lib.require_cuda(samples, "samples")
    if samples.ndim != 2 or samples.dtype != torch.float32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be an fp32 tensor (S, width) with contiguous columns, got {tuple(samples.shape)} {samples.dtype}")
    S, width = (int(v) for v in samples.shape)
    dev = samples.device
    if len(first) != S or len(n_new) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} offsets, counts and configs, got {len(first)}, {len(n_new)} and {len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, STATE_WORDS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {STATE_WORDS}) on {dev}")
    for t, name in ((out_peak, "out_peak"), (out_gain, "out_gain")):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous fp32 tensor ({S}, pitch) on {dev}")
    if out_peak.shape[1] != out_gain.shape[1]:
        raise ValueError("out_peak and out_gain must have one pitch")
    blocks, fp = [], []
    for s in range(S):
        n, f = int(n_new[s]), int(first[s])
        if n < 0 or (n and not 0 <= f <= width - n):
            raise ValueError(f"slot {s}: columns [{f}, {f + n}) are no part of a row of {width} samples")
        if n and configs[s] is None:
            raise ValueError(f"slot {s} has {n} samples and no config")
        cfg = configs[s] if n else None
        blocks.append(cfg.block(sample_rate) if cfg else 0)
        fp += cfg.fparams(sample_rate) if cfg else (0.0,) * 10
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    I64 = C.c_int64 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_level_items(samples.data_ptr(), samples.stride(0), S, I64(*[int(v) for v in first]),
                                               I64(*[int(v) for v in n_new]), (C.c_int32 * S)(*blocks), (C.c_float * (10 * S))(*fp),
                                               state.data_ptr(), out_peak.data_ptr(), out_gain.data_ptr(), int(out_peak.shape[1]),
                                               table.data_ptr(), _lib.stream_ptr()),
                   "level_items")
