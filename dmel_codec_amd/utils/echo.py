"""The echo rule of encode sessions opened with echo= (models/stream_sessions.py: EncodeSessions), on the host: the config, the
per-session state, the scan over samples, and the report a caller reads.  The pool's kernel (dmel_echo_items) is held to scan() bit
for bit; only echo_items(), the launch at the end, needs a GPU.

What an agent says into a phone line comes back through the hybrid or the speakerphone and reaches the listening session as if the
caller had said it.  This rule is what a telephony front end puts in front of its detectors: an acoustic echo canceller, a block
NLMS adaptive FIR per session, on the session's samples at the codec's rate, as f32, behind the convert, downmix and resample
launches, whatever the wire was.  It adds no latency: no sample is held back, and the samples are re-written in place.

Precision: everything is fp32, every operation is rounded on its own (no fused multiply-add), the divisions are the IEEE ones.
The float parameters reach the rule as fp32 values computed once on the host: the fields as they are, and fN = fp32(N).

Signals, at the codec's rate:

    d[t]    the session's sample t, counted from its first codec-rate sample (the microphone, the near end)
    x[j]    the far-end stream: what the agent sends.  It has its own counter, is pushed on its own and may run ahead of d
    xd[t]   = x[t - delay_samples]; 0 where t - delay_samples < 0, and 0 where that far sample had not been pushed when sample t
            was processed: such samples are counted in far_missing and are never revisited -- a far sample that arrives after
            its turn is dropped, the later ones keep their places

One summation order for everything, sum8(v[0 .. n)): the terms in 8 contiguous segments with the boundaries floor(q n / 8), each
segment summed in ascending order starting from 0.0f, the eight sums combined as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
Eight independent chains let the kernel hide latency; here they are eight slices of one sequential accumulate.

Blocks: N = block_samples samples each, consecutive, counted from the session's first sample; the filter w[0 .. L), L = taps, is
fixed during a block.  Per sample at position i of the open block:

    yhat = sum8_k( w[k] * xd[t - k] ), k = 0 .. L - 1;      e = d - yhat;      e replaces d in place at once

Per completed block, in block order, t0 its first sample:

    E  = sum8( xd[j]^2 ) over the L + N - 1 samples j in [t0 - L + 1, t0 + N) the block read;  mx = max |xd[j]| over them
    Ed = sum8( d^2 ),  Ee = sum8( e^2 ),  md = max |d| over the block
    the block adapts iff E >= far_floor and not (double_talk > 0 and md > double_talk * mx)       (a Geigel test); else frozen += 1
    adapting:  step = mu / (fN * E + eps)                                                         (a product, a sum, a division)
               every k:  g[k] = sum8_i( e[i] * xd[t0 + i - k] ), i = 0 .. N - 1;   w[k] = w[k] + step * g[k];       adapted += 1
    sd = sd + meter * (Ed - sd);   se = se + meter * (Ee - se)                                    (three rounded operations each)
    out_in[b] = Ed,  out_res[b] = Ee;   blocks += 1

The step is normalised by N * E, not by E: N * E bounds the trace of the block's Gram matrix (every one of its N diagonal entries
is a window energy of at most E), so the update is stable for any far-end colouring with mu < 2.  Normalising by E alone diverged
on coloured far ends in a float64 prototype.  Larger N converges roughly in proportion slower, hence the default of 32.

State of a session: one row of ROW_WORDS = 68112 4-byte words.

    0  T            int32   microphone samples seen                    5  frozen       int32   completed blocks that did not adapt
    1  F            int32   far samples pushed                         6  far_missing  int32
    2  fill         int32   samples of the open block, T mod N         7  sd           fp32    meter of Ed
    3  blocks       int32   completed blocks                           8  se           fp32    meter of Ee
    4  adapted      int32   completed blocks that adapted              9 .. 15         reserved, kept at 0
    16   .. 2064    w[2048]       fp32, the taps; the words from L on are kept as they are (0 in a row the rule made)
    2064 .. 2320    e_open[256]   fp32, e of the open block's `fill` samples, 0 behind them
    2320 .. 2576    d_open[256]   fp32, d of the same samples (Ed needs them when the block completes), 0 behind them
    2576 .. 68112   far[65536]    fp32, a ring: xd's source, x[j] at word j mod 65536 -- or 0 where x[j] was missing at its turn

The first STATE_WORDS = 2576 words and the live part of the ring (far_live) are what a snapshot carries.  A zeroed row is the
fresh state.  e_open, d_open, fill and the ring are carried, so the result cannot depend on how either stream was cut into
pushes, provided the far samples are present when needed.  The ring holds the oldest sample an open block can still read
(delay_samples + L + N - 2 behind the newest microphone sample) up to MAX_AHEAD = 39232 far samples ahead of the microphone:
scan() refuses a far push beyond that, dmel_echo_items drops its surplus samples.

A call processes its far samples first, then its microphone samples: the far chunk of a step is present for the step's own samples.

THE DEFAULTS ARE CHECKED ON SYNTHETIC SIGNALS ONLY (white noise, AR(1) noise and a harmonic voiced-like signal through a random
decaying path: tests/test_echo_cpu.py) and are not tuned on speech or on lines.  No G.168 conformance is claimed.  There is no
residual echo suppressor, no comfort noise and no nonlinear processing: what the linear filter does not model stays in e.  The
Geigel test freezes on loud near-end speech only; quiet double talk disturbs the taps.  The counters are int32; nothing checks for
their overflow (2^31 samples at 24 kHz are 24.8 hours).  NaN input is outside the contract.  Not served: frequency-domain or
partitioned filters, automatic bulk-delay search, stereo far ends, far streams at another rate or format than codec-rate f32."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

HEADER_WORDS = 16
MIN_TAPS, MAX_TAPS = 64, 2048
MIN_BLOCK, MAX_BLOCK = 16, 256
MAX_DELAY = 24000
FAR_RING = 65536
O_W, O_E, O_D, O_FAR = HEADER_WORDS, HEADER_WORDS + MAX_TAPS, HEADER_WORDS + MAX_TAPS + MAX_BLOCK, HEADER_WORDS + MAX_TAPS + 2 * MAX_BLOCK
STATE_WORDS = O_FAR                                    # 2576: header, taps, the open block
ROW_WORDS = O_FAR + FAR_RING                           # 68112
MAX_AHEAD = FAR_RING - MAX_DELAY - MAX_TAPS - MAX_BLOCK                # 39232: far samples ahead of the microphone the ring takes
TABLE_WORDS = 16                                       # 4-byte words of table scratch per slot of dmel_echo_items
PASS_SAMPLES = 2048                                    # what one pass of the kernel's workgroup takes through LDS: 2048 // N blocks
I_T, I_F, I_FILL, I_BLOCKS, I_ADAPTED, I_FROZEN, I_MISSING, I_SD, I_SE = range(9)
_MASK = FAR_RING - 1


@dataclasses.dataclass(frozen=True)
class EchoConfig:
    """Plain values; see the module for what each does.  The defaults are checked on synthetic signals only."""
    taps: int = 1024                                   # L: a multiple of 64 in [64, 2048]; 1024 are 43 ms at 24 kHz
    block_samples: int = 32                            # N: a multiple of 8 in [16, 256]
    delay_samples: int = 0                             # the bulk delay of the echo path the taps need not span, 0 .. 24000
    mu: float = 1.0                                    # in (0, 2)
    eps: float = 1e-6
    far_floor: float = 1e-3                            # window energy below which a block does not adapt
    double_talk: float = 0.5                           # Geigel threshold; 0 disables the test
    meter: float = 0.05                                # in (0, 1]

    def __post_init__(self):
        for name, lo, hi, mult in (("taps", MIN_TAPS, MAX_TAPS, 64), ("block_samples", MIN_BLOCK, MAX_BLOCK, 8),
                                   ("delay_samples", 0, MAX_DELAY, 1)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi or v % mult:
                raise ValueError(f"{name} must be an integer in [{lo}, {hi}]" + (f", a multiple of {mult}" if mult > 1 else "") + f", got {v!r}")
        f32 = np.finfo(np.float32)
        for name in ("mu", "eps", "far_floor", "double_talk", "meter"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
            if v != 0 and not float(f32.tiny) <= v <= float(f32.max):       # what the kernel computes with is the fp32 value
                raise ValueError(f"{name} = {v!r} is no normal fp32 number")
            object.__setattr__(self, name, float(v))
        if not 0.0 < self.mu < 2.0:
            raise ValueError(f"mu must be in (0, 2), got {self.mu!r}")
        if not self.eps > 0.0:
            raise ValueError(f"eps must be > 0, got {self.eps!r}")
        if not 0.0 < self.meter <= 1.0:
            raise ValueError(f"meter must be in (0, 1], got {self.meter!r}")

    def fparams(self) -> Tuple[float, ...]:
        """(mu, eps, far_floor, double_talk, meter, fN) as the fp32 values scan and dmel_echo_items compute with"""
        return _fparams(self)

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "EchoConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _fparams(config: EchoConfig) -> Tuple[float, ...]:
    """a pool asks for them on every step"""
    return tuple(float(np.float32(v)) for v in (config.mu, config.eps, config.far_floor, config.double_talk, config.meter,
                                                config.block_samples))


def as_config(echo) -> Optional[EchoConfig]:
    """what open(echo=) takes: None / False -> None, True -> the defaults, an EchoConfig -> itself"""
    if echo is None or echo is False:
        return None
    if echo is True:
        return EchoConfig()
    if isinstance(echo, EchoConfig):
        return echo
    raise ValueError(f"echo must be None, a bool or an EchoConfig, got {type(echo).__name__}")


def fresh_state() -> torch.Tensor:
    """(68112,) int32 zeros: the state of a session that has seen no sample of either stream"""
    return torch.zeros(ROW_WORDS, dtype=torch.int32)


def _check_state(state: torch.Tensor) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (ROW_WORDS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {ROW_WORDS} words, got {tuple(state.shape)} {state.dtype}")


# ------------------------------------------------------------------------------------------------ the summation order
def _seq(v: np.ndarray) -> np.ndarray:
    """the last axis summed in ascending order in fp32, starting from 0.0f"""
    z = np.zeros(v.shape[:-1] + (1,), dtype=np.float32)
    return np.add.accumulate(np.concatenate((z, v), axis=-1), axis=-1, dtype=np.float32)[..., -1]


def _tree(s: np.ndarray) -> np.ndarray:
    """(..., 8) -> ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))"""
    return ((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))


def sum8(v) -> np.float32:
    """sum8 of a 1-D fp32 array of any length (the module has the order)"""
    v = np.asarray(v, dtype=np.float32)
    n = int(v.shape[0])
    return np.float32(_tree(np.stack([_seq(v[q * n // 8:(q + 1) * n // 8]) for q in range(8)])))


def _sum8_even(v: np.ndarray) -> np.ndarray:
    """sum8 along the last axis, whose length is a multiple of 8: the segments are the rows of a reshape"""
    return _tree(_seq(v.reshape(v.shape[:-1] + (8, v.shape[-1] // 8))))


def _host(a, name: str) -> np.ndarray:
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a if a is not None else np.zeros(0, dtype=np.float32))
    if a.ndim != 1 or a.dtype != np.float32:
        raise ValueError(f"{name} must be a 1-D fp32 array on the host, got {a.shape} {a.dtype}")
    return a


def scan(mic, far, config: EchoConfig, state: Optional[torch.Tensor] = None,
         far_pushed_before: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One step of a session: the far chunk, then the microphone chunk.  mic: (n,) fp32 on the host (a numpy array or a CPU
    tensor), n >= 0; far: (m,) fp32 likewise, m >= 0, or None, the far samples pushed with this step, appended behind the ones
    the state has; state: what an earlier call returned (None: fresh); far_pushed_before: the caller's own count of the far samples
    pushed so far, checked against the state's (None: not checked) -> (e (n,) fp32: the cancelled samples, state after the step,
    block_in (B,) fp32: Ed, block_res (B,) fp32: Ee) over the B blocks the samples completed.  No argument is modified.  Any split
    of either stream gives the bits of one call, provided every far sample is pushed no later than the microphone sample that
    needs it.  ValueError where the far stream would run more than MAX_AHEAD samples ahead of the microphone."""
    d, x = _host(mic, "mic"), _host(far, "far")
    L, N, delay = config.taps, config.block_samples, config.delay_samples
    mu, eps, far_floor, dt, meter, fN = (np.float32(v) for v in config.fparams())
    if state is None:
        state = fresh_state()
    _check_state(state)
    words = state.clone().numpy()
    fl = words.view(np.float32)
    T, F, fill, blocks, adapted, frozen, missing = (int(words[k]) for k in (I_T, I_F, I_FILL, I_BLOCKS, I_ADAPTED, I_FROZEN, I_MISSING))
    if far_pushed_before is not None and int(far_pushed_before) != F:
        raise ValueError(f"the state has {F} far samples, the caller counts {far_pushed_before}")
    if not 0 <= fill < N:
        raise ValueError(f"the state's open block holds {fill} samples, which is no part of a block of {N}")
    n, m = int(d.shape[0]), int(x.shape[0])
    if F + m - T > MAX_AHEAD:
        raise ValueError(f"{F + m} far samples against {T} microphone samples: more than {MAX_AHEAD} ahead")
    e = np.empty(n, dtype=np.float32)
    if n == 0 and m == 0:                                                    # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(e), torch.from_numpy(words), torch.zeros(0), torch.zeros(0)
    ring = fl[O_FAR:]
    j = F + np.arange(m, dtype=np.int64)
    keep = j >= T - delay                                                    # a far sample behind its turn is dropped: its word is the 0 of its turn
    ring[j[keep] & _MASK] = x[keep]
    F += m
    j = T + np.arange(n, dtype=np.int64) - delay
    late = j >= F                                                            # not pushed at its turn: 0, counted, never revisited
    ring[j[late] & _MASK] = 0.0
    missing += int(late.sum())
    if n == 0:
        words[I_F] = F
        return torch.from_numpy(e), torch.from_numpy(words), torch.zeros(0), torch.zeros(0)
    sd, se = np.float32(fl[I_SD]), np.float32(fl[I_SE])
    w = fl[O_W:O_W + L].copy()
    e_blk, d_blk = fl[O_E:O_E + N].copy(), fl[O_D:O_D + N].copy()
    ins, res = [], []
    at = 0
    while at < n:
        k = min(N - fill, n - at)
        t0 = T - fill                                                        # the open block's first sample
        jw = t0 - delay - (L - 1) + np.arange(L + N - 1, dtype=np.int64)     # the far window of the block: xw[q] = xd[t0 - (L - 1) + q]
        xw = np.where(jw >= 0, ring[jw & _MASK], np.float32(0.0)).astype(np.float32)
        X = np.lib.stride_tricks.sliding_window_view(xw[::-1], L)[::-1]      # X[i, k] = xw[L - 1 + i - k] = xd[t0 + i - k]
        ds = d[at:at + k]
        yhat = _sum8_even(w[None, :] * X[fill:fill + k])
        es = ds - yhat
        e[at:at + k] = es
        e_blk[fill:fill + k], d_blk[fill:fill + k] = es, ds
        at, fill, T = at + k, fill + k, T + k
        if fill < N:
            break
        E, mx = sum8(xw * xw), np.float32(np.abs(xw).max())
        Ed, Ee, md = _sum8_even(d_blk * d_blk), _sum8_even(e_blk * e_blk), np.float32(np.abs(d_blk).max())
        if E >= far_floor and not (dt > 0 and md > dt * mx):
            t = fN * E
            t = t + eps
            step = mu / t
            g = _sum8_even(e_blk[None, :] * X.T)
            w = w + step * g
            adapted += 1
        else:
            frozen += 1
        t = Ed - sd
        t = meter * t
        sd = sd + t
        t = Ee - se
        t = meter * t
        se = se + t
        ins.append(Ed), res.append(Ee)
        blocks, fill = blocks + 1, 0
    fl[O_W:O_W + L] = w
    fl[O_E:O_E + MAX_BLOCK], fl[O_D:O_D + MAX_BLOCK] = 0.0, 0.0
    fl[O_E:O_E + fill], fl[O_D:O_D + fill] = e_blk[:fill], d_blk[:fill]
    fl[I_SD], fl[I_SE] = sd, se
    words[I_T:I_MISSING + 1] = (T, F, fill, blocks, adapted, frozen, missing)
    return (torch.from_numpy(e), torch.from_numpy(words), torch.from_numpy(np.array(ins, dtype=np.float32)),
            torch.from_numpy(np.array(res, dtype=np.float32)))


def far_live(config: EchoConfig, mic_samples: int, far_pushed: int) -> Tuple[int, int]:
    """[lo, hi): the far samples x[j] a session that has seen `mic_samples` and was pushed `far_pushed` can still read -- from the
    oldest one its open block's window holds to the newest one pushed or zeroed.  What a snapshot carries of the ring."""
    T, F = int(mic_samples), int(far_pushed)
    lo = max(0, T - T % config.block_samples - config.delay_samples - (config.taps - 1))
    return lo, max(lo, F, T - config.delay_samples)


def ring_pieces(lo: int, hi: int) -> List[Tuple[int, int]]:
    """the two runs of ring words (first word, words) that hold x[lo .. hi), the second one from word 0 (either may be empty)"""
    a = lo & _MASK
    n0 = min(hi - lo, FAR_RING - a)
    return [(a, n0), (0, hi - lo - n0)]


@dataclasses.dataclass(frozen=True)
class EchoReport:
    """What a caller reads of a session's canceller, built from the header of its state row.  Blocks are blocks of `block`
    samples at the codec's rate.

        erle_db            10 log10(sd / se): the metered echo return loss enhancement; +inf where nothing is left, nan before
                           the first block or on silence
        adapted_blocks     completed blocks that moved the taps;  frozen_blocks: those that did not (far end too quiet, or the
                           Geigel test saw the near end);  blocks: both
        far_missing        microphone samples whose far sample had not been pushed at their turn (read as 0)
        far_ahead          far samples pushed beyond the microphone samples seen
        total_samples      microphone samples seen, the open block's included;  far_samples: far samples pushed
    """
    erle_db: float
    adapted_blocks: int
    frozen_blocks: int
    blocks: int
    far_missing: int
    far_ahead: int
    total_samples: int
    far_samples: int = 0
    input_energy: float = 0.0
    residual_energy: float = 0.0
    block: int = 32
    sample_rate: int = 24000


def _erle(sd: float, se: float) -> float:
    if not sd > 0:
        return math.nan if not se > 0 else -math.inf
    return math.inf if not se > 0 else 10.0 * math.log10(sd / se)


def report(state: torch.Tensor, block: int = 32, sample_rate: int = 24000) -> EchoReport:
    """the report of a state row, or of its first 16 words (any device -- one copy to the host); block: N of the session's config"""
    row = state[:HEADER_WORDS].cpu()
    w, f = [int(v) for v in row.tolist()], [float(v) for v in row.view(torch.float32).tolist()]
    return EchoReport(erle_db=_erle(f[I_SD], f[I_SE]), adapted_blocks=w[I_ADAPTED], frozen_blocks=w[I_FROZEN], blocks=w[I_BLOCKS],
                      far_missing=w[I_MISSING], far_ahead=max(0, w[I_F] - w[I_T]), total_samples=w[I_T], far_samples=w[I_F],
                      input_energy=f[I_SD], residual_energy=f[I_SE], block=int(block), sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def max_blocks(n_new: int, block: int) -> int:
    """the most blocks n_new samples can complete, whatever the open block holds: what a row of out_in / out_res must take"""
    return (int(n_new) + int(block) - 1) // int(block)


def echo_items(samples: torch.Tensor, first: Sequence[int], n_new: Sequence[int], far: Sequence[Optional[torch.Tensor]],
               configs: Sequence[Optional[EchoConfig]], state: torch.Tensor, out_in: torch.Tensor, out_res: torch.Tensor,
               table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_echo_items).  samples: (S, width) fp32 CUDA with contiguous columns; slot s first
    appends far[s] -- a contiguous (m,) fp32 tensor on the same device, or None -- to its far history, then cancels the n_new[s]
    samples at columns [first[s], first[s] + n_new[s]) of its row IN PLACE; no other column is written.  A slot with neither far
    nor new samples is idle: its rows are not touched, configs[s] may be None.  state: (S, 68112) int32, contiguous, updated in
    place; out_in / out_res: (S, pitch) fp32, contiguous, pitch >= max_blocks(n_new[s], N) for every s; the words behind the blocks
    a row completed are not written.  table: int32 device scratch of 16 * S words a caller that cancels every step keeps (default:
    allocated here).  The caller keeps far within MAX_AHEAD samples ahead of the slot's microphone samples (the kernel drops the
    surplus).  Runs on the current stream."""
    _lib.require_cuda(samples, "samples")
    if samples.ndim != 2 or samples.dtype != torch.float32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be an fp32 tensor (S, width) with contiguous columns, got {tuple(samples.shape)} {samples.dtype}")
    S, width = (int(v) for v in samples.shape)
    dev = samples.device
    if len(first) != S or len(n_new) != S or len(far) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} offsets, counts, far chunks and configs, got {len(first)}, {len(n_new)}, {len(far)} and "
                         f"{len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, ROW_WORDS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {ROW_WORDS}) on {dev}")
    for t, name in ((out_in, "out_in"), (out_res, "out_res")):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous fp32 tensor ({S}, pitch) on {dev}")
    if out_in.shape[1] != out_res.shape[1]:
        raise ValueError("out_in and out_res must have one pitch")
    ip, fp, fptr, fn = [], [], [], []
    for s in range(S):
        n, f, x = int(n_new[s]), int(first[s]), far[s]
        if n < 0 or (n and not 0 <= f <= width - n):
            raise ValueError(f"slot {s}: columns [{f}, {f + n}) are no part of a row of {width} samples")
        if x is not None and (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim != 1 or not x.is_contiguous()
                              or x.device != dev):
            raise ValueError(f"slot {s}: far must be a contiguous 1-D fp32 tensor on {dev}")
        m = 0 if x is None else int(x.shape[0])
        if (n or m) and configs[s] is None:
            raise ValueError(f"slot {s} has {n} samples and {m} far samples and no config")
        cfg = configs[s] if n or m else None
        ip += (cfg.taps, cfg.block_samples, cfg.delay_samples) if cfg else (0, 0, 0)
        fp += cfg.fparams() if cfg else (0.0,) * 6
        fptr.append(x.data_ptr() if m else None)
        fn.append(m)
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    I64 = C.c_int64 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_echo_items(samples.data_ptr(), samples.stride(0), S, I64(*[int(v) for v in first]),
                                              I64(*[int(v) for v in n_new]), (C.c_void_p * S)(*fptr), I64(*fn),
                                              (C.c_int32 * (3 * S))(*ip), (C.c_float * (6 * S))(*fp), state.data_ptr(), ROW_WORDS,
                                              out_in.data_ptr(), out_res.data_ptr(), int(out_in.shape[1]), table.data_ptr(),
                                              _lib.stream_ptr()),
                   "echo_items")
