"""The DTMF (touch-tone key) rule of encode sessions opened with dtmf= (models/stream_sessions.py: EncodeSessions), on the host: the
config, the per-session state, the scan over samples, and the report a caller reads.  The pool's kernel (dmel_dtmf_items) is held
to scan() bit for bit; only dtmf_items(), the launch at the end, needs a GPU.

The detector reads what every step leaves on the device anyway: the session's samples at the codec's rate, as f32, behind the
convert, downmix and resample launches, whatever the wire was.  A key is a pair of tones, one of the rows 697, 770, 852, 941 Hz and
one of the columns 1209, 1336, 1477, 1633 Hz; key k = 4 * row + col is KEYS[k] of "123A456B789C*0#D".  Filter k of the bank of
eight is row k for k < 4 and column k - 4 else.

Blocks: N = block_samples samples each (None: (sample_rate * 128 + 5000) // 10000, 12.8 ms: 307 at 24 kHz, 102 at 8 kHz, 564 at
44.1 kHz; 32 <= N <= 4096), consecutive, not overlapping, rectangular, counted from the session's first sample at the codec's rate.
A partial last block is never decided.  With hits = misses = 2 a tone or a pause of 40 ms (the minimum of ITU-T Q.24) spans two
whole blocks wherever it starts.

Per block and filter k, over the block's samples x in sample order, from s1 = s2 = 0 (Goertzel):

    p = c_k * s1;  q = p - s2;  s0 = x + q           (three fp32 operations, each rounded -- no fused multiply-add)
    s2 = s1;  s1 = s0
    c_k = fp32(2 cos(2 pi f_k / sample_rate)), computed in float64 on the host and passed in: the kernel evaluates no cosine

    block power   P_k = (s1 * s1 + s2 * s2) - c_k * (s1 * s2)      (each product, the sum and the difference rounded separately)
    block energy  E: e = e + x * x in sample order, from e = 0      (one rounded multiply and one rounded add per sample)

Decision of a whole block: r = argmax of P_0 .. P_3, c = argmax of P_4 .. P_7, the lowest index on a tie.  The block decides key
4 r + c where all of these hold, each evaluated in fp32 exactly as written (Pr = P_r, Pc = P_(4 + c)):

    1. E > emin,  emin = fp32(min_mean_square * N)
    2. Pr > rel * P_j for the other three rows j, Pc > rel * P_j for the other three columns    (an fp32 multiply, then a compare)
    3. Pc <= max_col_over_row * Pr  and  Pr <= max_row_over_col * Pc                             (the twist limits)
    4. (Pr + Pc) > g * E,  g = fp32(purity * N / 2)                                               (a clean pair gives about N / 2 * E)

Otherwise it decides nothing.  Keys are stored as key + 1, 0 meaning none, here and in every output.

State machine, per decided block in block order, d its decision and b = blocks its index:

    no key down:   d == 0: candidate = 0, run = 0;   d == candidate: run += 1;   else candidate = d, run = 1
                   candidate != 0 and run >= hits:   down = candidate, miss_run = 0, the event (down, start_block = b - run + 1,
                                                     end_block = -1) is written to ring[events % 32], events += 1
    a key down:    d == down: miss_run = 0;   else miss_run += 1, and at miss_run >= misses: the newest event's end_block =
                                                     b - miss_run + 1, down = candidate = run = miss_run = 0
    blocks += 1;   decided[b] = d, pressed[b] = down (the state AFTER the block), uint8 both

State of a session: STATE_WORDS = 128 4-byte words; a zeroed row is the fresh state.

    0 .. 7     s1 of the eight filters in the open (partial) block, fp32        17  fill: samples of the open block consumed, < N
    8 .. 15    s2 of the eight filters, fp32                                    18  blocks decided since the session opened
    16         e, the energy of the open block, fp32                            19  down (key + 1)       20  candidate (key + 1)
    24 .. 31   reserved, kept at 0                                              21  run   22  miss_run   23  events, since open
    32 .. 127  the ring of the last 32 events, three words each: key + 1, start_block, end_block (-1 while the key is down);
               event number i lies at ring[i % 32]

When a block completes, words 0 .. 16 return to 0 (fill == 0 goes with a zeroed carry).  Because the open block's filter state is
carried, no sample has to be kept, and the result cannot depend on how the stream was cut into pushes.

THE DEFAULTS ARE CHECKED ON SYNTHETIC SIGNALS ONLY (tone pairs with twist and white noise, harmonic buzz, single tones:
tests/test_dtmf_cpu.py).  No conformance to ITU-T Q.24 is claimed, talk-off on real speech is unmeasured, and a deployment should
tune on its own lines.  The block counter is an int32: 2^31 blocks of 12.8 ms are 318 days; nothing checks for the overflow.  NaN
input is outside the contract."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

ROWS_HZ = (697.0, 770.0, 852.0, 941.0)
COLS_HZ = (1209.0, 1336.0, 1477.0, 1633.0)
KEYS = "123A456B789C*0#D"
STATE_WORDS = 128
RING = 32                                              # events kept
MIN_BLOCK, MAX_BLOCK = 32, 4096
MAX_RUN = 1 << 20                                      # hits and misses
TABLE_WORDS = 20                                       # 4-byte words of table scratch per slot of dmel_dtmf_items
I_S1, I_S2, I_E, I_FILL, I_BLOCKS, I_DOWN, I_CAND, I_RUN, I_MISS, I_EVENTS, I_RING = 0, 8, 16, 17, 18, 19, 20, 21, 22, 23, 32


def default_block(sample_rate: int) -> int:
    """12.8 ms in samples of `sample_rate`, rounded to the nearest"""
    return (int(sample_rate) * 128 + 5000) // 10000


@dataclasses.dataclass(frozen=True)
class DtmfConfig:
    """Plain values; see the module for what each does.  block_samples: None for 12.8 ms at the rate the detector runs at.  The
    defaults are checked on synthetic signals only."""
    block_samples: Optional[int] = None
    min_mean_square: float = 1e-6
    rel: float = 6.0
    max_col_over_row: float = 2.51                     # 4 dB
    max_row_over_col: float = 6.31                     # 8 dB
    purity: float = 0.5
    hits: int = 2
    misses: int = 2

    def __post_init__(self):
        n = self.block_samples
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not MIN_BLOCK <= n <= MAX_BLOCK):
            raise ValueError(f"block_samples must be None or an integer in [{MIN_BLOCK}, {MAX_BLOCK}], got {n!r}")
        for name in ("min_mean_square", "rel", "max_col_over_row", "max_row_over_col", "purity"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
            object.__setattr__(self, name, float(v))
        for name in ("hits", "misses"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_RUN:
                raise ValueError(f"{name} must be an integer in [1, {MAX_RUN}], got {v!r}")

    def block(self, sample_rate: int) -> int:
        """N at `sample_rate`; ValueError where the rate or the block does not fit"""
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
            raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
        if 2 * max(COLS_HZ) >= sample_rate:
            raise ValueError(f"a sample rate of {sample_rate} Hz does not carry the {max(COLS_HZ):.0f} Hz column")
        n = default_block(sample_rate) if self.block_samples is None else self.block_samples
        if not MIN_BLOCK <= n <= MAX_BLOCK:
            raise ValueError(f"a block of {n} samples at {sample_rate} Hz is outside [{MIN_BLOCK}, {MAX_BLOCK}]: set block_samples")
        return n

    def coefficients(self, sample_rate: int) -> Tuple[float, ...]:
        """c_k = fp32(2 cos(2 pi f_k / sample_rate)) of the eight filters, rows first"""
        return _tables(self, sample_rate)[0]

    def fparams(self, sample_rate: int) -> Tuple[float, ...]:
        """(emin, rel, max_col_over_row, max_row_over_col, g) as the fp32 values scan and dmel_dtmf_items compare with"""
        return _tables(self, sample_rate)[1]

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "DtmfConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _tables(config: DtmfConfig, sample_rate: int) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    """(coefficients, fparams) of a config at a rate: a pool asks for them on every step"""
    n = config.block(sample_rate)
    coef = tuple(float(np.float32(2.0 * math.cos(2.0 * math.pi * f / sample_rate))) for f in ROWS_HZ + COLS_HZ)
    return coef, tuple(float(np.float32(v)) for v in (config.min_mean_square * n, config.rel, config.max_col_over_row,
                                                      config.max_row_over_col, config.purity * n / 2))


def as_config(dtmf) -> Optional[DtmfConfig]:
    """what open(dtmf=) takes: None / False -> None, True -> the defaults, a DtmfConfig -> itself"""
    if dtmf is None or dtmf is False:
        return None
    if dtmf is True:
        return DtmfConfig()
    if isinstance(dtmf, DtmfConfig):
        return dtmf
    raise ValueError(f"dtmf must be None, a bool or a DtmfConfig, got {type(dtmf).__name__}")


def fresh_state() -> torch.Tensor:
    """(128,) int32 zeros: the state of a session that has seen no sample"""
    return torch.zeros(STATE_WORDS, dtype=torch.int32)


def _check_state(state: torch.Tensor) -> None:
    if state.dtype != torch.int32 or tuple(state.shape) != (STATE_WORDS,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {STATE_WORDS} words, got {tuple(state.shape)} {state.dtype}")


def _decide(P: np.ndarray, E: np.float32, emin, rel, mcr, mrc, g) -> int:
    """the decision of one whole block: key + 1, or 0.  P: (8,) fp32 powers; every product and sum is one fp32 operation"""
    r, c = int(np.argmax(P[:4])), int(np.argmax(P[4:]))
    Pr, Pc = P[r], P[4 + c]
    ok = bool(E > emin)
    for j in range(4):
        if j != r:
            ok = ok and bool(Pr > rel * P[j])
        if j != c:
            ok = ok and bool(Pc > rel * P[4 + j])
    ok = ok and bool(Pc <= mcr * Pr) and bool(Pr <= mrc * Pc)
    ok = ok and bool((Pr + Pc) > g * E)
    return 4 * r + c + 1 if ok else 0


def scan(samples, config: DtmfConfig, state: Optional[torch.Tensor] = None,
         sample_rate: int = 24000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """samples: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0, at `sample_rate`; state: what an earlier call
    returned (None: fresh) -> (state after the samples, decided (B,) uint8, pressed (B,) uint8) over the B blocks the samples
    completed.  `state` is not modified.  Any split of the samples gives the bits of one call."""
    x = samples.numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"samples must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    N = config.block(sample_rate)
    coef = np.array(config.coefficients(sample_rate), dtype=np.float32)
    emin, rel, mcr, mrc, g = (np.float32(v) for v in config.fparams(sample_rate))
    if state is None:
        state = fresh_state()
    _check_state(state)
    words = state.clone().numpy()
    n = int(x.shape[0])
    if n == 0:                                                               # as an idle slot of the launch: the row is not touched
        return torch.from_numpy(words), torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8)
    fill = int(words[I_FILL])
    if not 0 <= fill < N:
        raise ValueError(f"the state's open block holds {fill} samples, which is no part of a block of {N}")
    # the blocks side by side: block j of this call holds positions [j N, (j + 1) N) of the stream that began `fill` samples ago
    nblk, done = -(-(fill + n) // N), (fill + n) // N
    grid = np.zeros(nblk * N, dtype=np.float32)
    grid[fill:fill + n] = x
    grid = grid.reshape(nblk, N)
    live = np.zeros(nblk * N, dtype=bool)
    live[fill:fill + n] = True
    live = live.reshape(nblk, N)
    s1, s2, e = np.zeros((nblk, 8), np.float32), np.zeros((nblk, 8), np.float32), np.zeros(nblk, np.float32)
    s1[0], s2[0], e[0] = words[I_S1:I_S1 + 8].view(np.float32), words[I_S2:I_S2 + 8].view(np.float32), words[I_E:I_E + 1].view(np.float32)[0]
    lo = 0 if nblk > 1 else fill
    hi = N if nblk > 1 else fill + n
    for i in range(lo, hi):                                                  # sample order inside every block
        on, xi = live[:, i], grid[:, i]
        p = coef[None, :] * s1
        q = p - s2
        s0 = xi[:, None] + q                                                 # three fp32 operations, each rounded
        s2 = np.where(on[:, None], s1, s2)
        s1 = np.where(on[:, None], s0, s1)
        sq = xi * xi
        e = np.where(on, e + sq, e)
    a, b, m = s1 * s1, s2 * s2, s1 * s2
    P = (a + b) - coef[None, :] * m
    blocks, down, cand, run, miss, events = (int(words[k]) for k in (I_BLOCKS, I_DOWN, I_CAND, I_RUN, I_MISS, I_EVENTS))
    hits, misses = config.hits, config.misses
    decided, pressed = np.zeros(done, dtype=np.uint8), np.zeros(done, dtype=np.uint8)
    for j in range(done):
        d = _decide(P[j], e[j], emin, rel, mcr, mrc, g)
        if down == 0:
            if d == 0:
                cand, run = 0, 0
            elif d == cand:
                run += 1
            else:
                cand, run = d, 1
            if cand and run >= hits:
                down, miss = cand, 0
                at = I_RING + 3 * (events % RING)
                words[at:at + 3] = (down, blocks - run + 1, -1)
                events += 1
        elif d == down:
            miss = 0
        else:
            miss += 1
            if miss >= misses:
                words[I_RING + 3 * ((events - 1) % RING) + 2] = blocks - miss + 1
                down = cand = run = miss = 0
        blocks += 1
        decided[j], pressed[j] = d, down
    fill = (fill + n) % N
    words[:I_FILL] = 0
    if fill:                                                                 # the open block's carry
        words[I_S1:I_S1 + 8], words[I_S2:I_S2 + 8] = s1[-1].view(np.int32), s2[-1].view(np.int32)
        words[I_E] = e[-1:].view(np.int32)[0]
    words[I_FILL:I_EVENTS + 1] = (fill, blocks, down, cand, run, miss, events)
    return torch.from_numpy(words), torch.from_numpy(decided), torch.from_numpy(pressed)


@dataclasses.dataclass(frozen=True)
class DtmfReport:
    """What a caller reads of a session's detector, built from its state row.  Samples are samples at the codec's rate.

        digits     the keys of the retained events (the last 32), in order
        events     (index since open, key, start_sample, end_sample | None while the key is down) of each retained event
        total      events since the session opened
        down       the key held now, or None
        blocks     whole blocks decided;  samples: samples seen, the open block's included
    """
    digits: str
    events: Tuple[Tuple[int, str, int, Optional[int]], ...]
    total: int
    down: Optional[str]
    blocks: int
    samples: int
    block: int = 307
    sample_rate: int = 24000

    def seconds(self, sample: int) -> float:
        return int(sample) / self.sample_rate


def report(state: torch.Tensor, block: int = 307, sample_rate: int = 24000) -> DtmfReport:
    """the report of a state row (any device -- one copy to the host); block: N of the session's config at its rate"""
    w = [int(v) for v in state.tolist()]
    total, events = w[I_EVENTS], []
    for i in range(max(0, total - RING), total):
        key, start, end = w[I_RING + 3 * (i % RING):I_RING + 3 * (i % RING) + 3]
        events.append((i, KEYS[key - 1], start * block, None if end < 0 else end * block))
    return DtmfReport(digits="".join(ev[1] for ev in events), events=tuple(events), total=total,
                      down=KEYS[w[I_DOWN] - 1] if w[I_DOWN] else None, blocks=w[I_BLOCKS], samples=w[I_BLOCKS] * block + w[I_FILL],
                      block=int(block), sample_rate=int(sample_rate))


# ---------------------------------------------------------------------------------------------------- the launch
def max_blocks(n_new: int, block: int) -> int:
    """the most blocks n_new samples can complete, whatever the open block holds: what a row of decided / pressed must take"""
    return (int(n_new) + int(block) - 1) // int(block)


def dtmf_items(samples: torch.Tensor, first: Sequence[int], n_new: Sequence[int], configs: Sequence[Optional[DtmfConfig]],
               state: torch.Tensor, decided: torch.Tensor, pressed: torch.Tensor, sample_rate: int = 24000,
               table: Optional[torch.Tensor] = None) -> None:
    """all slots of a step in ONE launch (dmel_dtmf_items).  samples: (S, width) fp32 CUDA with contiguous columns; slot s scans
    the n_new[s] samples at columns [first[s], first[s] + n_new[s]) of its row (0: the slot is idle, its rows are not touched,
    configs[s] may be None); state: (S, 128) int32, contiguous, updated in place; decided / pressed: (S, pitch) uint8,
    contiguous, pitch >= max_blocks(n_new[s], N) for every s; the bytes behind the blocks a row completed are not written.  table:
    int32 device scratch of 20 * S words a caller that scans every step keeps (default: allocated here).  Runs on the current
    stream."""
    _lib.require_cuda(samples, "samples")
    if samples.ndim != 2 or samples.dtype != torch.float32 or (samples.shape[1] > 1 and samples.stride(1) != 1):
        raise ValueError(f"samples must be an fp32 tensor (S, width) with contiguous columns, got {tuple(samples.shape)} {samples.dtype}")
    S, width = (int(v) for v in samples.shape)
    dev = samples.device
    if len(first) != S or len(n_new) != S or len(configs) != S:
        raise ValueError(f"{S} slots need {S} offsets, counts and configs, got {len(first)}, {len(n_new)} and {len(configs)}")
    if state.dtype != torch.int32 or tuple(state.shape) != (S, STATE_WORDS) or not state.is_contiguous() or state.device != dev:
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, {STATE_WORDS}) on {dev}")
    for t, name in ((decided, "decided"), (pressed, "pressed")):
        if t.dtype != torch.uint8 or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous uint8 tensor ({S}, pitch) on {dev}")
    if decided.shape[1] != pressed.shape[1]:
        raise ValueError("decided and pressed must have one pitch")
    blocks, coef, fp, ip = [], [], [], []
    for s in range(S):
        n, f = int(n_new[s]), int(first[s])
        if n < 0 or (n and not 0 <= f <= width - n):
            raise ValueError(f"slot {s}: columns [{f}, {f + n}) are no part of a row of {width} samples")
        if n and configs[s] is None:
            raise ValueError(f"slot {s} has {n} samples and no config")
        cfg = configs[s] if n else None
        blocks.append(cfg.block(sample_rate) if cfg else 0)
        coef += cfg.coefficients(sample_rate) if cfg else (0.0,) * 8
        fp += cfg.fparams(sample_rate) if cfg else (0.0,) * 5
        ip += (cfg.hits, cfg.misses) if cfg else (0, 0)
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    I64 = C.c_int64 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_dtmf_items(samples.data_ptr(), samples.stride(0), S, I64(*[int(v) for v in first]),
                                              I64(*[int(v) for v in n_new]), (C.c_int32 * S)(*blocks), (C.c_float * (8 * S))(*coef),
                                              (C.c_float * (5 * S))(*fp), (C.c_int32 * (2 * S))(*ip), state.data_ptr(),
                                              decided.data_ptr(), pressed.data_ptr(), int(decided.shape[1]), table.data_ptr(),
                                              _lib.stream_ptr()),
                   "dtmf_items")
