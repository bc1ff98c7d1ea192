"""The tone rule of decode sessions in pools built with tones=True (models/stream_sessions.py: DecodeSessions.send_dtmf /
send_tones), on the host: segments and programs, the two tables, the rendering, the splice, and the builders for DTMF keys and
plain tones.  The pool's kernel (dmel_tone_items) is held to render() bit for bit; only tone_items(), the launch at the end,
needs a GPU.

A SEGMENT is the plain tuple (f1, f2, a1, a2, on, off, ramp): two tones of f1 and f2 Hz (integers, 0 <= f < rate / 2; f = 0 goes
with a = 0 and means "no such tone") with the amplitudes a1 and a2 (finite, >= 0, a1 + a2 <= 1 after their rounding to fp32, so
that no wire clips), sounding for `on` samples and followed by `off` samples of silence, the first and the last `ramp` samples of
the sound shaped by a raised cosine.  on, off and ramp count samples at the codec's (vocoder's) rate: 1 <= on < 2^24,
0 <= off < 2^24, 0 <= ramp <= min(on // 2, 4096).  A PROGRAM is a tuple of 1 .. 64 segments, played one after the other.

Tables, computed in float64 on the host and rounded once; the kernel evaluates no sine and no cosine:

    SIN  = sine_table(rate):  SIN[j]  = fp32(sin(2 pi j / rate)),               j in [0, rate)
    RAMP = ramp_table(n):     RAMP[i] = fp32(0.5 - 0.5 cos(pi (i + 0.5) / n)),  i in [0, n)

Sample i of a segment, 0 <= i < on:

    p_k = (f_k * i) mod rate                 exact integer arithmetic; the phase starts at 0 in every segment
    t_k = a_k * SIN[p_k]                     k = 1, 2
    x   = t_1 + t_2
    g   = RAMP[i] for i < ramp,  RAMP[on - 1 - i] for i >= on - ramp,  1.0f otherwise          (RAMP = ramp_table(ramp))
    y   = x * g

four separately rounded fp32 operations (two products, the sum, the product with g), no fused multiply-add.  The samples
on .. on + off - 1 are +0.0f.

splice(audio, inserts, rate) puts the rendering of a program IN FRONT OF sample P of a signal: that is what a session's audio is held
to -- its wire chain (resample, format, channels) applied to the splice of its codec-rate stream, however the tokens were cut
into pushes.

THE LEVELS ARE CHECKED ON SYNTHETIC SIGNALS AGAINST THIS PROJECT'S OWN DETECTOR ONLY (utils/dtmf.py: scan with the default
DtmfConfig reads the keys of dtmf_program back: tests/test_tones_cpu.py).  No conformance to ITU-T Q.23 / Q.24 is claimed; a
deployment should check its levels, twist and timing against the far end it dials."""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from . import dtmf

Segment = Tuple[int, int, float, float, int, int, int]
Program = Tuple[Segment, ...]

MAX_SEGMENTS = 64                                      # of a program, and of one tone part of dmel_tone_items
MAX_RAMP = 4096
MAX_SPAN = 1 << 24                                     # on and off lie below it
MIN_RATE, MAX_RATE = 4000, 192000
SEG_WORDS = 8                                          # 4-byte words per segment of the C entry's table: the seven and ramp_off
PART_TABLE_WORDS, SEG_TABLE_WORDS = 6, 5               # int64 of table scratch per part and per segment of dmel_tone_items


def check_rate(rate) -> int:
    if isinstance(rate, bool) or not isinstance(rate, int) or not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"rate must be an integer in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate!r}")
    return rate


@functools.lru_cache(maxsize=8)
def _sine(rate: int) -> np.ndarray:
    t = np.sin(2.0 * np.pi * np.arange(rate, dtype=np.float64) / rate).astype(np.float32)
    t.setflags(write=False)
    return t


def sine_table(rate: int) -> np.ndarray:
    """(rate,) fp32, read-only: sin(2 pi j / rate) in float64, rounded once"""
    return _sine(check_rate(rate))


@functools.lru_cache(maxsize=64)
def _ramp(n: int) -> np.ndarray:
    t = (0.5 - 0.5 * np.cos(np.pi * (np.arange(n, dtype=np.float64) + 0.5) / max(n, 1))).astype(np.float32)
    t.setflags(write=False)
    return t


def ramp_table(n: int) -> np.ndarray:
    """(n,) fp32, read-only: 0.5 - 0.5 cos(pi (i + 0.5) / n) in float64, rounded once; n in [0, 4096]"""
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_RAMP:
        raise ValueError(f"a ramp has 0 .. {MAX_RAMP} samples, got {n!r}")
    return _ramp(n)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_program(program, rate: int) -> Program:
    """the program as a tuple of plain tuples, its amplitudes rounded to fp32 (what render and the kernel multiply with);
    ValueError for anything outside the bounds of the module"""
    rate = check_rate(rate)
    try:
        segs = [tuple(s) for s in program]
    except TypeError:
        raise ValueError(f"a program is a sequence of segments (f1, f2, a1, a2, on, off, ramp), got {program!r}") from None
    if not 1 <= len(segs) <= MAX_SEGMENTS:
        raise ValueError(f"a program has 1 .. {MAX_SEGMENTS} segments, got {len(segs)}")
    out = []
    for k, s in enumerate(segs):
        if len(s) != 7:
            raise ValueError(f"segment {k}: expected (f1, f2, a1, a2, on, off, ramp), got {s!r}")
        f1, f2, a1, a2, on, off, ramp = s
        amps = []
        for name, f, a in (("f1", f1, a1), ("f2", f2, a2)):
            if not _is_int(f) or not 0 <= 2 * f < rate:
                raise ValueError(f"segment {k}: {name} must be an integer frequency in [0, {rate} / 2) Hz, got {f!r}")
            if isinstance(a, bool) or not isinstance(a, (int, float, np.floating)) or not math.isfinite(a) or a < 0:
                raise ValueError(f"segment {k}: the amplitude of {name} must be finite and >= 0, got {a!r}")
            a = float(np.float32(a))
            if f == 0 and a != 0.0:
                raise ValueError(f"segment {k}: {name} = 0 means no tone and goes with the amplitude 0, got {a!r}")
            amps.append(a)
        if amps[0] + amps[1] > 1.0:
            raise ValueError(f"segment {k}: the amplitudes {amps[0]!r} + {amps[1]!r} exceed 1: the sum of the tones would clip")
        if not _is_int(on) or not 1 <= on < MAX_SPAN:
            raise ValueError(f"segment {k}: on must be an integer in [1, 2^24) samples, got {on!r}")
        if not _is_int(off) or not 0 <= off < MAX_SPAN:
            raise ValueError(f"segment {k}: off must be an integer in [0, 2^24) samples, got {off!r}")
        if not _is_int(ramp) or not 0 <= ramp <= min(on // 2, MAX_RAMP):
            raise ValueError(f"segment {k}: ramp must be an integer in [0, min(on // 2, {MAX_RAMP})] samples, got {ramp!r}")
        out.append((int(f1), int(f2), amps[0], amps[1], int(on), int(off), int(ramp)))
    return tuple(out)


def _samples(ms, rate: int, what: str) -> int:
    if isinstance(ms, bool) or not isinstance(ms, (int, float)) or not math.isfinite(ms) or ms < 0:
        raise ValueError(f"{what} must be a finite number of milliseconds >= 0, got {ms!r}")
    return int(math.floor(ms * rate / 1000.0 + 0.5))


def _amplitude(db, what: str) -> float:
    if isinstance(db, bool) or not isinstance(db, (int, float)) or not math.isfinite(db):
        raise ValueError(f"{what} must be a finite level in dB, got {db!r}")
    return 10.0 ** (db / 20.0)


def dtmf_program(keys: str, rate: int, tone_ms=80, gap_ms=80, level_dbfs=-10.0, twist_db=2.0, ramp_ms=1.0) -> Program:
    """one segment per key of `keys` (dtmf.KEYS, letters in either case): the row tone at 10^(level_dbfs / 20), the column tone at
    10^((level_dbfs + twist_db) / 20), tone_ms of sound and gap_ms of silence, ramp_ms of raised cosine at both ends of the sound;
    milliseconds become floor(ms * rate / 1000 + 0.5) samples.  ValueError: a character that is no key, no key at all or more
    than 64, and whatever check_program refuses (levels that clip, a ramp above half the tone)"""
    rate = check_rate(rate)
    if not isinstance(keys, str) or not keys:
        raise ValueError(f"keys must be a non-empty string of {dtmf.KEYS!r}, got {keys!r}")
    on, off, ramp = _samples(tone_ms, rate, "tone_ms"), _samples(gap_ms, rate, "gap_ms"), _samples(ramp_ms, rate, "ramp_ms")
    if isinstance(twist_db, bool) or not isinstance(twist_db, (int, float)) or not math.isfinite(twist_db):
        raise ValueError(f"twist_db must be a finite number of dB, got {twist_db!r}")
    a_row, a_col = _amplitude(level_dbfs, "level_dbfs"), _amplitude(level_dbfs + twist_db, "level_dbfs + twist_db")
    segs = []
    for ch in keys:
        k = dtmf.KEYS.find(ch.upper())
        if k < 0 or len(ch) != 1:
            raise ValueError(f"{ch!r} is no DTMF key: the keys are {dtmf.KEYS!r}")
        segs.append((int(dtmf.ROWS_HZ[k // 4]), int(dtmf.COLS_HZ[k % 4]), a_row, a_col, on, off, ramp))
    return check_program(segs, rate)


def tone_program(freqs, ms, rate: int, level_dbfs=-10.0, gap_ms=0, ramp_ms=1.0) -> Program:
    """one segment of one or two tones (a beep, a dial tone, a ring-back cadence when sent repeatedly): every tone at
    10^(level_dbfs / 20), `ms` of sound, gap_ms of silence behind it, ramp_ms of raised cosine at both ends"""
    rate = check_rate(rate)
    freqs = (freqs,) if _is_int(freqs) else tuple(freqs)
    if not 1 <= len(freqs) <= 2:
        raise ValueError(f"a tone segment has one or two frequencies, got {len(freqs)}")
    if any(not _is_int(f) or f <= 0 for f in freqs):
        raise ValueError(f"frequencies must be positive integers (Hz), got {freqs!r}")
    a = _amplitude(level_dbfs, "level_dbfs")
    f2, a2 = (freqs[1], a) if len(freqs) == 2 else (0, 0.0)
    return check_program([(freqs[0], f2, a, a2, _samples(ms, rate, "ms"), _samples(gap_ms, rate, "gap_ms"),
                           _samples(ramp_ms, rate, "ramp_ms"))], rate)


def length(program) -> int:
    """samples the program renders to: the sum of on + off"""
    return sum(int(s[4]) + int(s[5]) for s in program)


def render(program, rate: int) -> np.ndarray:
    """(length(program),) fp32: the rule of the module, segment after segment"""
    program = check_program(program, rate)
    sin = sine_table(rate)
    out = np.zeros(length(program), dtype=np.float32)
    at = 0
    for f1, f2, a1, a2, on, off, ramp in program:
        i = np.arange(on, dtype=np.int64)
        t1 = np.float32(a1) * sin[(f1 * i) % rate]
        t2 = np.float32(a2) * sin[(f2 * i) % rate]
        x = t1 + t2
        g = np.ones(on, dtype=np.float32)
        if ramp:
            r = ramp_table(ramp)
            g[:ramp], g[on - ramp:] = r, r[::-1]
        out[at:at + on] = x * g                       # float32 arrays throughout: every operation is rounded to fp32
        at += on + off
    return out


def splice(audio, inserts, rate: int) -> np.ndarray:
    """audio: (n,) fp32 on the host (a numpy array or a CPU tensor); inserts: [(P, program), ...] with P non-decreasing and
    0 <= P <= n; rate: the rate of `audio`, at which the programs are rendered -> audio with render(program, rate) in front of its
    sample P, for every insert; equal P in list order"""
    x = audio.numpy() if isinstance(audio, torch.Tensor) else np.asarray(audio)
    if x.ndim != 1 or x.dtype != np.float32:
        raise ValueError(f"audio must be a 1-D fp32 array on the host, got {x.shape} {x.dtype}")
    parts, at = [], 0
    for k, (P, program) in enumerate(inserts):
        if not _is_int(P) or not at <= P <= x.shape[0]:
            raise ValueError(f"insert {k}: its position {P!r} must be an integer in [{at}, {x.shape[0]}] (non-decreasing positions "
                             f"inside the audio)")
        parts += [x[at:P], render(program, rate)]
        at = int(P)
    return np.concatenate(parts + [x[at:]]) if parts else x.copy()


# ---------------------------------------------------------------------------------------------------- the launch
def segment_words(program, ramp_off: Dict[int, int]) -> list:
    """the 8 words per segment dmel_tone_items takes, the amplitudes as the bits of their fp32 values; ramp_off: {ramp length:
    the offset of its table in the ramp arena} (a ramp of 0 reads nothing)"""
    words = []
    for f1, f2, a1, a2, on, off, ramp in program:
        bits = np.array([a1, a2], dtype=np.float32).view(np.int32)
        words += [f1, f2, int(bits[0]), int(bits[1]), on, off, ramp, ramp_off[ramp] if ramp else 0]
    return words


def table_words(parts: int, segments: int) -> int:
    """int64 of device scratch dmel_tone_items needs for that many parts and segments"""
    return PART_TABLE_WORDS * parts + SEG_TABLE_WORDS * segments


def ramp_arena(lengths, dev) -> Tuple[torch.Tensor, Dict[int, int]]:
    """the ramp tables of `lengths` back to back on `dev` -> (arena, {length: offset})"""
    off, at = {}, 0
    for n in sorted({int(n) for n in lengths if n}):
        off[n], at = at, at + n
    arena = np.concatenate([ramp_table(n) for n in off] + [np.zeros(1, np.float32)])
    return torch.from_numpy(arena).to(dev), off


def tone_items(parts: Sequence[Tuple[torch.Tensor, object]], rate: int, sine: Optional[torch.Tensor] = None,
               ramps: Optional[torch.Tensor] = None, ramp_off: Optional[Dict[int, int]] = None,
               table: Optional[torch.Tensor] = None) -> None:
    """parts of (dst, what) in ONE launch (dmel_tone_items): dst a 1-D fp32 CUDA tensor with contiguous samples; `what` a 1-D fp32
    CUDA tensor of dst's length (the part is its copy) or a checked program of length(program) == dst's length (the part is its
    rendering).  A spliced piece is three or more parts whose dst follow each other: head, tone, tail.  The destinations must not
    overlap each other or a source.  sine: sine_table(rate) on the device; ramps, ramp_off: the arena with the ramp table of every
    ramp length the programs use and {length: offset} (default for all three: built here); table: int64 device scratch of
    table_words(len(parts), segments) a caller that sends every step keeps.  Runs on the current stream."""
    R = len(parts)
    if R == 0:
        raise ValueError("no part to write")
    dev = parts[0][0].device
    programs = [w for _, w in parts if not isinstance(w, torch.Tensor)]
    if ramp_off is None or ramps is None:
        ramps, ramp_off = ramp_arena([s[6] for p in programs for s in p], dev)
    if sine is None:
        sine = torch.tensor(sine_table(rate)).to(dev)
    dst, src, n, first, count, words = [], [], [], [], [], []
    for r, (d, w) in enumerate(parts):
        _lib.require_cuda(d, "dst")
        if d.dtype != torch.float32 or d.ndim != 1 or (d.shape[0] > 1 and d.stride(0) != 1) or d.device != dev:
            raise ValueError(f"part {r}: dst must be a 1-D fp32 tensor of contiguous samples on {dev}")
        if isinstance(w, torch.Tensor):
            if w.dtype != torch.float32 or w.shape != d.shape or (w.shape[0] > 1 and w.stride(0) != 1) or w.device != dev:
                raise ValueError(f"part {r}: a source must be a 1-D fp32 tensor of dst's {d.shape[0]} contiguous samples on {dev}")
            src.append(w.data_ptr() or None)          # an empty copy is idle: the entry does not look at its pointers
            first.append(0)
            count.append(0)
        else:
            if length(w) != d.shape[0]:
                raise ValueError(f"part {r}: a program of {length(w)} samples into a destination of {d.shape[0]}")
            src.append(None)
            first.append(len(words) // SEG_WORDS)
            count.append(len(w))
            words += segment_words(w, ramp_off)
        dst.append(d.data_ptr() or None)
        n.append(d.shape[0])
    n_segs = len(words) // SEG_WORDS
    if table is None:
        table = torch.empty(max(table_words(R, n_segs), 1), dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or table.numel() < table_words(R, n_segs) or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {table_words(R, n_segs)} contiguous int64 on {dev}")
    P = C.c_void_p * R
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_tone_items(P(*dst), P(*src), (C.c_int64 * R)(*n), (C.c_int32 * R)(*first), (C.c_int32 * R)(*count), R,
                                              (C.c_int32 * max(len(words), 1))(*words), n_segs, sine.data_ptr(), int(rate),
                                              ramps.data_ptr(), int(ramps.numel()), table.data_ptr(), _lib.stream_ptr()),
                   "tone_items")
