"""The speaking-rate rule of decode sessions opened with pace= in pools built with pace=True (models/stream_sessions.py:
DecodeSessions.set_pace), on the host: the config, the requests, the per-session state row, the scan over samples, the integer
bookkeeping a pool sizes its outputs with, and the report a caller reads.  The pool's kernel (dmel_pace_items) is held to scan() bit
for bit; only pace_items(), the launch at the end, needs a GPU.

The rule is waveform-similarity overlap-add (WSOLA) on x, the session's finished speech stream at the codec's rate, positions counted
from 0: output frames of H samples are cut from x at positions that advance faster or slower than the output does, each moved
within +-D samples to where it continues the frame before it best, and cross-faded over the natural continuation of that frame.
The pitch stays; the pace changes.  The output length is NOT the input length, so every count is a pure function of integers.

Precision: everything is fp32, every operation is rounded on its own (no fused multiply-add), the divisions are the IEEE ones, and
every sum is sum8 exactly as utils/echo.py defines it (eight contiguous segments, each summed in ascending order from 0.0f, joined
as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))).

SIZES.  config.samples(rate) -> (H, D): H, the synthesis hop, is hop_ms in samples rounded to the nearest multiple of 8,
64 <= H <= 512; D, the search half-width, is search_ms in samples rounded to the nearest, 0 <= D <= 512.  Rates are integers in
permille of the unchanged speed, MIN_PERMILLE = 500 .. MAX_PERMILLE = 2000; 1500 speaks one and a half times as fast.  The analysis
hop of a rate r is Ha(r) = (H * r + 500) // 1000.  The weight table is W[i] = fp32(0.5 - 0.5 cos(pi (i + 0.5) / H)), i < H, computed
in float64 and rounded once (weight_table); the launch takes it from the caller, as the ramp tables of utils/shape.py are passed.

THE STREAM.  Samples at or behind the stream's final length L read as 0.0.  Output frame k = 0, 1, ... has a NOMINAL position a_k:
a_0 = 0, a_k = a_{k-1} + Ha(r_k), where r_k is the rate in force at input position a_{k-1}: that of the last request (P, permille)
with P <= a_{k-1}, else initial_permille.  Frame k has a CHOSEN position p_k, p_0 = 0.

FRAME 0 is x[0 : H] unchanged.

FRAME k >= 1.  t = p_{k-1} + H is the natural continuation of the frame before; old[i] = x[t + i], i < H.

    natural    a_k - D <= t <= a_k + D:  p_k = t, no search.  Rate 1000 is the identity by this, and a rate near 1000 copies the input
               until the drift exceeds D.
    quiet      otherwise, e0 = sum8(old * old) < floor:  p_k = a_k.
    searched   otherwise, for every d in [-D, D] with c = a_k + d >= 0:  b[i] = x[c + i],  cc = sum8(old * b),  e = sum8(b * b),
               q(d) = cc > 0 ? (cc * cc) / (e + eps) : 0  (a product, a sum, a division).  p_k = a_k + d*, d* the d with the largest
               VALUE q; among equal values the smallest |d| wins, then the negative d: a total order, so the order in which the
               candidates are reduced cannot matter (and where every q is 0, d* = 0).
    output     new[i] = x[p_k + i]:  m = new - old;  m = W[i] * m;  y[k H + i] = old + m  (three rounded operations).  Where
               p_k == t, new and old are the same samples and y[k H + i] = old[i], copied.

READINESS AND END depend on integers only: p_k never leaves the device.  A call that is not final computes frame 0 when fed >= H and
frame k >= 1 when fed >= max(a_{k-1} + 2 H, a_k + H) + D, fed the samples taken so far: then no sample the frame can read is
missing.  A final call computes every frame with a_k < L; its last frame K - 1 hands out min(H, L - a_{K-1}) samples only, so at
rate 1000 the output is x bit for bit, L samples long.  With K frames computed the rule reads input only at or behind
keep = max(0, min(a_{K-1} + H, a_K) - D); nothing in front of it is kept, hence fewer than 2 H + 2 D samples are held.  A final call
keeps nothing.

REQUESTS.  A request is (P, permille) with P >= the samples fed when it is made and P non-decreasing (equal positions: the later
request wins); check_request refuses the rest.  A frame whose a_{k-1} lies in front of the fed count is therefore never touched by a
later request, and the result cannot depend on how x was cut into calls.

THE INTEGERS a pool tracks per session without touching the device: (K, a_{K-1}, a_K, fed), a_{K-1} read as 0 while K == 0.
advance() steps them and gives the frames and samples of a step, keep_from() the position above, max_out() the most one step can
hand out.

State of a session: a row of HEADER = 16 4-byte words and 2 H + 2 D floats, the held input samples [keep, fed), oldest first,
zeros behind them.

    0  K         int32  frames computed                         8  quiet      int32
    1  p_last    int32  p_{K-1}                                 9  out        int32  samples handed out
    2  a_last    int32  a_{K-1}                                 10 last_off   int32  p - a of the last frame
    3  a_next    int32  a_K                                     11 last_q     fp32   q of the last frame (0: natural, quiet)
    4  fed       int32  samples taken                           12 permille   int32  r_K, the rate that placed a_K (0 while K == 0)
    5  hold      int32  samples held, below 2 H + 2 D           13 .. 15      reserved, kept at 0
    6  natural   int32  frames copied (frame 0 among them)
    7  searched  int32

A zeroed row is the fresh state.  The launch takes hold and the four integers from the HOST, trusts them and writes them back.

THE DEFAULTS (10 ms hop, 6.5 ms search, floor 1e-6) ARE CHECKED ON SYNTHETIC SIGNALS ONLY (a harmonic voiced-like signal with vibrato,
tremolo and noise: tests/test_pace_cpu.py) and are not tuned on speech.  One fixed frame size is used whatever the pitch.  Transients
are not protected: a click may be repeated or dropped.  There is no pitch marking.  The counters and positions are int32; nothing
checks for their overflow.  NaN and infinite input are outside the contract."""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .echo import _sum8_even, sum8                     # the one summation order; _sum8_even is sum8 along rows of H % 8 == 0 terms

HEADER = 16
MIN_HOP, MAX_HOP = 64, 512
MAX_SEARCH = 512
MIN_PERMILLE, MAX_PERMILLE = 500, 2000
MAX_REQUESTS = 8                                       # live requests of a slot in one launch
TABLE_WORDS = 64                                       # 4-byte words of table scratch per slot of dmel_pace_items
WINDOW = 6144                                          # samples of a slot's stream the kernel's workgroup holds in LDS at a time
MAX_NEW = 1 << 26                                      # new samples of a slot in one launch
I_K, I_P, I_APREV, I_ANEXT, I_FED, I_HOLD, I_NATURAL, I_SEARCHED, I_QUIET, I_OUT, I_OFF, I_Q, I_PERMILLE = range(13)

Request = Tuple[int, int]                              # (P, permille)
Ints = Tuple[int, int, int, int]                       # (K, a_{K-1}, a_K, fed)
FRESH: Ints = (0, 0, 0, 0)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def analysis_hop(H: int, permille: int) -> int:
    """Ha(r), in integers"""
    return (int(H) * int(permille) + 500) // 1000


@functools.lru_cache(maxsize=64)
def _weights(H: int) -> np.ndarray:
    w = (0.5 - 0.5 * np.cos(np.pi * (np.arange(H, dtype=np.float64) + 0.5) / H)).astype(np.float32)
    w.setflags(write=False)
    return w


def weight_table(H: int) -> np.ndarray:
    """(H,) fp32, read-only: W of the module"""
    if not _is_int(H) or not MIN_HOP <= H <= MAX_HOP or H % 8:
        raise ValueError(f"a hop is a multiple of 8 in [{MIN_HOP}, {MAX_HOP}] samples, got {H!r}")
    return _weights(int(H))


def check_permille(permille) -> int:
    if not _is_int(permille) or not MIN_PERMILLE <= permille <= MAX_PERMILLE:
        raise ValueError(f"a rate is an integer in [{MIN_PERMILLE}, {MAX_PERMILLE}] permille, got {permille!r}")
    return int(permille)


@dataclasses.dataclass(frozen=True)
class PaceConfig:
    """Plain values; see the module for what each does.  The defaults are checked on synthetic signals only."""
    hop_ms: float = 10.0
    search_ms: float = 6.5
    floor: float = 1e-6
    eps: float = 1e-12
    initial_permille: int = 1000

    def __post_init__(self):
        f32 = np.finfo(np.float32)
        for name in ("hop_ms", "search_ms", "floor", "eps"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
            if name in ("floor", "eps") and v != 0 and not float(f32.tiny) <= v <= float(f32.max):
                raise ValueError(f"{name} = {v!r} is no normal fp32 number")       # what the kernel computes with is the fp32 value
            object.__setattr__(self, name, float(v))
        if not self.hop_ms > 0 or not self.eps > 0:
            raise ValueError(f"hop_ms and eps must be > 0, got {self.hop_ms!r} and {self.eps!r}")
        object.__setattr__(self, "initial_permille", check_permille(self.initial_permille))

    def samples(self, rate: int) -> Tuple[int, int]:
        """(H, D) at `rate`; ValueError where the rate or a size does not fit"""
        if isinstance(rate, bool) or not isinstance(rate, int) or rate <= 0:
            raise ValueError(f"rate must be a positive integer, got {rate!r}")
        return _samples(self, rate)

    def state_words(self, rate: int) -> int:
        """4-byte words of a session's state row: the header and 2 H + 2 D held samples"""
        H, D = self.samples(rate)
        return HEADER + 2 * H + 2 * D

    def fparams(self) -> Tuple[float, float]:
        """(floor, eps) as the fp32 values scan and dmel_pace_items compute with"""
        return float(np.float32(self.floor)), float(np.float32(self.eps))

    def as_dict(self) -> dict:
        """plain values (a snapshot's meta)"""
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d) -> "PaceConfig":
        return cls(**dict(d))


@functools.lru_cache(maxsize=64)
def _samples(config: PaceConfig, rate: int) -> Tuple[int, int]:
    H = 8 * int(math.floor(rate * config.hop_ms / 8000.0 + 0.5))
    D = int(math.floor(rate * config.search_ms / 1000.0 + 0.5))
    if not MIN_HOP <= H <= MAX_HOP:
        raise ValueError(f"a hop of {H} samples at {rate} Hz is outside [{MIN_HOP}, {MAX_HOP}]: set hop_ms")
    if not 0 <= D <= MAX_SEARCH:
        raise ValueError(f"a search half-width of {D} samples at {rate} Hz is outside [0, {MAX_SEARCH}]: set search_ms")
    return H, D


def as_config(pace) -> Optional[PaceConfig]:
    """what open(pace=) takes: None / False -> None, True -> the defaults, a PaceConfig -> itself"""
    if pace is None or pace is False:
        return None
    if pace is True:
        return PaceConfig()
    if isinstance(pace, PaceConfig):
        return pace
    raise ValueError(f"pace must be None, a bool or a PaceConfig, got {type(pace).__name__}")


# ---------------------------------------------------------------------------------------------------- requests and integers
def check_request(request, fed: int = 0, after: int = 0) -> Request:
    """(P, permille) as plain ints; ValueError outside the bounds of the module.  fed: the samples the pacer has taken when the
    request is made; after: an earlier request's position"""
    try:
        P, permille = request
    except (TypeError, ValueError):
        raise ValueError(f"a request is (P, permille), got {request!r}") from None
    lo = max(int(fed), int(after))
    if not _is_int(P) or not lo <= P < 2 ** 30:
        raise ValueError(f"a request's position must be an integer in [{lo}, 2^30): not in front of the {int(fed)} samples fed nor of "
                         f"an earlier request ({int(after)}), got {P!r}")
    return int(P), check_permille(permille)


def _ordered(requests) -> List[Request]:
    out, after = [], 0
    for r in requests:
        r = check_request(r, 0, after)
        out.append(r)
        after = r[0]
    return out


def rate_at(requests: Sequence[Request], initial: int, pos: int) -> int:
    """the rate in force at input position pos: the last request with P <= pos, else `initial`"""
    r = int(initial)
    for P, permille in requests:
        if P <= pos:
            r = permille
    return r


def live(requests: Sequence[Request], initial: int, a_next: int) -> Tuple[List[Request], int]:
    """what frames behind a_K still need: the requests in front of which a_K lies, and the rate in force at a_K"""
    return [r for r in requests if r[0] > a_next], rate_at(requests, initial, a_next)


def ready(k: int, a_prev: int, a_k: int, H: int, D: int) -> int:
    """the fed count from which a call that is not final computes frame k"""
    return H if k == 0 else max(a_prev + 2 * H, a_k + H) + D


def advance(ints: Ints, requests: Sequence[Request], n_new: int, final: bool, H: int, D: int,
            initial: int = 1000) -> Tuple[Ints, int, int]:
    """one step on integers alone: (K, a_{K-1}, a_K, fed), ALL requests of the session (or live()'s, with its rate as `initial`),
    the samples the step takes -> (the integers after it, the frames it completes, the samples it hands out)"""
    K, a_prev, a_next, fed = (int(v) for v in ints)
    L = fed + int(n_new)
    frames = n_out = 0
    while (a_next < L) if final else (L >= ready(K, a_prev, a_next, H, D)):
        a_prev, a_next = a_next, a_next + analysis_hop(H, rate_at(requests, initial, a_next))
        K, frames, n_out = K + 1, frames + 1, n_out + H
    if final and frames:
        n_out -= H - min(H, L - a_prev)
    return (K, a_prev, a_next, L), frames, n_out


def keep_from(ints: Ints, H: int, D: int, final: bool = False) -> int:
    """the position nothing in front of which is kept behind a step that left `ints`; held = fed - keep_from"""
    K, a_prev, a_next, fed = (int(v) for v in ints)
    if final:
        return fed
    if K == 0:
        return 0
    return min(fed, max(0, min(a_prev + H, a_next) - D))


def max_out(n_in: int, H: int, D: int) -> int:
    """the most samples one step of n_in new samples can hand out, at any rate and in any state: a frame that waits lies less than
    3 H / 2 + D in front of the fed count, frames are at least H / 2 apart, and every one hands out at most H"""
    half = H // 2
    return H * -(-(int(n_in) + 3 * half + D) // half)


# ---------------------------------------------------------------------------------------------------- the scan
def fresh_state(config: PaceConfig, rate: int) -> torch.Tensor:
    """int32 zeros of config.state_words(rate): the state of a session that has taken no sample"""
    return torch.zeros(config.state_words(rate), dtype=torch.int32)


def ints_of(state: torch.Tensor) -> Ints:
    """(K, a_{K-1}, a_K, fed) of a host state row"""
    return tuple(int(state[i]) for i in (I_K, I_APREV, I_ANEXT, I_FED))


def _best(q: np.ndarray, d: np.ndarray) -> int:
    """index of the largest value q; equal values: the smallest |d|, then the negative d"""
    at = np.nonzero(q == q.max())[0]
    return int(at[np.lexsort((d[at], np.abs(d[at])))[0]])


def scan(x, requests: Sequence[Request], config: PaceConfig, rate: int, state: Optional[torch.Tensor] = None,
         final: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """x: (n,) fp32 on the host (a numpy array or a CPU tensor), n >= 0, the samples behind those `state` has taken; requests: ALL
    requests of the session so far, [(P, permille), ...] at absolute input positions; state: what an earlier call returned (None:
    fresh); final: these are the stream's last samples -> (y fp32: the samples handed out, state after the step, frame_offset (F,)
    int32: p_k - a_k, frame_score (F,) fp32: q, 0 for natural and quiet frames, of the F frames the step completed).  No argument is
    modified.  Any cut of the samples gives the bits of one call.  n == 0 without final is an idle step: the state comes back as
    it is."""
    xs = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if xs.ndim != 1 or xs.dtype != np.float32:
        raise ValueError(f"x must be a 1-D fp32 array on the host, got {xs.shape} {xs.dtype}")
    H, D = config.samples(rate)
    W = weight_table(H)
    floor, eps = (np.float32(v) for v in config.fparams())
    words_n = config.state_words(rate)
    if state is None:
        state = fresh_state(config, rate)
    if state.dtype != torch.int32 or tuple(state.shape) != (words_n,) or state.device.type != "cpu":
        raise ValueError(f"state must be a CPU int32 tensor of {words_n} words, got {tuple(state.shape)} {state.dtype}")
    words = state.clone().numpy()
    fl = words.view(np.float32)
    ints = ints_of(state)
    K, a_prev, a_next, fed = ints
    hold, p_prev = int(words[I_HOLD]), int(words[I_P])
    if not 0 <= hold < max(1, 2 * H + 2 * D) or hold > fed:
        raise ValueError(f"the state holds {hold} samples, which H = {H}, D = {D} and {fed} fed samples do not allow")
    n = int(xs.shape[0])
    none_f, none_i = torch.zeros(0, dtype=torch.float32), torch.zeros(0, dtype=torch.int32)
    if n == 0 and not final:
        return none_f, torch.from_numpy(words), none_i, none_f.clone()
    reqs = _ordered(requests)
    base, L = fed - hold, fed + n
    buf = np.concatenate([fl[HEADER:HEADER + hold].copy(), xs])

    def read(pos: int, cnt: int) -> np.ndarray:
        """x[pos : pos + cnt], 0.0 at and behind L"""
        assert pos >= base, (pos, base)
        out = np.zeros(cnt, dtype=np.float32)
        have = max(0, min(cnt, L - pos))
        out[:have] = buf[pos - base:pos - base + have]
        return out

    after, frames, n_out = advance(ints, reqs, n, final, H, D, config.initial_permille)
    y = np.empty(n_out, dtype=np.float32)
    offs, scores = np.zeros(frames, dtype=np.int32), np.zeros(frames, dtype=np.float32)
    natural, searched, quiet = (int(words[i]) for i in (I_NATURAL, I_SEARCHED, I_QUIET))
    permille = int(words[I_PERMILLE])
    for j in range(frames):
        a_k, q = a_next, np.float32(0.0)
        if K == 0:
            p, out = 0, read(0, H)
            natural += 1
        else:
            t = p_prev + H
            old = read(t, H)
            if a_k - D <= t <= a_k + D:
                p = t
                natural += 1
            elif _sum8_even(old * old) < floor:
                p = a_k
                quiet += 1
            else:
                lo = max(-D, -a_k)
                d = np.arange(lo, D + 1, dtype=np.int64)
                B = np.lib.stride_tricks.sliding_window_view(read(a_k + lo, D - lo + H), H)
                cc, e = _sum8_even(old[None, :] * B), _sum8_even(B * B)
                qs = np.where(cc > 0, (cc * cc) / (e + eps), np.float32(0.0)).astype(np.float32)
                i = _best(qs, d)
                p, q = a_k + int(d[i]), qs[i]
                searched += 1
            if p == t:
                out = old
            else:
                m = read(p, H) - old
                m = W * m
                out = old + m
        emit = min(H, n_out - j * H)
        y[j * H:j * H + emit] = out[:emit]
        offs[j], scores[j] = p - a_k, q
        permille = rate_at(reqs, config.initial_permille, a_k)
        a_prev, a_next = a_k, a_k + analysis_hop(H, permille)
        K, p_prev = K + 1, p
    assert (K, a_prev, a_next, L) == after
    keep = keep_from(after, H, D, final)
    new_hold = L - keep
    assert 0 <= new_hold < max(1, 2 * H + 2 * D), (new_hold, H, D)
    held = read(keep, new_hold)
    words[I_K], words[I_P], words[I_APREV], words[I_ANEXT], words[I_FED], words[I_HOLD] = K, p_prev, a_prev, a_next, L, new_hold
    words[I_NATURAL], words[I_SEARCHED], words[I_QUIET], words[I_OUT] = natural, searched, quiet, int(words[I_OUT]) + n_out
    words[I_PERMILLE] = permille
    if frames:
        words[I_OFF], fl[I_Q] = offs[-1], scores[-1]
    fl[HEADER:HEADER + new_hold] = held
    words[HEADER + new_hold:] = 0
    return torch.from_numpy(y), torch.from_numpy(words), torch.from_numpy(offs), torch.from_numpy(scores)


@dataclasses.dataclass(frozen=True)
class PaceReport:
    """What a caller reads of a session's pacer, built from the header of its state row.

        frames                      output frames computed = natural + searched + quiet
        natural, searched, quiet    frames copied as the input continues, placed by the search, placed on a silent template
        samples_in, samples_out     input samples taken, samples handed out
        permille                    the rate that placed the next frame (the initial rate before the first)
        ratio                       samples_out / samples_in so far (0.0 before the first sample)
        last_offset, last_score     p - a and q of the last frame
    """
    frames: int
    natural: int
    searched: int
    quiet: int
    samples_in: int
    samples_out: int
    permille: int
    ratio: float
    last_offset: int
    last_score: float


def report(state: torch.Tensor, initial_permille: int = 1000) -> PaceReport:
    """the report of a state row or of its header (any device -- one copy to the host)"""
    row = state[:HEADER].cpu()
    w, f = [int(v) for v in row.tolist()], [float(v) for v in row.view(torch.float32).tolist()]
    return PaceReport(frames=w[I_K], natural=w[I_NATURAL], searched=w[I_SEARCHED], quiet=w[I_QUIET], samples_in=w[I_FED],
                      samples_out=w[I_OUT], permille=w[I_PERMILLE] or int(initial_permille),
                      ratio=w[I_OUT] / w[I_FED] if w[I_FED] else 0.0, last_offset=w[I_OFF], last_score=f[I_Q])


# ---------------------------------------------------------------------------------------------------- the launch
def weight_arena(hops, dev) -> Tuple[torch.Tensor, Dict[int, int]]:
    """the weight tables of `hops` back to back on `dev` -> (arena, {H: offset})"""
    off, at = {}, 0
    for h in sorted({int(h) for h in hops if h}):
        off[h], at = at, at + h
    arena = np.concatenate([weight_table(h) for h in off] + [np.zeros(1, np.float32)])
    return torch.from_numpy(arena).to(dev), off


def pace_items(src: Sequence[Optional[torch.Tensor]], dst: Sequence[Optional[torch.Tensor]], configs: Sequence[Optional[PaceConfig]],
               requests: Sequence[Sequence[Request]], ints: Sequence[Ints], final: Sequence[bool], state: torch.Tensor,
               out_offset: torch.Tensor, out_score: torch.Tensor, rate: int, weights: Optional[torch.Tensor] = None,
               weight_off: Optional[Dict[int, int]] = None, table: Optional[torch.Tensor] = None,
               initial: Optional[Sequence[Optional[int]]] = None) -> Tuple[List[int], List[Ints], List[int]]:
    """all slots of a step in ONE launch (dmel_pace_items) -> (the samples each slot's dst received, each slot's integers after the
    step, the frames each slot completed).  Slot s takes the samples of src[s] (a 1-D fp32 CUDA tensor with contiguous samples, or
    None for none) as x[fed ...], with the requests requests[s] (absolute positions; all of the session's, or those still live) and
    the integers ints[s] = (K, a_{K-1}, a_K, fed) the caller tracks from advance(), and writes the step's samples to dst[s] (another
    buffer than src[s]; at least that long; None where nothing can leave).  A slot with no samples that is not final is idle: its
    rows are not touched, configs[s] may be None and its integers come back as they are.  state: (S, pitch) int32, contiguous,
    pitch >= configs[s].state_words(rate), updated in place; out_offset (int32) / out_score (fp32): (S, pitch), contiguous, pitch >=
    the frames any slot completes.  weights, weight_off: the arena with the table of every hop in use and {H: offset} (default:
    built here); table: int32 device scratch of 64 * S words a caller that paces every step keeps; initial[s]: the rate in force in
    front of requests[s] where the caller has folded earlier requests away with live() (default: the config's initial_permille).
    Runs on the current stream."""
    S = len(src)
    if S == 0:
        raise ValueError("no slot to pace")
    if not (len(dst) == len(configs) == len(requests) == len(ints) == len(final) == S):
        raise ValueError(f"{S} slots need {S} of every per-slot argument")
    _lib.require_cuda(state, "state")
    dev = state.device
    if state.dtype != torch.int32 or state.ndim != 2 or state.shape[0] != S or not state.is_contiguous():
        raise ValueError(f"state must be a contiguous int32 tensor ({S}, pitch) on {dev}")
    for t, name, dt in ((out_offset, "out_offset", torch.int32), (out_score, "out_score", torch.float32)):
        if t.dtype != dt or t.ndim != 2 or t.shape[0] != S or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {dt} tensor ({S}, pitch) on {dev}")
    if out_offset.shape[1] != out_score.shape[1]:
        raise ValueError("out_offset and out_score must have one pitch")
    sizes = [cfg.samples(rate) if cfg is not None else (0, 0) for cfg in configs]
    if weight_off is None or weights is None:
        weights, weight_off = weight_arena([h for h, _ in sizes], dev)
    sp, dp, cap, n_new, flags, hs, ds, fp, iv, basep, counts, words, woff = [], [], [], [], [], [], [], [], [], [], [], [], []
    out, after, frames = [], [], []
    for s in range(S):
        x, d, cfg = src[s], dst[s], configs[s]
        for t, name in ((x, "src"), (d, "dst")):
            if t is not None and (t.dtype != torch.float32 or t.ndim != 1 or (t.shape[0] > 1 and t.stride(0) != 1) or t.device != dev):
                raise ValueError(f"slot {s}: {name} must be a 1-D fp32 tensor of contiguous samples on {dev}")
        n = 0 if x is None else int(x.shape[0])
        idle = n == 0 and not final[s]
        if not idle and cfg is None:
            raise ValueError(f"slot {s} takes part and has no config")
        H, D = sizes[s]
        sp.append(x.data_ptr() or None if n else None)
        dp.append(d.data_ptr() or None if d is not None and d.shape[0] else None)
        cap.append(0 if d is None else int(d.shape[0]))
        n_new.append(n)
        flags.append(1 if final[s] else 0)
        hs.append(H), ds.append(D)
        fp += list(cfg.fparams()) if cfg else [0.0, 0.0]
        if idle:
            iv += [0] * 5
            basep.append(0), counts.append(0), woff.append(0)
            words += [0] * (2 * MAX_REQUESTS)
            out.append(0), after.append(tuple(int(v) for v in ints[s])), frames.append(0)
            continue
        K, a_prev, a_next, fed = (int(v) for v in ints[s])
        first = cfg.initial_permille if initial is None or initial[s] is None else check_permille(initial[s])
        lv, b = live(_ordered(requests[s]), first, a_next)
        if len(lv) > MAX_REQUESTS:
            raise ValueError(f"slot {s}: {len(lv)} live requests, at most {MAX_REQUESTS}")
        if H not in weight_off:
            raise ValueError(f"slot {s}: no weight table of {H} samples in the arena")
        nxt, fr, no = advance((K, a_prev, a_next, fed), lv, n, bool(final[s]), H, D, b)
        iv += [K, a_prev, a_next, fed, fed - keep_from((K, a_prev, a_next, fed), H, D)]
        basep.append(b), counts.append(len(lv)), woff.append(weight_off[H])
        for k in range(MAX_REQUESTS):
            words += [min(lv[k][0] - fed, 1 << 30), lv[k][1]] if k < len(lv) else [0, 0]
        out.append(no), after.append(nxt), frames.append(fr)
    if table is None:
        table = torch.empty(TABLE_WORDS * S, dtype=torch.int32, device=dev)
    elif table.dtype != torch.int32 or table.numel() < TABLE_WORDS * S or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {TABLE_WORDS * S} contiguous int32 on {dev}")
    P, I64, I32 = C.c_void_p * S, C.c_int64 * S, C.c_int32 * S
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_pace_items(P(*dp), I64(*cap), P(*sp), I64(*n_new), (C.c_int64 * (5 * S))(*iv), I32(*flags), I32(*hs),
                                              I32(*ds), (C.c_float * (2 * S))(*fp), I32(*basep), I32(*counts),
                                              (C.c_int32 * (2 * MAX_REQUESTS * S))(*words), S, weights.data_ptr(), int(weights.numel()),
                                              I32(*woff), state.data_ptr(), int(state.shape[1]), out_offset.data_ptr(),
                                              out_score.data_ptr(), int(out_offset.shape[1]), table.data_ptr(), _lib.stream_ptr()),
                   "pace_items")
    return out, after, frames
