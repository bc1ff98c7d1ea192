"""The cross-fade rule of decode sessions that emit early (models/stream_sessions.py: DecodeSessions, open(crossfade_samples=F)), on
the host: the weights, the blend, and a stitcher that turns prefix decodes into the pieces such a session hands out.  The pool's
kernel (dmel_crossfade_items) is held to this module bit for bit; only crossfade_items(), the launch at the end, needs a GPU.

An early session cuts every piece from a different prefix decode, so the waveform steps at a piece boundary.  With a cross-fade of
F samples (1 <= F <= samples per mel frame) a piece ends F samples early, those F samples -- the tail -- wait, and the next piece
begins with the blend of the tail and the next decode's version of the same samples:

    w_i   = 0.5 - 0.5 cos(pi (i + 0.5) / F),  i in [0, F): float64 on the host, rounded once to fp32
    out_i = old_i + w_i * (new_i - old_i):    three fp32 operations, each rounded (no fused multiply-add)

Where both versions agree the blend returns `old` exactly (new - old is 0), so a session whose look-ahead covers the geometry's
hold returns decode()'s audio, F samples late.  With raw ranges [A_j, B_j) (what the session hands out without a fade) and prefix
decodes P_j:

    first non-empty piece                 P[A, B - F)
    next non-empty piece                  blend(tail, P[A - F, A)) then P[A, B - F)      (up to B on the final push)
    empty raw range                       nothing; the tail waits
    final push with an empty raw range    the tail, unblended: no newer version exists

The pieces tile [0, total) without gap or overlap; the audio runs F samples behind the mel."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib

MAX_FADE = 4096                                        # what one row of dmel_crossfade_items takes


def check_fade(F, limit: Optional[int] = None, what: str = "crossfade_samples") -> int:
    """F as an int in [1, min(limit, MAX_FADE)]; a bool or a non-int is a ValueError"""
    top = MAX_FADE if limit is None else min(int(limit), MAX_FADE)
    if isinstance(F, bool) or not isinstance(F, int) or not 1 <= F <= top:
        raise ValueError(f"{what} must be an integer in [1, {top}], got {F!r}")
    return F


def weights(F: int) -> torch.Tensor:
    """(F,) fp32: 0.5 - 0.5 cos(pi (i + 0.5) / F) in float64, rounded once"""
    F = check_fade(F)
    return torch.tensor([0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / F) for i in range(F)], dtype=torch.float64).to(torch.float32)


def blend(old: torch.Tensor, new: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """old + w * (new - old) over the last dimension: on CPU fp32 tensors the bits of the pool's kernel"""
    return old + w * (new - old)


class Stitcher:
    """One session's cross-fade on the host.  push(prefix, a, b, final): `prefix` is the prefix decode of the moment (..., n) with
    samples last, [a, b) the raw sample range of the push (a == b: no new frames) -> the piece the session hands out.  F = 0 hands
    out the raw crops."""

    def __init__(self, F: int):
        self.F = check_fade(F) if F else 0
        self.w = weights(F) if F else None
        self.tail: Optional[torch.Tensor] = None
        self.at = 0                                    # the raw frontier: the next range starts here
        self.finished = False

    def push(self, prefix: torch.Tensor, a: int, b: int, final: bool = False) -> torch.Tensor:
        if self.finished:
            raise RuntimeError("stream already finished")
        if a != self.at or b < a or b > prefix.shape[-1]:
            raise ValueError(f"raw range [{a}, {b}) does not continue at {self.at} inside a decode of {prefix.shape[-1]} samples")
        F = self.F
        if b - a and b - a < F:
            raise ValueError(f"a raw piece of {b - a} samples is shorter than the fade of {F}")
        self.at, self.finished = b, final
        if F == 0:
            return prefix[..., a:b].clone()
        if b == a:
            if final and self.tail is not None:
                out, self.tail = self.tail, None
                return out
            return prefix[..., a:a].clone()
        head = []
        if self.tail is not None:
            head.append(blend(self.tail, prefix[..., a - F:a], self.w.to(prefix.device)))
        end = b if final else b - F
        self.tail = None if final else prefix[..., b - F:b].clone()
        return torch.cat(head + [prefix[..., a:end]], dim=-1)


def stitch(prefixes: Sequence[torch.Tensor], ranges: Sequence[Tuple[int, int]], F: int) -> List[torch.Tensor]:
    """the pieces of a whole session: prefixes[j] and ranges[j] = (A_j, B_j) of push j, the last push final"""
    st = Stitcher(F)
    return [st.push(p, a, b, j == len(ranges) - 1) for j, (p, (a, b)) in enumerate(zip(prefixes, ranges))]


# ---------------------------------------------------------------------------------------------------- the launch
def crossfade_items(rows: Sequence[Tuple[Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor], torch.Tensor]],
                    table: Optional[torch.Tensor] = None) -> None:
    """rows of (blend | None, tail, save | None, w), 1-D fp32 CUDA tensors of one length F per row with contiguous samples, in ONE
    launch (dmel_crossfade_items): blend[:] = tail + w * (blend - tail) in place where blend is given, then tail[:] = save where save
    is given.  The blend and save regions of a row must not overlap, and no two rows may share what they write.  table: device
    scratch of 5 * len(rows) int64 a caller that fades every step keeps (default: allocated here).  Runs on the current stream."""
    R = len(rows)
    if R == 0:
        raise ValueError("no row to cross-fade")
    dev = rows[0][1].device
    for r, (x, tail, save, w) in enumerate(rows):
        F = tail.shape[0] if tail.ndim == 1 else -1
        for t, name in ((x, "blend"), (tail, "tail"), (save, "save"), (w, "w")):
            if t is None and name in ("blend", "save"):
                continue
            _lib.require_cuda(t, name)
            if t.dtype != torch.float32 or t.ndim != 1 or t.shape[0] != F or (F > 1 and t.stride(0) != 1) or t.device != dev:
                raise ValueError(f"row {r}: {name} must be a 1-D fp32 tensor of the row's {F} contiguous samples on {dev}")
    if table is None:
        table = torch.empty(5 * R, dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or table.numel() < 5 * R or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {5 * R} contiguous int64 on {dev}")
    P, I64 = C.c_void_p * R, C.c_int64 * R
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_crossfade_items(P(*[ptr(x) for x, _, _, _ in rows]), P(*[t.data_ptr() for _, t, _, _ in rows]),
                                                   P(*[ptr(s) for _, _, s, _ in rows]), P(*[w.data_ptr() for _, _, _, w in rows]),
                                                   I64(*[t.shape[0] for _, t, _, _ in rows]), R, table.data_ptr(), _lib.stream_ptr()),
                   "crossfade_items")
