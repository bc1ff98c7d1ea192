"""The sample format of the wire on the MI355X: 16-bit signed PCM <-> fp32 (csrc/small_ops.hip: pcm_convert_kernel, through
dmel_pcm_convert_items).  Microphones, RTP, WebSocket audio and sound cards carry int16; the codec computes in fp32.

The rounding rule, written down once:

    s16 -> f32   y = x / 32768                                      exact; full scale is -1.0, the largest value 1 - 2^-15
    f32 -> s16   y = round_half_even(clamp(x * 32768, -32768, 32767))
                 the product is exact (a power of two); ties go to the EVEN integer (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -1.5 -> -2),
                 as torch.round and numpy.rint do -- not truncation, not round-half-away, not a scale of 32767; NaN -> 0, +-inf
                 saturate; no dither, so the result is deterministic.  On the CPU:
                 clamp(round(nan_to_num(y, nan=0) * 32768), -32768, 32767).to(int16)

from_pcm16 / to_pcm16 convert a whole tensor, convert_items any list of ragged pieces, each in ONE launch.  The session pools
(models/stream_sessions.py) fold the same launch into the per-slot copies they make anyway: open(sample_format="s16").

Out of scope: other formats (s24, s32, u8, mu-law) and dither."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib

# sample_format -> (DMEL_SAMPLE_* of include/dmel_hip.h, dtype)
FORMATS = {"f32": (0, torch.float32), "s16": (1, torch.int16)}
_CODE = {dt: code for code, dt in FORMATS.values()}
MAX_ITEMS = 65535


def check_format(sample_format) -> str:
    if sample_format not in FORMATS:
        raise ValueError(f"unknown sample format {sample_format!r}: expected one of {sorted(FORMATS)}")
    return sample_format


@torch.no_grad()
def convert_items(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], table: Optional[torch.Tensor] = None) -> None:
    """dsts[i][:] = convert(srcs[i]) for lists of 1-D CUDA tensors with contiguous samples, int16 or float32, in ONE launch: s16 -> f32,
    f32 -> s16 (the rounding rule of the module docstring) or f32 -> f32 (a copy); s16 -> s16 is refused.  Pieces may have any
    lengths, 0 included, and any alignment; no destination may overlap a source or another destination.  table: device scratch of
    4 * len(srcs) int64 a caller that converts every step keeps (default: allocated here).  Runs on the current stream."""
    B = len(srcs)
    if B != len(dsts) or not 1 <= B <= MAX_ITEMS:
        raise ValueError(f"expected as many destinations as sources, 1 .. {MAX_ITEMS} of them (got {B} and {len(dsts)})")
    dev = srcs[0].device
    for i, (x, y) in enumerate(zip(srcs, dsts)):
        _lib.require_cuda(x, "source")
        _lib.require_cuda(y, "destination")
        if x.dtype not in _CODE or y.dtype not in _CODE:
            raise ValueError(f"item {i}: {x.dtype} -> {y.dtype}: samples are torch.int16 or torch.float32")
        if x.ndim != 1 or y.ndim != 1 or x.shape != y.shape or (x.shape[0] > 1 and (x.stride(0) != 1 or y.stride(0) != 1)):
            raise ValueError(f"item {i}: expected two 1-D tensors of equal length with contiguous samples, got {tuple(x.shape)} "
                             f"(stride {x.stride()}) -> {tuple(y.shape)} (stride {y.stride()})")
        if x.device != dev or y.device != dev:
            raise ValueError(f"item {i}: all pieces must live on one device")
    if table is None:
        table = torch.empty(4 * B, dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or table.numel() < 4 * B or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {4 * B} contiguous int64 on {dev}")
    P, I32, I64 = C.c_void_p * B, C.c_int32 * B, C.c_int64 * B
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_pcm_convert_items(P(*[x.data_ptr() for x in srcs]), I32(*[_CODE[x.dtype] for x in srcs]),
                                                     P(*[y.data_ptr() for y in dsts]), I32(*[_CODE[y.dtype] for y in dsts]),
                                                     I64(*[x.shape[0] for x in srcs]), B, table.data_ptr(), _lib.stream_ptr()),
                   "pcm_convert_items")


def _rows(x: torch.Tensor, dtype, what: str) -> torch.Tensor:
    _lib.require_cuda(x, what)
    if x.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {x.dtype}")
    if x.ndim not in (1, 2):
        raise ValueError(f"{what}: expected (n,) or (B, n), got {tuple(x.shape)}")
    return x.contiguous()


def _convert_rows(x: torch.Tensor, dtype) -> torch.Tensor:
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    xs, ys = (x[None], y[None]) if x.ndim == 1 else (x, y)
    if x.numel():
        for a in range(0, xs.shape[0], MAX_ITEMS):                 # one item per row; a launch takes 65535 of them
            convert_items(list(xs[a:a + MAX_ITEMS].unbind(0)), list(ys[a:a + MAX_ITEMS].unbind(0)))
    return y


def from_pcm16(x: torch.Tensor) -> torch.Tensor:
    """x (B, n) or (n,) torch.int16 on the GPU -> float32 of the same shape, x / 32768 (exact).  What a caller puts in front of the
    whole-clip encode()."""
    return _convert_rows(_rows(x, torch.int16, "pcm"), torch.float32)


def to_pcm16(y: torch.Tensor) -> torch.Tensor:
    """y (B, n) or (n,) torch.float32 on the GPU -> torch.int16 of the same shape by the rounding rule of the module docstring.
    What a caller puts behind the whole-clip decode()."""
    return _convert_rows(_rows(y, torch.float32, "waveform"), torch.int16)
