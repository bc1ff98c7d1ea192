"""The sample format of the wire on the MI355X: 16-bit signed PCM or 8-bit G.711 (mu-law, A-law) <-> fp32 (csrc/small_ops.hip:
pcm_convert_kernel, through dmel_pcm_convert_items).  Microphones, RTP, WebSocket audio and sound cards carry int16, telephony (PSTN
gateways, SIP trunks, RTP payload types 0 and 8) carries G.711 at 8 kHz; the codec computes in fp32.

The rounding rule, written down once:

    s16 -> f32   y = x / 32768                                      exact; full scale is -1.0, the largest value 1 - 2^-15
    f32 -> s16   y = round_half_even(clamp(x * 32768, -32768, 32767))
                 the product is exact (a power of two); ties go to the EVEN integer (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -1.5 -> -2),
                 as torch.round and numpy.rint do -- not truncation, not round-half-away, not a scale of 32767; NaN -> 0, +-inf
                 saturate; no dither, so the result is deterministic.  On the CPU:
                 clamp(round(nan_to_num(y, nan=0) * 32768), -32768, 32767).to(int16)

The companding rule, written down once: ITU-T G.711 as Sun's g711.c and CPython's audioop restate it.  Integer arithmetic on the s16
value x (>> is an arithmetic shift), so every check of it is an equality of bits:

    mu-law encode   v = x >> 2; neg = v < 0; m = min((neg ? -v : v) + 33, 8191); seg = floor(log2(m)) - 5       (0 .. 7)
                    code = ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF)
    mu-law decode   u = ~code & 0xFF; t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4); x = (u & 0x80) ? 0x84 - t : t - 0x84
    A-law encode    v = x >> 3; neg = v < 0; m = neg ? -v - 1 : v; seg = max(floor(log2(max(m, 1))) - 4, 0)
                    mant = seg < 2 ? (m >> 1) & 15 : (m >> seg) & 15; code = ((seg << 4) | mant) ^ (neg ? 0x55 : 0xD5)
    A-law decode    a = code ^ 0x55; t = (a & 15) << 4; seg = (a & 0x70) >> 4; t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1)
                    x = (a & 0x80) ? t : -t
    law -> f32      y = decode(code) / 32768                        exact
    f32 -> law      code = encode(the f32 -> s16 rule above, unchanged): NaN and 0.0 give 0xFF (mu-law) and 0xD5 (A-law)

encode(decode(c)) == c for all 256 A-law codes and for every mu-law code but 0x7F ("negative zero": it decodes to 0, which encodes as
0xFF).  law <-> s16 and law <-> law are not served.

The channel rule, written down once.  The codec is mono; sound cards, WAV, RTP L16 and WebRTC deliver INTERLEAVED frames, usually
stereo (telephony call recordings put one party on the left channel and the other on the right), and a playback device opened as
stereo wants stereo frames.  An interleaved piece of n frames and c channels is a contiguous (n, c) array: frame i, channel j is
element i * c + j.  1 <= c <= 8.

    downmix (c -> 1)    each channel's sample goes to f32 by its format's rule above (s16: x / 32768; law: decode / 32768; f32: the
                        value itself); then acc = x_0; acc += x_1; ... acc += x_{c-1} in fp32, in channel order; then
                        y = acc / (float)c, the IEEE correctly rounded fp32 division -- NOT a multiply by a rounded reciprocal.
                        Bit for bit numpy.mean(y, axis=0) of the channel-first float32 array, which is what librosa's to_mono
                        computes (the reference loads its clips with librosa.load(..., mono=True)).  acc * float32(1 / c) differs
                        from it for c = 3, 5, 6, 7, torch.mean(dim=-1) of the interleaved array for c = 5, 6, 7, numpy.mean over
                        the contiguous last axis for c = 8: the oracle is the explicit left-to-right sum and a division, nothing
                        shorter.  For s16 and law sources the channel values and their sum are exact in fp32 (at most 16 + 3
                        bits): the result is the fp64 mean rounded once.  Nothing is sanitised: an f32 NaN or inf propagates.
    pick (c -> 1, k)    y = x_k converted by its format's rule, no arithmetic; for f32 the word is untouched.  Two sessions pushed
                        the same stereo tensor, one with channel=0 and one with channel=1, are the two parties of a call recording.
    fan-out (1 -> c)    the mono sample is converted ONCE by the f32 -> format rule above and stored c times, frame by frame; for
                        f32 -> f32 the word is copied.

Not served, refused: c -> c' with both above 1, weights, channel maps, more than 8 channels, planar (channel-first) pieces.  One side
of every conversion is still f32: stereo s16 -> mono s16 is refused like s16 -> s16.

from_pcm16 / to_pcm16, from_g711 / to_g711 and downmix / fan_out convert a whole tensor, convert_items any list of ragged pieces, each in ONE launch.  The
session pools (models/stream_sessions.py) fold the same launch into the per-slot copies they make anyway:
open(sample_format="s16" | "ulaw" | "alaw", channels=c[, channel=k]).

Out of scope: other formats (s24, s32, u8), law <-> s16 transcoding, packet-loss concealment and dither."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .. import _lib

# sample_format -> (DMEL_SAMPLE_* of include/dmel_hip.h, dtype)
FORMATS = {"f32": (0, torch.float32), "s16": (1, torch.int16), "ulaw": (8, torch.uint8), "alaw": (9, torch.uint8)}
LAWS = ("ulaw", "alaw")
_INFER = {torch.float32: "f32", torch.int16: "s16"}                # torch.uint8 alone does not say which law
MAX_ITEMS = 65535
MAX_CHANNELS = 8                                                   # DMEL_MAX_CHANNELS of include/dmel_hip.h


def check_format(sample_format) -> str:
    if sample_format not in FORMATS:
        raise ValueError(f"unknown sample format {sample_format!r}: expected one of {sorted(FORMATS)}")
    return sample_format


def _formats(pieces, names, what: str):
    """the format name of every piece: the one the caller gave, else the one its dtype implies (None: no format has that dtype)"""
    if names is not None and len(names) != len(pieces):
        raise ValueError(f"{what}_formats names {len(names)} pieces, expected {len(pieces)}")
    out = []
    for i, t in enumerate(pieces):
        name = None if names is None else names[i]
        if name is None:
            if t.dtype == torch.uint8:
                raise ValueError(f"item {i}: a torch.uint8 {what} is mu-law or A-law: name it ({what}_formats=, one of {list(LAWS)})")
            name = _INFER.get(t.dtype)
        elif t.dtype != FORMATS[check_format(name)][1]:
            raise ValueError(f"item {i}: a {what} of format {name!r} is {FORMATS[name][1]}, got {t.dtype}")
        out.append(name)
    return out


def _channel_tables(B: int, src_channels, dst_channels, src_pick):
    """the three per-item channel tables as lists of int (defaults: 1, 1, -1), refused here as dmel_pcm_convert_items_ch refuses them"""
    tabs = []
    for name, t, default in (("src_channels", src_channels, 1), ("dst_channels", dst_channels, 1), ("src_pick", src_pick, -1)):
        if t is None:
            t = [default] * B
        elif len(t) != B:
            raise ValueError(f"{name} names {len(t)} pieces, expected {B}")
        tabs.append([default if v is None else int(v) for v in t])
    for i, (sc, dc, k) in enumerate(zip(*tabs)):
        if not (1 <= sc <= MAX_CHANNELS and 1 <= dc <= MAX_CHANNELS):
            raise ValueError(f"item {i}: channel counts {sc} -> {dc}, expected 1 .. {MAX_CHANNELS}")
        if sc > 1 and dc > 1:
            raise ValueError(f"item {i}: {sc} -> {dc} channels is not served: one side is mono")
        if k != -1 and not (sc > 1 and 0 <= k < sc):
            raise ValueError(f"item {i}: channel {k} of a source with {sc} channel(s): expected None (the mean)"
                             + (f" or 0 .. {sc - 1}" if sc > 1 else ""))
    return tabs


def _piece_ok(t: torch.Tensor, n: int, c: int) -> bool:
    """a mono piece is 1-D with contiguous samples; a piece of c > 1 channels is (n, c) with strides (c, 1)"""
    if c == 1:
        return t.ndim == 1 and t.shape[0] == n and (n <= 1 or t.stride(0) == 1)
    return t.ndim == 2 and tuple(t.shape) == (n, c) and (n == 0 or t.stride(1) == 1) and (n <= 1 or t.stride(0) == c)


@torch.no_grad()
def convert_items(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], table: Optional[torch.Tensor] = None,
                  src_formats: Optional[Sequence[Optional[str]]] = None, dst_formats: Optional[Sequence[Optional[str]]] = None,
                  src_channels: Optional[Sequence[Optional[int]]] = None, dst_channels: Optional[Sequence[Optional[int]]] = None,
                  src_pick: Optional[Sequence[Optional[int]]] = None) -> None:
    """dsts[i][:] = convert(srcs[i]) for lists of 1-D CUDA tensors with contiguous samples, in ONE launch: s16 -> f32, f32 -> s16 (the
    rounding rule of the module docstring), f32 -> f32 (a copy), ulaw / alaw -> f32 and f32 -> ulaw / alaw (the companding rule of
    the module docstring); s16 -> s16, law <-> s16 and law <-> law are refused.  src_formats / dst_formats: the name of each piece's
    format (utils/pcm.py: FORMATS; an entry may be None); by default a piece's dtype says it, float32 or int16 -- a torch.uint8 piece
    must be named, because its dtype does not say which law.  Pieces may have any lengths, 0 included, and any alignment; no
    destination may overlap a source or another destination.  table: device scratch of 4 * len(srcs) int64 a caller that converts
    every step keeps (default: allocated here).  Runs on the current stream.

    Interleaved channels (the channel rule of the module docstring): src_channels / dst_channels name each piece's channel count
    (None, or an entry None: 1).  A piece with c > 1 channels is a 2-D (n, c) tensor with strides (c, 1) and its partner is 1-D of
    length n: a source of c channels is downmixed -- the mean, or channel src_pick[i] of it -- into its mono f32 destination, a mono
    f32 source is fanned out into all c channels of its destination.  c -> c' with both above 1 is refused."""
    B = len(srcs)
    if B != len(dsts) or not 1 <= B <= MAX_ITEMS:
        raise ValueError(f"expected as many destinations as sources, 1 .. {MAX_ITEMS} of them (got {B} and {len(dsts)})")
    sf, df = _formats(srcs, src_formats, "source"), _formats(dsts, dst_formats, "destination")
    sc, dc, pick = _channel_tables(B, src_channels, dst_channels, src_pick)
    dev = srcs[0].device
    for i, (x, y) in enumerate(zip(srcs, dsts)):
        _lib.require_cuda(x, "source")
        _lib.require_cuda(y, "destination")
        if sf[i] is None or df[i] is None:
            raise ValueError(f"item {i}: {x.dtype} -> {y.dtype}: samples are torch.int16, torch.float32 or (named) torch.uint8")
        if sc[i] == 1 and dc[i] == 1:
            if x.ndim != 1 or y.ndim != 1 or x.shape != y.shape or (x.shape[0] > 1 and (x.stride(0) != 1 or y.stride(0) != 1)):
                raise ValueError(f"item {i}: expected two 1-D tensors of equal length with contiguous samples, got {tuple(x.shape)} "
                                 f"(stride {x.stride()}) -> {tuple(y.shape)} (stride {y.stride()})")
        elif x.ndim == 0 or not (_piece_ok(x, x.shape[0], sc[i]) and _piece_ok(y, x.shape[0], dc[i])):
            raise ValueError(f"item {i}: {sc[i]} -> {dc[i]} channels: expected an interleaved (n, c) piece with strides (c, 1) and a "
                             f"1-D partner of length n, got {tuple(x.shape)} (stride {x.stride()}) -> {tuple(y.shape)} "
                             f"(stride {y.stride()})")
        if x.device != dev or y.device != dev:
            raise ValueError(f"item {i}: all pieces must live on one device")
    if table is None:
        table = torch.empty(4 * B, dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or table.numel() < 4 * B or table.device != dev or not table.is_contiguous():
        raise ValueError(f"table must hold {4 * B} contiguous int64 on {dev}")
    P, I32, I64 = C.c_void_p * B, C.c_int32 * B, C.c_int64 * B
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_pcm_convert_items_ch(P(*[x.data_ptr() for x in srcs]), I32(*[FORMATS[f][0] for f in sf]), I32(*sc),
                                                        I32(*pick), P(*[y.data_ptr() for y in dsts]), I32(*[FORMATS[f][0] for f in df]),
                                                        I32(*dc), I64(*[x.shape[0] for x in srcs]), B, table.data_ptr(),
                                                        _lib.stream_ptr()),
                   "pcm_convert_items")


def convert_packed(srcs: Sequence[torch.Tensor], formats: Sequence[str], channels: Sequence[int],
                   table: Optional[torch.Tensor] = None) -> list:
    """mono f32 pieces -> each in its format and fanned out into its channels, all by ONE convert_items launch into one packed buffer
    of bytes, each piece at a multiple of 16 of them.  -> the destinations: views of that buffer in the format's dtype, (n,) for
    one channel and interleaved frames (n, c) for c > 1"""
    at, total = [], 0
    for y, f, c in zip(srcs, formats, channels):
        size = y.shape[0] * c * FORMATS[f][1].itemsize
        at.append((total, size))
        total += (size + 15) // 16 * 16
    packed = torch.empty(total, dtype=torch.uint8, device=srcs[0].device)
    dsts = [packed[a:a + size].view(FORMATS[f][1]) for (a, size), f in zip(at, formats)]
    dsts = [d if c == 1 else d.view(-1, c) for d, c in zip(dsts, channels)]
    convert_items(srcs, dsts, table=table, dst_formats=formats, dst_channels=channels)
    return dsts


def _rows(x: torch.Tensor, dtype, what: str) -> torch.Tensor:
    _lib.require_cuda(x, what)
    if x.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {x.dtype}")
    if x.ndim not in (1, 2):
        raise ValueError(f"{what}: expected (n,) or (B, n), got {tuple(x.shape)}")
    return x.contiguous()


def _convert_rows(x: torch.Tensor, src_format: str, dst_format: str, src_channels: Optional[int] = None,
                  dst_channels: Optional[int] = None, pick: int = -1) -> torch.Tensor:
    """x: contiguous rows (n,) / (B, n), with the channels as one more, last axis where src_channels names them (1 included) -> the
    converted rows, with such an axis where dst_channels names them.  One item per row; a launch takes 65535 of them."""
    frames = tuple(x.shape if src_channels is None else x.shape[:-1])
    sc, dc = src_channels or 1, dst_channels or 1
    y = torch.empty(frames if dst_channels is None else frames + (dc,), dtype=FORMATS[dst_format][1], device=x.device)
    if x.numel():
        rows = (-1, frames[-1])                                    # a 1-channel row is a view of its samples, a mono piece
        xs, ys = x.view(rows if sc == 1 else rows + (sc,)), y.view(rows if dc == 1 else rows + (dc,))
        for a in range(0, xs.shape[0], MAX_ITEMS):
            k = min(MAX_ITEMS, xs.shape[0] - a)
            convert_items(list(xs[a:a + k].unbind(0)), list(ys[a:a + k].unbind(0)), src_formats=[src_format] * k,
                          dst_formats=[dst_format] * k, src_channels=[sc] * k, dst_channels=[dc] * k, src_pick=[pick] * k)
    return y


def from_pcm16(x: torch.Tensor) -> torch.Tensor:
    """x (B, n) or (n,) torch.int16 on the GPU -> float32 of the same shape, x / 32768 (exact).  What a caller puts in front of the
    whole-clip encode()."""
    return _convert_rows(_rows(x, torch.int16, "pcm"), "s16", "f32")


def to_pcm16(y: torch.Tensor) -> torch.Tensor:
    """y (B, n) or (n,) torch.float32 on the GPU -> torch.int16 of the same shape by the rounding rule of the module docstring.
    What a caller puts behind the whole-clip decode()."""
    return _convert_rows(_rows(y, torch.float32, "waveform"), "f32", "s16")


def _check_law(law) -> str:
    if law not in LAWS:
        raise ValueError(f"unknown companding law {law!r}: expected one of {list(LAWS)}")
    return law


def from_g711(x: torch.Tensor, law: str) -> torch.Tensor:
    """x (B, n) or (n,) torch.uint8 on the GPU, G.711 codes of `law` ("ulaw" | "alaw") -> float32 of the same shape, decode(code) /
    32768 (exact).  What a caller puts in front of the whole-clip encode(..., sample_rate=8000)."""
    return _convert_rows(_rows(x, torch.uint8, "g711"), _check_law(law), "f32")


def to_g711(y: torch.Tensor, law: str) -> torch.Tensor:
    """y (B, n) or (n,) torch.float32 on the GPU -> torch.uint8 G.711 codes of `law` ("ulaw" | "alaw") of the same shape: the s16
    rounding rule, then the companding rule of the module docstring.  What a caller puts behind the whole-clip decode()."""
    return _convert_rows(_rows(y, torch.float32, "waveform"), "f32", _check_law(law))


def _check_channels(channels) -> int:
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"channels={channels!r}: expected an int in 1 .. {MAX_CHANNELS}")
    return channels


def check_channel(channel, channels: int) -> int:
    """the pick of a c-channel source as the C entry takes it: None -> -1 (the mean), else 0 .. c - 1 (and c > 1)"""
    if channel is None:
        return -1
    if isinstance(channel, bool) or not isinstance(channel, int) or channels == 1 or not 0 <= channel < channels:
        raise ValueError(f"channel={channel!r} of {channels} channel(s): expected None (the mean)"
                         + (f" or 0 .. {channels - 1}" if channels > 1 else ""))
    return channel


def downmix(x: torch.Tensor, sample_format: Optional[str] = None, channel: Optional[int] = None) -> torch.Tensor:
    """x (n, c) or (B, n, c) on the GPU, interleaved frames of c = 1 .. 8 channels -> mono float32 (n,) / (B, n) by the channel rule of
    the module docstring: the mean over the channels (channel=None) or channel `channel` of every frame.  sample_format: by default the
    dtype says it as in convert_items (float32 or int16); torch.uint8 must be named ("ulaw" | "alaw").  One launch per 65535 rows.
    What a caller puts in front of the whole-clip encode()."""
    fmt = _formats([x], None if sample_format is None else [sample_format], "source")[0]
    if fmt is None:
        raise ValueError(f"{x.dtype}: samples are torch.int16, torch.float32 or (named) torch.uint8")
    if x.ndim not in (2, 3):
        raise ValueError(f"expected interleaved frames (n, c) or (B, n, c), got {tuple(x.shape)}")
    c = x.shape[-1]
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"{c} channels: expected 1 .. {MAX_CHANNELS} (interleaved frames, channels last)")
    pick = check_channel(channel, c)
    _lib.require_cuda(x, "audio")
    return _convert_rows(x.contiguous(), fmt, "f32", src_channels=c, pick=pick)


def fan_out(y: torch.Tensor, channels: int, sample_format: str = "f32") -> torch.Tensor:
    """y (n,) or (B, n) float32 on the GPU -> interleaved frames (n, c) / (B, n, c) of the format's dtype: every sample converted once
    by the f32 -> format rule of the module docstring and stored in all c = `channels` channels of its frame.  One launch per 65535
    rows.  What a caller puts behind the whole-clip decode()."""
    c = _check_channels(channels)
    check_format(sample_format)
    return _convert_rows(_rows(y, torch.float32, "waveform"), "f32", sample_format, dst_channels=c)
