"""The G.711 companding rule of dmel_codec_amd/utils/pcm.py restated in numpy on the CPU: what the GPU conversions are held to, bit for
bit.  Integer arithmetic on the s16 value; tests/test_g711_cpu.py checks this restatement against CPython's audioop (where it exists),
against values pinned by hand and against the round-trip property, so that the GPU tests compare against something that was itself
compared."""
import numpy as np
import torch

LAWS = ("ulaw", "alaw")
NEUTRAL = {"ulaw": 0xFF, "alaw": 0xD5}                 # what 0 (and NaN) encode to

# (s16 value, code) and (code, s16 value) pinned by hand from the rule
HAND_ENCODE = {"ulaw": [(-32768, 0x00), (-32124, 0x00), (-4, 0x7E), (-3, 0x7E), (-1, 0x7E), (0, 0xFF), (3, 0xFF), (4, 0xFE),
                        (131, 0xEF), (132, 0xEF), (32123, 0x80), (32767, 0x80)],
               "alaw": [(-32768, 0x2A), (-9, 0x55), (-1, 0x55), (0, 0xD5), (8, 0xD5), (511, 0xCA), (512, 0xF5), (32767, 0xAA)]}
HAND_DECODE = {"ulaw": [(0x00, -32124), (0x7F, 0), (0x80, 32124), (0xFF, 0)],
               "alaw": [(0x55, -8), (0xD5, 8), (0x2A, -32256), (0xAA, 32256)]}


def _floor_log2(m: np.ndarray) -> np.ndarray:
    """floor(log2(m)) for m >= 1, by comparison with the powers of two (no floating point)"""
    return (m[..., None] >= (1 << np.arange(1, 16))).sum(-1)


def encode(x, law: str) -> np.ndarray:
    """s16 values (any integer array-like in -32768 .. 32767) -> uint8 codes"""
    x = np.asarray(x).astype(np.int32)
    assert x.min(initial=0) >= -32768 and x.max(initial=0) <= 32767
    if law == "ulaw":
        v = x >> 2
        neg = v < 0
        m = np.minimum(np.where(neg, -v, v) + 33, 8191)
        seg = _floor_log2(m) - 5
        assert seg.min(initial=0) >= 0 and seg.max(initial=0) <= 7
        code = ((seg << 4) | ((m >> (seg + 1)) & 15)) ^ np.where(neg, 0x7F, 0xFF)
    elif law == "alaw":
        v = x >> 3
        neg = v < 0
        m = np.where(neg, -v - 1, v)
        seg = np.maximum(_floor_log2(np.maximum(m, 1)) - 4, 0)
        mant = np.where(seg < 2, (m >> 1) & 15, (m >> seg) & 15)
        code = ((seg << 4) | mant) ^ np.where(neg, 0x55, 0xD5)
    else:
        raise ValueError(law)
    assert code.min(initial=0) >= 0 and code.max(initial=0) <= 255
    return code.astype(np.uint8)


def decode(code, law: str) -> np.ndarray:
    """uint8 codes -> s16 values as int16"""
    c = np.asarray(code).astype(np.int32)
    assert c.min(initial=0) >= 0 and c.max(initial=0) <= 255
    if law == "ulaw":
        u = ~c & 0xFF
        t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
        x = np.where(u & 0x80, 0x84 - t, t - 0x84)
    elif law == "alaw":
        a = c ^ 0x55
        t = (a & 15) << 4
        seg = (a & 0x70) >> 4
        t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
        x = np.where(a & 0x80, t, -t)
    else:
        raise ValueError(law)
    return x.astype(np.int16)


def f32_to_s16(y: torch.Tensor) -> torch.Tensor:
    """the s16 rounding rule of utils/pcm.py on the CPU (torch.round rounds halves to even)"""
    y = y.detach().cpu().float()
    return torch.clamp(torch.round(torch.nan_to_num(y, nan=0.0) * 32768), -32768, 32767).to(torch.int16)


def f32_to_law(y: torch.Tensor, law: str) -> torch.Tensor:
    """float32 tensor -> uint8 codes: the s16 rounding rule, then encode"""
    return torch.from_numpy(encode(f32_to_s16(y).numpy(), law))


def law_to_f32(code: torch.Tensor, law: str) -> torch.Tensor:
    """uint8 codes -> float32, decode(code) / 32768 (exact)"""
    return torch.from_numpy(decode(code.detach().cpu().numpy(), law)).float() / 32768


def segment_edges(law: str):
    """the s16 values at which the code's segment changes, on both sides of zero, found from encode() itself over all 65536 values"""
    x = np.arange(-32768, 32768)
    seg = (encode(x, law) ^ NEUTRAL[law]) & 0xF0
    return [int(v) for v in x[1:][seg[1:] != seg[:-1]]]
