"""The channel rule of dmel_codec_amd/utils/pcm.py restated on the CPU: what the GPU conversions are held to, bit for bit.  An
interleaved piece is an (n, c) array, frame i, channel j at element i * c + j.

    downmix   every channel to f32 by its format's rule; acc = x_0; acc += x_1; ...; y = acc / float32(c) -- numpy's float32 division,
              which is the IEEE one.  Deliberately the explicit left-to-right sum and a division: numpy.mean over the last axis,
              torch.mean and a multiply by float32(1 / c) all differ from it for some c (tests/test_channels_cpu.py shows where).
    pick      channel k by its format's rule, no arithmetic
    fan-out   the mono sample converted once by the f32 -> format rule and repeated c times

tests/test_channels_cpu.py checks this restatement against values pinned by hand, against numpy.mean(axis=0) of the channel-first array
(what librosa's to_mono computes) and, for the integer formats, against the fp64 mean rounded once."""
import numpy as np
import torch

import g711_ref

DTYPE = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


def to_f32(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """samples of format `fmt`, any shape -> float32 on the CPU by the format's rule (exact for s16 and the laws)"""
    x = x.detach().cpu()
    assert x.dtype == DTYPE[fmt], (x.dtype, fmt)
    if fmt == "f32":
        return x.clone()
    if fmt == "s16":
        return x.float() / 32768
    return g711_ref.law_to_f32(x, fmt)


def from_f32(y: torch.Tensor, fmt: str) -> torch.Tensor:
    """float32, any shape -> samples of format `fmt` on the CPU by the f32 -> format rule"""
    y = y.detach().cpu()
    assert y.dtype == torch.float32
    if fmt == "f32":
        return y.clone()
    return g711_ref.f32_to_s16(y) if fmt == "s16" else g711_ref.f32_to_law(y, fmt)


def downmix(x: torch.Tensor, fmt: str, channel=None) -> torch.Tensor:
    """x (n, c) of format `fmt` -> float32 (n,): the mean in channel order (channel=None) or channel `channel`"""
    assert x.ndim == 2 and 1 <= x.shape[1] <= 8
    y = to_f32(x, fmt).numpy()
    if channel is not None:
        return torch.from_numpy(y[:, channel].copy())
    acc = y[:, 0].copy()
    for j in range(1, y.shape[1]):
        acc = acc + y[:, j]                                        # float32 + float32, one rounding each
    assert acc.dtype == np.float32
    with np.errstate(all="ignore"):
        return torch.from_numpy(acc / np.float32(y.shape[1]))


def fan_out(y: torch.Tensor, channels: int, fmt: str) -> torch.Tensor:
    """y (n,) float32 -> (n, channels) of format `fmt`: converted once, stored `channels` times"""
    assert y.ndim == 1
    return from_f32(y, fmt)[:, None].repeat(1, channels).contiguous()


def words(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t
