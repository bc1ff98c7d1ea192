"""The single-segment K loop of the fp16-split convolution kernel (conv_bf16_kernel<TAPS > 0>, conv_igemm.hip) against the generic one.

The specialised loop keeps the generic loop's K order, MFMA order, accumulators, staging split and epilogue, so every output must be
bit-identical: each case runs once with the default dispatch and once with DMEL_CONV_SPEC=0 (read per call) and compares with torch.equal.
Covered: every taps x dilation of the vocoder's AMP blocks on every routed tile (forced with DMEL_CONV_TILE_BF16) and the automatic choice,
T not a multiple of any tile, the LINEAR epilogue with residual, accumulate and out_div (whole BigVGANs), RESSKIP with ragged in / out
lengths (the WaveNet's residual / skip 1x1 convolution), a BigVGAN-base forward and a whole decode()."""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
F16X2 = 3                        # DMEL_PRECISION_FP32_F16X2: the fp16-split kernel (NP = 2)
SPEC_TILES = [None, 1, 2, 3, 6, 7]   # automatic, 128x96, 64x128, 32x256, 128x64, 256x96


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def lib():
    from dmel_codec_amd import _lib
    return _lib.lib()


def check(rc, what=""):
    from dmel_codec_amd import _lib
    _lib.check(rc, what)


def stream():
    from dmel_codec_amd import _lib
    return _lib.stream_ptr()


def both(monkeypatch, fn):
    """fn() with the default dispatch and with DMEL_CONV_SPEC=0; both results cloned after a synchronise."""
    out = []
    for spec in ("1", "0"):
        monkeypatch.setenv("DMEL_CONV_SPEC", spec)
        y = fn()
        torch.cuda.synchronize()
        out.append(y.clone())
    monkeypatch.delenv("DMEL_CONV_SPEC")
    return out


def set_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    else:
        monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))


# ------------------------------------------------------------------------------------ single convolutions through the C ABI
# (Cout, Cin, k, dilation, T, B): every (k, dilation) of the AMP blocks (halo 2 .. 50: both staging classes), Cin ragged against the
# 16-channel K step, T ragged against every tile width and below the halo
CONV_SHAPES = [(cout, cin, k, d, T, 2) for (cout, cin, T) in [(128, 64, 1000), (64, 40, 333)] for k in (3, 7, 11) for d in (1, 3, 5)]
CONV_SHAPES += [(256, 128, 7, 5, 97, 3), (32, 17, 11, 5, 31, 1)]


def shape_id(s):
    Cout, Cin, k, dil, T, B = s
    return f"{Cout}x{Cin}k{k}d{dil}-T{T}-B{B}"


@pytest.mark.parametrize("tile", SPEC_TILES, ids=lambda t: "auto" if t is None else f"tile{t}")
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=shape_id)
def test_conv_spec_is_bit_identical(dev, monkeypatch, shape, tile):
    Cout, Cin, k, dil, T, B = shape
    g = torch.Generator().manual_seed(Cout * 31 + Cin * 7 + k * 5 + dil * 3 + T)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(B, Cin, T, generator=g).to(dev)
    y = torch.empty(B, Cout, T, device=dev)
    h = C.c_void_p()
    check(lib().dmel_conv_create(C.byref(h), w.data_ptr(), b.data_ptr(), Cout, Cin, k, dil), "dmel_conv_create")
    try:
        check(lib().dmel_conv_set_precision(h, F16X2))
        monkeypatch.setenv("DMEL_CONV_PC", "0")
        set_tile(monkeypatch, tile)

        def run():
            y.fill_(float("nan"))
            check(lib().dmel_conv_forward(h, x.data_ptr(), y.data_ptr(), B, T, stream()), shape_id(shape))
            return y
        ys, yg = both(monkeypatch, run)
    finally:
        lib().dmel_conv_destroy(h)
    assert bool(torch.isfinite(ys).all())
    assert torch.equal(ys, yg), float((ys - yg).abs().max())


# ------------------------------------------------------------------------------------ modules: epilogue modes
@pytest.mark.parametrize("tile", SPEC_TILES, ids=lambda t: "auto" if t is None else f"tile{t}")
@pytest.mark.parametrize("name", ["bigvgan_tiny", "bigvgan_tiny_ampblock2"])
def test_bigvgan_spec_is_bit_identical(dev, golden, monkeypatch, name, tile):
    """Residual add, accumulate and out_div of the AMP branch sums (LINEAR epilogue), every routed tile."""
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
    gd = golden(name)
    m = BigVGAN(AttrDict(dict(gd.meta["h"])))
    m.load_state_dict(gd.sd)
    m = m.to(dev)
    mel = gd.ins["mel"].to(dev)
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    set_tile(monkeypatch, tile)
    ys, yg = both(monkeypatch, lambda: m(mel))
    assert torch.equal(ys, yg), float((ys - yg).abs().max())
    assert rel_err(ys, gd.outs["audio"]) < TOL


@pytest.mark.parametrize("tile", [None, 1], ids=["auto", "tile1"])
def test_wavenet_resskip_spec_is_bit_identical(dev, monkeypatch, tile):
    """RESSKIP (residual / skip with skip accumulation) with ragged in / out lengths, an empty item included; tile 1 routes the 1x1
    residual / skip convolution to the single-segment loop."""
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    torch.manual_seed(71)
    m = WaveNet(input_channels=64, output_channels=24, residual_channels=64, residual_layers=4, dilation_cycle=4, condition_channels=64)
    g = torch.Generator().manual_seed(72)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("weight_g"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    m.set_precision("fp32_f16x2")
    m = m.to(dev)
    T, lens = 300, torch.tensor([300, 177, 0, 299])
    x, c = torch.randn(4, 64, T, generator=g).to(dev), torch.randn(4, 64, T, generator=g).to(dev)
    ld = lens.to(dev)
    monkeypatch.setenv("DMEL_WAVENET_FUSED", "0")
    monkeypatch.setenv("DMEL_WAVENET_PRESPLIT", "0")
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    set_tile(monkeypatch, tile)
    ys, yg = both(monkeypatch, lambda: m(x, condition=c, in_lengths=ld, out_lengths=ld))
    assert torch.equal(ys, yg), float((ys - yg).abs().max())
    assert bool((ys[2] == 0).all())


# ------------------------------------------------------------------------------------ the bench codec
@pytest.fixture(scope="module")
def codec(dev):
    from dmel_codec_amd.configs import build_codec
    torch.manual_seed(114514)
    c = build_codec(sample_rate=24000, n_mels=80, dmel_groups=8, levels=(7, 5, 5), vocoder="base_24k_100band", f_max=None)
    g = torch.Generator().manual_seed(114515)
    with torch.no_grad():
        for name, p in c.vocoder.named_parameters():
            if name.endswith("weight_v"):
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
            elif name.endswith("weight_g"):
                p.fill_(1.0)
    return c.eval().to(dev)


def test_bigvgan_base_forward_spec_is_bit_identical(dev, monkeypatch, codec):
    g = torch.Generator().manual_seed(5)
    mel = (torch.randn(2, codec.vocoder.h.num_mels, 80, generator=g) * 0.5).to(dev)
    monkeypatch.delenv("DMEL_CONV_PC", raising=False)
    monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    with torch.no_grad():
        ys, yg = both(monkeypatch, lambda: codec.vocoder(mel))
    assert bool(torch.isfinite(ys).all())
    assert torch.equal(ys, yg), float((ys - yg).abs().max())


def test_decode_spec_is_bit_identical(dev, monkeypatch, codec):
    g = torch.Generator().manual_seed(6)
    audio = (torch.randn(3, 1, 24000, generator=g) * 0.3).to(dev)
    lens = torch.tensor([24000, 17000, 9001], device=dev)
    monkeypatch.delenv("DMEL_CONV_PC", raising=False)
    monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    with torch.no_grad():
        ids, il = codec.encode(audio, lens)

        def run():
            torch.manual_seed(7)          # decode() draws Gaussian noise
            wav, _ = codec.decode(ids, il, return_audios=True)
            return wav
        ys, yg = both(monkeypatch, run)
    assert bool(torch.isfinite(ys).all())
    assert torch.equal(ys, yg), float((ys - yg).abs().max())
