"""One vocoder pass over mel windows of different lengths: BigVGAN.forward(x, lengths) / dmel_bigvgan_forward_items, the per-item
conv_post (dmel_conv_post_items_f32) and VQGAN.decode(..., item_audio=True).

Every comparison is torch.equal against the call that existed before: forward() on the item alone, cut to its own length.  The mel
holds NaN at and beyond each item's length, so a single read of the padding by any layer shows in the audio.

Shapes.  The tiny generators have 32 / 16 / 8 (or 16 / 8 / 4) channels: one or two 32-row tiles, so the split kernels run their
32 x 256 tile (conv_pre, every AMP convolution, the second up stage) and their 64 x 128 tile (the first up stage: two phases of 32
rows) -- pick_tile_bf16 in conv_igemm.hip.  The activation's tile is 1008 outputs.  Lengths in mel frames, batch [Tmax, 1, 2, 0, k]:
  (129, 127)  one frame on either side of 128: the 128-column tile of the first up stage (Tcols = frames), and for the x4 x2 models
              508 | 516 around 2 x 256 at stage 1, 1016 | 1032 around 4 x 256 at the output rate
  (127, 125)  x4 x2 models: 1000 | 1016 output samples, either side of the 1008-sample activation tile (126 frames)
  (253, 251)  1004 | 1012 around 1008 at stage 1 of the x4 x2 models and at the output rate of the x2 x2 model"""
import math

import pytest
import torch

from test_gpu_conv_matrix import check, lib, stream

pytestmark = pytest.mark.gpu

PAIRS = [(129, 127), (127, 125), (253, 251)]
PRECISIONS = ["fp32", "fp32_bf16x3", "bf16"]
# AMPBlock1 snakebeta logscale / AMPBlock1 snake, no weight norm, no tanh, no bias / AMPBlock2 / AMPBlock1 snakebeta in linear scale
MODELS = ["bigvgan_tiny", "bigvgan_tiny_snake_nowm", "bigvgan_tiny_ampblock2", "bigvgan_tiny_linscale"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_lengths_sit_on_both_sides_of_the_tiles():
    for up, first in ((8, 4), (4, 2)):
        stages = lambda n: (n, n * first, n * up)
        assert stages(127)[0] < 128 < stages(129)[0]
        if up == 8:
            assert stages(127)[1] < 512 < stages(129)[1] and stages(127)[2] < 1024 < stages(129)[2]
            assert stages(125)[2] < 1008 < stages(127)[2] and stages(251)[1] < 1008 < stages(253)[1]
        else:
            assert stages(251)[2] < 1008 < stages(253)[2]


_MODELS = {}


def model(name, golden, dev):
    if name not in _MODELS:
        from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
        from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
        gd = golden("bigvgan_tiny" if name == "bigvgan_tiny_linscale" else name)
        h = AttrDict(dict(gd.meta["h"]))
        if name == "bigvgan_tiny_linscale":
            h["snake_logscale"] = False
        m = BigVGAN(h)
        if name.endswith("nowm"):
            m.remove_weight_norm()
        m.load_state_dict(gd.sd)
        if name == "bigvgan_tiny_linscale":        # the same convolutions; alpha and beta as a linear-scale model holds them, in [0.5, 1.5)
            g = torch.Generator().manual_seed(31)
            with torch.no_grad():
                for pname, p in m.named_parameters():
                    if pname.split(".")[-1] in ("alpha", "beta"):
                        p.copy_(torch.rand(p.shape, generator=g) + 0.5)
        _MODELS[name] = (m.to(dev), h)
    return _MODELS[name]


def batch(h, pair, dev):
    """mel (5, num_mels, Tmax) with NaN at and beyond each item's length, and the lengths [Tmax, 1, 2, 0, k]"""
    tmax, k = pair
    lens = [tmax, 1, 2, 0, k]
    g = torch.Generator().manual_seed(1000 * tmax + k)
    mel = torch.randn(5, h.num_mels, tmax, generator=g)
    for b, n in enumerate(lens):
        mel[b, :, n:] = float("nan")
    return mel.to(dev), lens


_REFS = {}


def singles(name, precision, pair, m, mel, lens):
    """forward() on every item alone: computed once per (model, precision, lengths) and shared"""
    key = (name, precision, pair)
    if key not in _REFS:
        m.set_streams(3)
        _REFS[key] = [m(mel[b:b + 1, :, :n]).clone() if n else None for b, n in enumerate(lens)]
    return _REFS[key]


def hold_items(y, want, lens, up, what):
    assert y.shape == (len(lens), 1, max(lens) * up)
    bad = []
    for b, n in enumerate(lens):
        if n:
            if not bool(torch.isfinite(y[b, :, :n * up]).all()):
                bad.append(f"item {b} (len {n}): non-finite audio")
            elif not torch.equal(y[b:b + 1, :, :n * up], want[b]):
                d = y[b:b + 1, :, :n * up] != want[b]
                first = int(d.flatten().nonzero()[0])
                bad.append(f"item {b} (len {n}): {int(d.sum())} of {d.numel()} samples differ from the item alone, first at {first}")
        if not bool((y[b, :, n * up:] == 0).all()):
            bad.append(f"item {b} (len {n}): {int((y[b, :, n * up:] != 0).sum())} samples behind its end are not 0")
    assert not bad, what + ": " + "; ".join(bad)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", MODELS)
def test_items_equal_each_item_alone(dev, golden, name, precision):
    m, h = model(name, golden, dev)
    up = math.prod(h.upsample_rates)
    m.set_precision(precision)
    try:
        for pair in PAIRS:
            mel, lens = batch(h, pair, dev)
            want = singles(name, precision, pair, m, mel, lens)
            for streams in (1, 3):
                m.set_streams(streams)
                y = m(mel, lengths=lens)
                hold_items(y, want, lens, up, f"{name} {precision} {pair} streams {streams}")
                assert y.grad_fn is None
            # lengths that already live on the GPU are not read by the host
            y = m(mel, lengths=torch.tensor(lens, dtype=torch.int64, device=dev))
            hold_items(y, want, lens, up, f"{name} {precision} {pair} device lengths")
    finally:
        m.set_streams(3)
        m.set_precision("fp32")


def test_fused_activation_stands_aside(dev, golden, monkeypatch):
    """DMEL_FUSE_SNAKE=1 asks for the act -> conv kernel, which has one row length per batch: under lengths it is not taken"""
    m, h = model("bigvgan_tiny", golden, dev)
    mel, lens = batch(h, PAIRS[0], dev)
    want = singles("bigvgan_tiny", "fp32", PAIRS[0], m, mel, lens)
    monkeypatch.setenv("DMEL_FUSE_SNAKE", "1")
    hold_items(m(mel, lengths=lens), want, lens, math.prod(h.upsample_rates), "fused env")


def test_equal_lengths_and_the_plain_call_agree(dev, golden):
    """every item as long as the pitch: the items pass has the bits of the plain batched call"""
    m, h = model("bigvgan_tiny_ampblock2", golden, dev)
    mel = torch.randn(3, h.num_mels, 130, generator=torch.Generator().manual_seed(5)).to(dev)
    assert torch.equal(m(mel, lengths=[130] * 3), m(mel))


# ------------------------------------------------------------------------------------ conv_post over items
def test_conv_post_items(dev):
    Cc, K, T = 4, 7, 1025 + 3
    lens = [0, 1, 3, 1024, 1025]
    g = torch.Generator().manual_seed(8)
    w = (torch.randn(Cc, K, generator=g) * 0.2).to(dev)
    x = torch.randn(len(lens), Cc, T, generator=g)
    for b, n in enumerate(lens):
        x[b, :, n:] = float("nan")
    x = x.to(dev)
    ld = torch.tensor(lens, dtype=torch.int64, device=dev)
    for act in (0, 2, 3):
        y = torch.full((len(lens), 1, T), -777.0, device=dev)
        check(lib().dmel_conv_post_items_f32(x.data_ptr(), w.data_ptr(), 0.3, act, y.data_ptr(), len(lens), Cc, K, T, ld.data_ptr(), stream()),
              "conv_post_items")
        for b, n in enumerate(lens):
            if n:
                xi = x[b:b + 1, :, :n].contiguous()
                yi = torch.empty(1, 1, n, device=dev)
                check(lib().dmel_conv_post_f32(xi.data_ptr(), w.data_ptr(), 0.3, act, yi.data_ptr(), 1, Cc, K, n, stream()), "conv_post")
                assert torch.equal(y[b:b + 1, :, :n], yi), (act, b, n)
            assert bool((y[b, :, n:] == 0).all()), (act, b, n)


# ------------------------------------------------------------------------------------ refusals
def test_refusals(dev, golden):
    m, h = model("bigvgan_tiny", golden, dev)
    mel = torch.randn(2, h.num_mels, 12, device=dev)
    for bad in ([12], [1, 2, 3], [13, 1], [-1, 4], [1.5, 2], torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0]),
                torch.tensor([1, 2], dtype=torch.int32, device=dev), torch.tensor([1, 2, 3], device=dev)):
        with pytest.raises(ValueError, match="lengths"):
            m(mel, lengths=bad)
    with pytest.raises(NotImplementedError, match="gradient"):
        m(mel.clone().requires_grad_(), lengths=[12, 3])
    with torch.no_grad():
        assert m(mel.clone().requires_grad_(), lengths=[12, 3]).shape == (2, 1, 96)       # no grad asked for: served
    # C ABI: a workspace one byte short is refused and nothing is written, neither the audio nor the workspace
    from dmel_codec_amd import _lib
    L = _lib.lib()
    with torch.cuda.device(dev):
        hd = m.native()
        need = L.dmel_bigvgan_items_workspace_bytes(hd, 2, 12)
        assert need >= L.dmel_bigvgan_workspace_bytes(hd, 2, 12) + 3 * 2 * 8
        ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
        audio = torch.full((2, 1, 96), -777.0, device=dev)
        lens = torch.tensor([12, 3], dtype=torch.int64, device=dev)
        rc = L.dmel_bigvgan_forward_items(hd, mel.data_ptr(), lens.data_ptr(), audio.data_ptr(), 2, 12, ws.data_ptr(), need - 1, _lib.stream_ptr())
        assert rc != 0 and "workspace" in L.dmel_last_error().decode()
        assert L.dmel_bigvgan_forward_items(hd, mel.data_ptr(), None, audio.data_ptr(), 2, 12, ws.data_ptr(), need, _lib.stream_ptr()) != 0
        torch.cuda.synchronize()
        assert bool((audio == -777.0).all()) and bool((ws == 0x5A).all())
        _lib.check(L.dmel_bigvgan_forward_items(hd, mel.data_ptr(), lens.data_ptr(), audio.data_ptr(), 2, 12, ws.data_ptr(), need,
                                                _lib.stream_ptr()), "bigvgan_forward_items")
        assert torch.equal(audio, m(mel, lengths=[12, 3]))
    assert L.dmel_abi_version() == 2


# ------------------------------------------------------------------------------------ decode(item_audio=True)
TINY_VOCODER = dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=64, resblock="1",
                    resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, activation="snakebeta", snake_logscale=True)


def test_decode_item_audio(dev):
    from test_gpu_parity import make_codec
    codec = make_codec(731, n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=TINY_VOCODER).to(dev)
    g = torch.Generator().manual_seed(23)
    B, T4 = 3, 40
    ids = torch.randint(0, 175, (B, 8, T4), generator=g, dtype=torch.int32).to(dev)
    flen = torch.tensor([T4, 13, 32], device=dev)
    noise = torch.randn(B, codec.decoder.input_channels, T4 * 4, generator=g).to(dev)
    audio0, mel0 = codec.decode(ids, flen, return_audios=True, noise=noise)
    audio, mel = codec.decode(ids, flen, return_audios=True, noise=noise, item_audio=True)
    assert torch.equal(mel, mel0) and audio.shape == audio0.shape
    assert torch.equal(audio0, codec.vocoder(mel0))                    # the default: the reference's audio of the padded mel, bit for bit
    up = audio.shape[-1] // mel.shape[-1]
    differs = False
    for b, n4 in enumerate(flen.tolist()):
        n = 4 * n4
        assert torch.equal(audio[b:b + 1, :, :n * up], codec.vocoder(mel[b:b + 1, :, :n])), b
        assert bool((audio[b, :, n * up:] == 0).all()), b
        differs |= not torch.equal(audio[b], audio0[b])
    assert differs                                                     # the padded call's tails do depend on the padding
