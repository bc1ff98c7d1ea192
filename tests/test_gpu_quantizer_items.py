"""One quantiser pass over windows of different lengths: DownsampleFiniteScalarQuantize.encode(z, lengths=) / .decode(ids, lengths=)
(dmel_quantizer_encode_items / dmel_quantizer_decode_items), the per-item depthwise conv + LayerNorm behind them
(dmel_convnext_forward_items) and VQGAN.get_quantized_features_from_indices(..., item_features=True).

Every comparison is torch.equal against the call that existed before: encode() / decode() on the item alone, cut to its own length.
The features hold NaN at and behind each item's length, so a single read of the padding by any layer shows in the ids; ids cannot hold
NaN, so the decode batches run twice, the padding filled with 0 and with the largest code, and must not differ.  Every ConvNeXt gamma
is N(0, 0.5): at the constructor's 1e-6 the reach of the depthwise k = 7 convolution across an item's end would be invisible.

Tiles: kDwTile = 32 columns in dwconv_ln (small_ops.hip), the 128- and 256-column tiles of the split convolution kernels
(pick_tile_bf16 in conv_igemm.hip), 256 threads in the FSQ kernels.  Lengths per stage, longest | second longest item of a batch:
  encode (134, 126): 134|126  67|63   33|31      (262, 250): 262|250 131|125  65|62      (518, 506): 518|506 259|253 129|126
  decode  (33, 31):   33|31   66|62  132|124      (65, 63):   65|63  130|126 260|252      (129, 127): 129|127 258|254 516|508"""
import ctypes as C
import math

import pytest
import torch

from test_gpu_parity import make_codec, randomise

pytestmark = pytest.mark.gpu

G, CG = 10, 70
ENC_PAIRS = [(134, 126), (262, 250), (518, 506)]
DEC_PAIRS = [(33, 31), (65, 63), (129, 127)]
CONFIGS = [([7, 5, 5], True), ([7, 5, 5], False), ([8, 6], True), ([8, 6], False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_lengths_sit_on_both_sides_of_the_tiles():
    down = lambda n: (n, n // 2, n // 4)
    up = lambda n: (n, 2 * n, 4 * n)
    for (tmax, k), edges in zip(ENC_PAIRS, [(128, 64, 32), (256, 128, 64), (512, 256, 128)]):
        assert all(b < e < a for a, b, e in zip(down(tmax), down(k), edges)), (tmax, k)
    for (tmax, k), edges in zip(DEC_PAIRS, [(32, 64, 128), (64, 128, 256), (128, 256, 512)]):
        assert all(b < e < a for a, b, e in zip(up(tmax), up(k), edges)), (tmax, k)
    assert [down(n) for n in (7, 5, 3)] == [(7, 3, 1), (5, 2, 1), (3, 1, 0)]          # the floors of the strided convolutions
    assert all(e % 32 == 0 for e in (32, 64, 128, 256, 512))                            # every edge is also an edge of the 32-column tile


_Q = {}


def quantizer(levels, prebound, dev):
    key = (tuple(levels), prebound)
    if key not in _Q:
        from dmel_codec_amd.models.modules.dowmsample_fsq import DownsampleFiniteScalarQuantize
        q = DownsampleFiniteScalarQuantize(input_dim=G * CG, n_codebooks=1, n_groups=G, levels=levels, downsample_factor=(2, 2),
                                           is_dmel=True, fsq_prebound=prebound)
        randomise(q, 5 + len(levels), scale=1.5)
        gen = torch.Generator().manual_seed(77)
        with torch.no_grad():
            for m in q.modules():
                if hasattr(m, "gamma"):
                    m.gamma.copy_(torch.randn(m.gamma.shape, generator=gen) * 0.5)
        _Q[key] = q.to(dev)
    return _Q[key]


def feature_batch(pair, dev):
    """z (7 * G, CG, Tmax) with NaN at and behind each item's length, and the lengths [Tmax, 4, 7, 5, 3, 0, k]"""
    tmax, k = pair
    lens = [tmax, 4, 7, 5, 3, 0, k]
    g = torch.Generator().manual_seed(1000 * tmax + k)
    z = torch.randn(len(lens) * G, CG, tmax, generator=g)
    for b, n in enumerate(lens):
        z[b * G:(b + 1) * G, :, n:] = float("nan")
    return z.to(dev), lens


def check_encode(q, z, lens, ids):
    assert ids.dtype == torch.int32 and ids.shape == (len(lens), G, z.shape[2] // 4)
    for b, n in enumerate(lens):
        assert not bool(ids[b, :, n // 4:].any()), (b, n)
        if n >= 4:
            alone = q.encode(z[b * G:(b + 1) * G, :, :n].contiguous())
            assert alone.shape == (1, G, n // 4)
            assert torch.equal(ids[b, :, :n // 4], alone[0]), (b, n, int((ids[b, :, :n // 4] != alone[0]).sum()))


@pytest.mark.parametrize("strict", [False, True], ids=["fp32", "strict"])
@pytest.mark.parametrize("levels,prebound", CONFIGS, ids=lambda v: "".join(map(str, v)) if isinstance(v, list) else str(v)[0])
@pytest.mark.parametrize("pair", ENC_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_encode_items_equal_each_item_alone(dev, pair, levels, prebound, strict):
    q = quantizer(levels, prebound, dev)
    q.strict_encode = strict
    try:
        z, lens = feature_batch(pair, dev)
        ids = q.encode(z, lengths=lens)
        check_encode(q, z, lens, ids)
        assert len(torch.unique(ids[0])) > 20                                          # many codes take part
    finally:
        q.strict_encode = False


def test_encode_lengths_on_the_device_and_beyond_T(dev):
    q = quantizer([7, 5, 5], True, dev)
    z, lens = feature_batch((134, 126), dev)
    ref = q.encode(z, lengths=lens)
    assert torch.equal(q.encode(z, lengths=torch.tensor(lens, dtype=torch.int64, device=dev)), ref)
    assert torch.equal(q.encode(z, lengths=torch.tensor(lens, dtype=torch.int32)), ref)          # a CPU integer tensor
    # device lengths are not read by the host: beyond T (and below 0) they are clamped on the device
    g = torch.Generator().manual_seed(3)
    full = torch.randn(3 * G, CG, 134, generator=g).to(dev)
    at_t = q.encode(full, lengths=[134, 134, 0])
    assert torch.equal(q.encode(full, lengths=torch.tensor([135, 10 ** 12, -5], dtype=torch.int64, device=dev)), at_t)
    assert torch.equal(at_t[:2], q.encode(full[:2 * G])) and not bool(at_t[2].any())


def token_batch(pair, n_codes, fill, dev):
    tmax, k = pair
    lens = [tmax, 1, 2, 0, k]
    g = torch.Generator().manual_seed(2000 * tmax + k)
    ids = torch.randint(0, n_codes, (len(lens), G, tmax), generator=g, dtype=torch.int32)
    for b, n in enumerate(lens):
        ids[b, :, n:] = fill
    return ids.to(dev), lens


@pytest.mark.parametrize("levels,prebound", CONFIGS, ids=lambda v: "".join(map(str, v)) if isinstance(v, list) else str(v)[0])
@pytest.mark.parametrize("pair", DEC_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_decode_items_equal_each_item_alone(dev, pair, levels, prebound):
    q = quantizer(levels, prebound, dev)
    n_codes = math.prod(levels)
    ids0, lens = token_batch(pair, n_codes, 0, dev)
    ids1, _ = token_batch(pair, n_codes, n_codes - 1, dev)
    z0, z1 = q.decode(ids0, lengths=lens), q.decode(ids1, lengths=lens)
    assert z0.shape == (len(lens), G * CG, 4 * pair[0]) and z0.dtype == torch.float32
    assert torch.equal(z0, z1)                                                         # the padding is not read
    for b, n in enumerate(lens):
        assert not bool(z0[b, :, 4 * n:].any()) and bool(torch.isfinite(z0[b]).all()), (b, n)
        if n:
            alone = q.decode(ids0[b:b + 1, :, :n].contiguous())
            assert torch.equal(z0[b, :, :4 * n], alone[0]), (b, n)
    # the plain call on the same padded batch DOES differ at the end of a shorter item: the depthwise convolutions reach across it
    plain = q.decode(ids1)
    assert not torch.equal(plain[4, :, :4 * lens[4]], z0[4, :, :4 * lens[4]])
    assert torch.equal(q.decode(ids0, lengths=torch.tensor(lens, dtype=torch.int64, device=dev)), z0)


def test_equal_lengths_equal_the_plain_call(dev):
    q = quantizer([8, 6], True, dev)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(3 * G, CG, 93, generator=g).to(dev)
    assert torch.equal(q.encode(z, lengths=[93, 93, 93]), q.encode(z))
    ids = torch.randint(0, 48, (3, G, 23), generator=g, dtype=torch.int32).to(dev)
    assert torch.equal(q.decode(ids, lengths=[23, 23, 23]), q.decode(ids))


def test_argument_errors(dev):
    q = quantizer([7, 5, 5], True, dev)
    z = torch.zeros(2 * G, CG, 12, device=dev)
    ids = torch.zeros(2, G, 3, dtype=torch.int32, device=dev)
    for bad in ([12], [12, 1, 2], [-1, 4], [13, 1], torch.tensor([1.0, 2.0]), [1.5, 2], torch.tensor([1.0, 2.0], device=dev),
                torch.tensor([1, 2], dtype=torch.int32, device=dev), torch.tensor([1, 2, 3], device=dev)):
        with pytest.raises(ValueError, match="lengths"):
            q.encode(z, lengths=bad)
    for bad in ([3], [-1, 2], [4, 1], torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError, match="lengths"):
            q.decode(ids, lengths=bad)
    with pytest.raises(ValueError, match="return_prequant"):
        q.encode(z, return_prequant=True, lengths=[12, 12])
    with pytest.raises(ValueError, match="return_prequant"):
        q.encode(z, return_latents=True, lengths=[12, 12])


def test_item_features_equal_the_single_item_call(dev):
    codec = make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(5)
        for m in codec.quantizer.modules():
            if hasattr(m, "gamma"):
                m.gamma.copy_(torch.randn(m.gamma.shape, generator=gen).to(m.gamma.device) * 0.5)
    codec.quantizer._free_native()
    lens = [33, 1, 2, 31]
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, 175, (4, 8, 33), generator=g, dtype=torch.int32).to(dev)
    wl = torch.tensor(lens, dtype=torch.int64, device=dev)
    other = ids.clone()
    for b, n in enumerate(lens):
        other[b, :, n:] = 174 - other[b, :, n:]
    z, mask = codec.get_quantized_features_from_indices(ids, wl, item_features=True)
    z2, _ = codec.get_quantized_features_from_indices(other, wl, item_features=True)
    assert torch.equal(z, z2) and mask.shape == (4, 1, 132)
    for b, n in enumerate(lens):
        alone, _ = codec.get_quantized_features_from_indices(ids[b:b + 1, :, :n].contiguous(), wl[b:b + 1])
        assert torch.equal(z[b, :, :4 * n], alone[0]), (b, n)
    padded, _ = codec.get_quantized_features_from_indices(ids, wl)                      # the reference: the padded batch
    assert not torch.equal(padded[3, :, :4 * 31], z[3, :, :4 * 31])
    # decode(): the flag reaches the quantiser, and with full lengths it changes nothing
    noise = torch.randn(4, codec.decoder.residual_channels, 132, generator=g).to(dev)
    full = torch.full((4,), 33, dtype=torch.int64, device=dev)
    assert torch.equal(codec.decode(ids, full, noise=noise, item_features=True), codec.decode(ids, full, noise=noise))
    a = codec.decode(ids, wl, noise=noise, item_features=True)
    b_ = codec.decode(other, wl, noise=noise, item_features=True)
    assert torch.equal(a[3, :, :4 * 31], b_[3, :, :4 * 31])


@pytest.mark.parametrize("T", [31, 33, 63, 65])
def test_dwconv_ln_items_against_the_plain_launch(dev, T):
    """The ConvNeXt block over rows of different lengths (dmel_convnext_forward_items: the per-item depthwise conv + LayerNorm and the two
    pointwise convolutions) against the plain launch on each row alone.  C = 70, T on either side of one and two 32-column tiles, rows
    that end inside the first tile, at a tile edge and one column beyond it, NaN behind every length."""
    from dmel_codec_amd import _lib
    from dmel_codec_amd.models.modules.firefly import ConvNeXtBlock
    m = ConvNeXtBlock(CG)
    randomise(m, 40, scale=1.5)
    with torch.no_grad():
        m.gamma.normal_(0, 0.5, generator=torch.Generator().manual_seed(2))
    m = m.to(dev)
    lens = [T, 1, 3, 4, 7, 0, min(T, 32), min(T, 33), T - 1, T - 3]
    g = torch.Generator().manual_seed(T)
    x = torch.randn(len(lens), CG, T, generator=g)
    for n, l in enumerate(lens):
        x[n, :, l:] = float("nan")
    x = x.to(dev)
    y = torch.full_like(x, -7.0)
    L = _lib.lib()
    with torch.no_grad(), torch.cuda.device(dev):
        h = m.native()
        ws = torch.empty(L.dmel_convnext_workspace_bytes(h, len(lens), T), dtype=torch.uint8, device=dev)
        ld = torch.tensor(lens, dtype=torch.int64, device=dev)
        _lib.check(L.dmel_convnext_forward_items(h, x.data_ptr(), ld.data_ptr(), y.data_ptr(), len(lens), T, ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr()), "convnext_forward_items")
        # the depthwise conv + LayerNorm alone: h1 is the first (N, C, T) block of the workspace
        h1 = ws[:len(lens) * CG * T * 4].view(torch.float32).view(len(lens), CG, T).clone()
        for n, l in enumerate(lens):
            assert not bool(y[n, :, l:].any()) and not bool(h1[n, :, l:].any()), (n, l)
            if l:
                alone = m(x[n:n + 1, :, :l].contiguous())
                assert torch.equal(y[n, :, :l], alone[0]), (n, l)
                h1_alone = m._ws.get(L.dmel_convnext_workspace_bytes(h, 1, l), dev)[:CG * l * 4].view(torch.float32).view(CG, l)
                assert torch.equal(h1[n, :, :l], h1_alone), (n, l)
