"""dmel_crossfade_items through the C ABI (csrc/small_ops.hip): per row, F samples inside an audio buffer blended in place with the
row's tail, and F other samples of the buffer saved as the new tail, one launch for all rows.  Every comparison is torch.equal against
the torch expression old + w * (new - old) on CPU fp32 tensors, over the WHOLE buffers: every element outside the rows' regions must
be what it was."""
import pytest
import torch

from dmel_codec_amd.utils import crossfade

pytestmark = pytest.mark.gpu

PITCH = 4096                                           # floats per row of the audio buffer; a multiple of 4: rows start 16-byte aligned
KINDS = ("both", "blend", "save")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def values(shape, g):
    """mixed signs, exact zeros of both signs, and runs where neighbours are equal"""
    x = torch.randn(shape, generator=g)
    hole = torch.rand(shape, generator=g)
    x[hole < 0.1] = 0.0
    x[(hole >= 0.1) & (hole < 0.15)] = -0.0
    return x


def run(dev, F, R, offsets, seed):
    """R rows, row r of kind KINDS[r % 3], its pointers offset by offsets[r % len(offsets)] floats from 16-byte alignment"""
    g = torch.Generator().manual_seed(seed)
    wav, tails, w = values((R, PITCH), g), values((R, 520), g), torch.zeros(R, 520)
    for r in range(R):
        off = offsets[r % len(offsets)]
        w[r, off:off + F] = crossfade.weights(F)
        if r % 2:                                      # where both versions agree the blend must return `old`, bit for bit
            wav[r, 8 + off:8 + off + F] = tails[r, off:off + F]
    d_wav, d_tails, d_w = wav.to(dev), tails.to(dev), w.to(dev)
    want_wav, want_tails = wav.clone(), tails.clone()
    rows = []
    for r in range(R):
        off, kind = offsets[r % len(offsets)], KINDS[r % 3]
        a, s = 8 + off, 8 + off + F + 4 * (r % 2)      # the save region starts at or behind the end of the blend region
        old, wr = tails[r, off:off + F], w[r, off:off + F]
        if kind != "save":
            want_wav[r, a:a + F] = old + wr * (wav[r, a:a + F] - old)
        if kind != "blend":
            want_tails[r, off:off + F] = wav[r, s:s + F]
        rows.append((d_wav[r, a:a + F] if kind != "save" else None, d_tails[r, off:off + F],
                     d_wav[r, s:s + F] if kind != "blend" else None, d_w[r, off:off + F]))
    crossfade.crossfade_items(rows)
    torch.cuda.synchronize()
    assert torch.equal(d_wav.cpu(), want_wav), f"audio differs (F {F}, R {R}, offsets {offsets})"
    assert torch.equal(d_tails.cpu(), want_tails), f"tails differ (F {F}, R {R}, offsets {offsets})"
    assert torch.equal(d_w.cpu(), w), "the weights were written"
    if R > 1:
        assert torch.equal(want_wav[1, 8 + offsets[1 % len(offsets)]:][:F], tails[1, offsets[1 % len(offsets)]:][:F])


@pytest.mark.parametrize("F", [1, 3, 4, 255, 256, 512])
@pytest.mark.parametrize("R", [1, 5])
def test_rows_equal_the_torch_expression_and_touch_nothing_else(dev, F, R):
    # all rows aligned (16 bytes per lane where F is a multiple of 4), all rows one float off (4 bytes per lane), and both kinds of
    # row side by side in one launch
    for n, offsets in enumerate([(0,), (1,), (0, 1), (1, 0)]):
        run(dev, F, R, offsets, seed=1000 * F + 10 * R + n)


def test_every_kind_of_row_alone(dev):
    """R = 1 puts KINDS[0] in the launch; here each kind is the only row of its launch, at both alignments"""
    g = torch.Generator().manual_seed(5)
    for F in (4, 255, 512):
        for off in (0, 1):
            for kind in KINDS:
                wav, tail, w = values((PITCH,), g), values((520,), g), crossfade.weights(F)
                d_wav, d_tail, d_w = wav.to(dev), tail.to(dev), torch.zeros(520).to(dev)
                d_w[off:off + F] = w.to(dev)
                a, s = 12 + off, 12 + off + F
                want_wav, want_tail = wav.clone(), tail.clone()
                if kind != "save":
                    want_wav[a:a + F] = tail[off:off + F] + w * (wav[a:a + F] - tail[off:off + F])
                if kind != "blend":
                    want_tail[off:off + F] = wav[s:s + F]
                crossfade.crossfade_items([(d_wav[a:a + F] if kind != "save" else None, d_tail[off:off + F],
                                            d_wav[s:s + F] if kind != "blend" else None, d_w[off:off + F])])
                assert torch.equal(d_wav.cpu(), want_wav) and torch.equal(d_tail.cpu(), want_tail), (F, off, kind)


def test_fades_of_more_than_one_tile(dev):
    """a workgroup covers 1024 elements of a row: the entry's longest fade and an odd one just above a tile, rows of both alignments
    and a short row beside them in one launch (the grid is sized by the longest row)"""
    g = torch.Generator().manual_seed(7)
    fades = [(4096, 0), (1027, 1), (4096, 1), (3, 0), (2048, 0)]
    n = 2 * 4096 + 16
    wav, tails, w = values((len(fades), n), g), values((len(fades), 4100), g), torch.zeros(len(fades), 4100)
    want_wav, want_tails = wav.clone(), tails.clone()
    for r, (F, off) in enumerate(fades):
        w[r, off:off + F] = crossfade.weights(F)
    d_wav, d_tails, d_w = wav.to(dev), tails.to(dev), w.to(dev)
    rows = []
    for r, (F, off) in enumerate(fades):
        a, s = 4 + off, 4 + off + F
        old = tails[r, off:off + F]
        want_wav[r, a:a + F] = old + w[r, off:off + F] * (wav[r, a:a + F] - old)
        want_tails[r, off:off + F] = wav[r, s:s + F]
        rows.append((d_wav[r, a:a + F], d_tails[r, off:off + F], d_wav[r, s:s + F], d_w[r, off:off + F]))
    crossfade.crossfade_items(rows)
    assert torch.equal(d_wav.cpu(), want_wav) and torch.equal(d_tails.cpu(), want_tails) and torch.equal(d_w.cpu(), w)


def test_refusals_leave_every_buffer_alone(dev):
    g = torch.Generator().manual_seed(6)
    wav, tail, w = values((PITCH,), g).to(dev), values((64,), g).to(dev), crossfade.weights(64).to(dev)
    before = wav.clone(), tail.clone()
    with pytest.raises(RuntimeError, match="row 1.*neither"):
        crossfade.crossfade_items([(wav[:64], tail, wav[64:128], w), (None, tail, None, w)])
    with pytest.raises(ValueError, match="row 0"):
        crossfade.crossfade_items([(wav[:32], tail, None, w)])             # a region of another length than the tail
    with pytest.raises(ValueError):
        crossfade.crossfade_items([])
    torch.cuda.synchronize()
    assert torch.equal(wav, before[0]) and torch.equal(tail, before[1])
