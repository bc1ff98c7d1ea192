"""The full-tile epilogue and the interior x staging of the fp16-split convolution kernels (conv_dev.h epi_full_tile, conv_bf16_kernel<NP = 2>::
store_x, the producer waves of conv_pc_kernel) against the edge code they bypass.

A tile whose 32 rows and 32 NT columns lie inside the output takes an epilogue without clamps, masks and selects, with the launch-uniform
flags (residual, running sum, 1 / out_div) resolved outside the row loop; a staged item whose columns and channels all exist is scaled and
split as packed fp32 without validity selects.  Both evaluate the expressions of the edge code in the same order, so every output must be
BIT-IDENTICAL to a run with DMEL_CONV_FASTPATH=0 (read per call), which sends every tile and every item through the edge code.  Each case runs
twice in one process, forced-edge and default, into NaN-prefilled guarded buffers (test_gpu_conv_matrix.Out / In): torch.equal, and the
default run within the per-element float64 bound of test_gpu_conv_matrix (its helper, its tau for the fp16 split; no tolerance of this
module's own).

Reference of the epilogue options (dmel_conv_forward_ex): ref = ((accumulate ? y_prev : 0) + conv1d(x, w) + b + residual) / out_div in float64,
scale A = (conv1d(|x|, |w|) + |b| + |y_prev| + |residual|) / out_div: the two extra additions and the division round once each, at 2^-24 of a
partial sum that A bounds -- far inside tau = 1.2e-6, so the bound of the plain convolution holds unchanged.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_matrix as M
from conftest import rel_err

pytestmark = pytest.mark.gpu

F16X2 = 3                               # DMEL_PRECISION_FP32_F16X2: the fp16-split kernels (NP = 2)
MODE = "fwd NP=2"
# tile -> its column width BN, one tile per width pick_tile_bf16 can choose at NP = 2: 128 x 64, 128 x 96, 64 x 128, 32 x 256
TILE_BN = {6: 64, 1: 96, 2: 128, 3: 256}
TAPS = [(1, 1), (3, 1), (3, 5), (7, 3), (11, 5)]      # halo 0, 2, 10, 18, 50: the 0-, 16- and 64-column staging classes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def route(monkeypatch, tile=None, pc="0"):
    """Kernel choice of the next launches: a forced conv_bf16_kernel tile or the automatic one; DMEL_CONV_PC=2 also sends small launches of
    >= 160 rows with taps to the producer / consumer kernel."""
    monkeypatch.setenv("DMEL_CONV_PC", pc)
    if tile is None:
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    else:
        monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))


def operands(Cout, Cin, k, T, B, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(B, Cin, T, generator=g)
    res = torch.randn(B, Cout, T, generator=g)
    yprev = torch.randn(B, Cout, T, generator=g)
    return w, b, x, res, yprev


def reference(w, b, x, dil, res=None, yprev=None, div=1.0):
    """float64 result and error scale of dmel_conv_forward_ex (module docstring)."""
    pad = dil * (w.shape[2] - 1) // 2
    ref = F.conv1d(x.double(), w.double(), b.double(), dilation=dil, padding=pad)
    A = F.conv1d(x.double().abs(), w.double().abs(), None, dilation=dil, padding=pad) + b.double().abs()[None, :, None]
    for extra in (res, yprev):
        if extra is not None:
            ref = ref + extra.double()
            A = A + extra.double().abs()
    return ref / div, A / div


def run_both(dev, monkeypatch, w, b, x, dil, what, res=None, yprev=None, div=1.0, in_len=None, out_len=None, fold=(0, 0)):
    """The launch with DMEL_CONV_FASTPATH=0 and with the switch unset, each into a fresh guarded output (prefilled with y_prev when the launch
    accumulates, with NaN otherwise).  Returns (edge, fast)."""
    B, Cin, T = x.shape
    Cout = w.shape[0]
    conv = M.Conv(w, b, dil)
    outs = []
    try:
        M.check(M.lib().dmel_conv_set_precision(conv.h, F16X2))
        xd = M.In(x, dev)
        rd = M.In(res, dev) if res is not None else None
        il = in_len.to(dev) if in_len is not None else None
        ol = out_len.to(dev) if out_len is not None else None
        for fast in ("0", None):
            if fast is None:
                monkeypatch.delenv("DMEL_CONV_FASTPATH", raising=False)
            else:
                monkeypatch.setenv("DMEL_CONV_FASTPATH", fast)
            y = M.Out((B, Cout, T), dev)
            if yprev is not None:
                y.t.copy_(yprev)
            M.check(M.lib().dmel_conv_forward_ex(conv.h, xd.ptr(), y.ptr(), B, T, rd.ptr() if rd is not None else None, 1 if yprev is not None else 0,
                                                 C.c_float(div), il.data_ptr() if il is not None else None, ol.data_ptr() if ol is not None else None,
                                                 fold[0], fold[1], M.stream()), what)
            outs.append(y.check(f"{what} fastpath={fast}").clone())
            xd.check(what)
            if rd is not None:
                rd.check(what)
    finally:
        monkeypatch.delenv("DMEL_CONV_FASTPATH", raising=False)
        conv.close()
    return outs


def assert_bound(y, ref, A, what):
    """test_gpu_conv_matrix's per-element bound (its ratio() and its tau), without entering this module's cases into that module's report."""
    r = M.ratio(y, ref, A)
    print(f"{what}: max |y - ref| / A = {r:.3e} (tau {M.TAU[MODE]:.2e})")
    assert r <= M.TAU[MODE], f"{what}: max |y - ref| / A = {r:.3e} > tau {M.TAU[MODE]:.2e} ({MODE})"


def assert_same_and_bounded(edge, fast, ref, A, what):
    assert torch.equal(fast, edge), (what, float((fast - edge).abs().max()))
    assert_bound(fast, ref, A, what)


# ------------------------------------------------------------------------------------ columns: every tile width, every kind of last tile
@pytest.mark.parametrize("tsel", ["7", "BN-1", "BN", "BN+1", "2BN+5"])
@pytest.mark.parametrize("tile", sorted(TILE_BN), ids=lambda t: f"tile{t}")
def test_columns(dev, monkeypatch, tile, tsel):
    """A tile that is all edge (T = 7), exact fits, a one-column last tile beside an interior one, two full tiles and a ragged third."""
    BN = TILE_BN[tile]
    T = {"7": 7, "BN-1": BN - 1, "BN": BN, "BN+1": BN + 1, "2BN+5": 2 * BN + 5}[tsel]
    w, b, x, _, _ = operands(64, 32, 3, T, 2, 1000 + tile * 10 + T)
    route(monkeypatch, tile)
    what = f"columns tile {tile} T {T}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, 1, what)
    assert_same_and_bounded(edge, fast, *reference(w, b, x, 1), what)


# ------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("Cout", [32, 40, 64, 96, 160, 256])
def test_rows(dev, monkeypatch, Cout):
    """Full and partial 32-row tiles side by side (40: the second tile has 8 rows and takes the edge code); 160 and 256 rows run on the
    producer / consumer kernel (DMEL_CONV_PC=2: also at this size), the others on the automatic conv_bf16_kernel tile."""
    T = 2 * 96 + 5
    w, b, x, _, _ = operands(Cout, 32, 3, T, 2, 2000 + Cout)
    route(monkeypatch, None, "2")
    what = f"rows Cout {Cout}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, 1, what)
    assert_same_and_bounded(edge, fast, *reference(w, b, x, 1), what)


# ------------------------------------------------------------------------------------ channels x taps, on both staging codes
@pytest.mark.parametrize("k,dil", TAPS, ids=lambda v: str(v))
@pytest.mark.parametrize("Cin", [8, 24, 32, 80])
@pytest.mark.parametrize("kernel", ["bf16", "pc"])
def test_channels_and_taps(dev, monkeypatch, kernel, Cin, k, dil):
    """Cin 8 (less than a 16-channel chunk), 24 and 80 (a last chunk with missing channels), 32 (whole chunks), with every halo class.
    bf16: 64 rows on the automatic tile (64 x 128; T = 129: an interior tile and a one-column one); pc: 160 rows on the producer / consumer
    kernel (T = 2 * 96 + 5), which refuses pointwise convolutions -- those fall to conv_bf16_kernel's 128 x 96 tile."""
    Cout, T = (64, 129) if kernel == "bf16" else (160, 2 * 96 + 5)
    w, b, x, _, _ = operands(Cout, Cin, k, T, 2, 3000 + Cin * 100 + k * 10 + dil + (7 if kernel == "pc" else 0))
    route(monkeypatch, None, "0" if kernel == "bf16" else "2")
    what = f"channels {kernel} Cin {Cin} k {k} d {dil}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, dil, what)
    assert_same_and_bounded(edge, fast, *reference(w, b, x, dil), what)


@pytest.mark.parametrize("k,dil", TAPS, ids=lambda v: str(v))
@pytest.mark.parametrize("kernel", ["bf16", "pc"])
def test_halo_wider_than_the_row(dev, monkeypatch, kernel, k, dil):
    """T = 7: every staged column of the halo-16 and halo-64 classes beyond the seventh is padding."""
    Cout = 64 if kernel == "bf16" else 160
    w, b, x, _, _ = operands(Cout, 32, k, 7, 3, 3500 + k * 10 + dil)
    route(monkeypatch, None, "0" if kernel == "bf16" else "2")
    what = f"short row {kernel} k {k} d {dil}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, dil, what)
    assert_same_and_bounded(edge, fast, *reference(w, b, x, dil), what)


# ------------------------------------------------------------------------------------ epilogue flags
@pytest.mark.parametrize("div", [1.0, 3.0], ids=["div1", "div3"])
@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("with_res", [0, 1], ids=["nores", "res"])
@pytest.mark.parametrize("kernel", ["bf16", "pc"])
def test_epilogue_combinations(dev, monkeypatch, kernel, with_res, acc, div):
    """Residual x running sum x out_div: the eight instantiations of epi_full_tile next to edge tiles (T = 2 * 96 + 5, a partial row tile at
    72 / 168 rows).  accumulate with out_div = 3 and a residual is the last convolution of a vocoder stage: (y_prev + conv + res) / 3."""
    Cout = 72 if kernel == "bf16" else 168
    T = 2 * 96 + 5
    w, b, x, res, yprev = operands(Cout, 32, 3, T, 2, 4000 + with_res * 4 + acc * 2 + int(div))
    res = res if with_res else None
    yprev = yprev if acc else None
    route(monkeypatch, None, "0" if kernel == "bf16" else "2")
    what = f"epilogue {kernel} res {with_res} acc {acc} div {div}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, 1, what, res=res, yprev=yprev, div=div)
    assert_same_and_bounded(edge, fast, *reference(w, b, x, 1, res, yprev, div), what)


# ------------------------------------------------------------------------------------ ragged items
@pytest.mark.parametrize("lens", ["0,T-1", "1,T"])
@pytest.mark.parametrize("tile", sorted(TILE_BN), ids=lambda t: f"tile{t}")
def test_ragged_items(dev, monkeypatch, tile, lens):
    """in_len = out_len per item in {0, 1, T - 1, T}, T = BN + 1: input columns behind the length read as zero, output columns at or behind it
    are exactly 0, the others equal the forced-edge run and meet the bound of a convolution over the masked input."""
    BN = TILE_BN[tile]
    T = BN + 1
    ln = torch.tensor({"0,T-1": [0, T - 1], "1,T": [1, T]}[lens], dtype=torch.int64)
    w, b, x, _, _ = operands(64, 32, 3, T, 2, 5000 + tile * 10 + int(ln[0]))
    route(monkeypatch, tile)
    what = f"ragged tile {tile} lens {ln.tolist()}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, 1, what, in_len=ln, out_len=ln)
    mask = (torch.arange(T)[None, :] < ln[:, None])[:, None, :]
    ref, A = reference(w, b, x * mask, 1)
    for i, n in enumerate(ln.tolist()):
        assert bool((fast[i, :, n:] == 0).all()) and bool((edge[i, :, n:] == 0).all()), (what, i)
        assert torch.equal(fast[i, :, :n], edge[i, :, :n]), (what, i)
    assert torch.equal(fast, edge), what
    assert_bound(fast, ref * mask, A, what)


# ------------------------------------------------------------------------------------ folded batch
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 5)], ids=lambda v: str(v))
def test_folded_batch(dev, monkeypatch, k, dil):
    """The decoder WaveNet's folded form: 3 items x 20 frames side by side in one row at a pitch of 27 columns, zero columns between them.  A
    folded launch takes no full-tile epilogue: gap columns are exactly 0, the rest equals the forced-edge run and meets the bound."""
    N, valid, P = 3, 20, 27
    T = N * P
    w, b, x, _, _ = operands(96, 64, k, T, 1, 6000 + dil)
    gap = (torch.arange(T) % P) >= valid
    x[:, :, gap] = 0.0
    route(monkeypatch, None)
    what = f"folded k {k} d {dil}"
    edge, fast = run_both(dev, monkeypatch, w, b, x, dil, what, fold=(P, valid))
    ref, A = reference(w, b, x, dil)
    ref[:, :, gap] = 0.0
    assert bool((fast[:, :, gap] == 0).all()), what
    assert_same_and_bounded(edge, fast, ref, A, what)


# ------------------------------------------------------------------------------------ whole networks
def both_switches(monkeypatch, fn):
    out = []
    for fast in ("0", None):
        if fast is None:
            monkeypatch.delenv("DMEL_CONV_FASTPATH", raising=False)
        else:
            monkeypatch.setenv("DMEL_CONV_FASTPATH", fast)
        y = fn()
        torch.cuda.synchronize()
        out.append(y.clone())
    return out


def test_whole_networks(dev, golden, monkeypatch):
    """dmel_bigvgan_forward (the tiny BigVGAN fixture: residual, running sum and out_div of the AMP blocks, transposed-conv phases) and
    dmel_wavenet_forward on the layered path (the tiny conditioned WaveNet of test_gpu_conv_matrix: GATE, RESSKIP, ragged lengths with an
    empty item): torch.equal with the switch off and on, and inside the parity bar."""
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
    monkeypatch.delenv("DMEL_CONV_PC", raising=False)
    monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    g = golden("bigvgan_tiny")
    voc = BigVGAN(AttrDict(dict(g.meta["h"])))
    voc.load_state_dict(g.sd)
    voc = voc.to(dev)
    mel = g.ins["mel"].to(dev)
    edge, fast = both_switches(monkeypatch, lambda: voc(mel))
    assert torch.equal(fast, edge), float((fast - edge).abs().max())
    assert rel_err(fast, g.outs["audio"]) < M.TOL

    m, x, c, lens, ref = M.wavenet_case()
    m = m.to(dev)
    xd, cd, ld = x.to(dev), c.to(dev), lens.to(dev)
    monkeypatch.setenv("DMEL_WAVENET_FUSED", "0")
    monkeypatch.setenv("DMEL_WAVENET_PRESPLIT", "0")
    edge, fast = both_switches(monkeypatch, lambda: m(xd, condition=cd, in_lengths=ld, out_lengths=ld))
    assert torch.equal(fast, edge), float((fast - edge).abs().max())
    assert rel_err(fast, ref) < M.TOL
