"""The vocoder's tail in one launch (dmel_snake_post_forward / _items, snake_post_kernel in aa_snake.hip): activation_post, conv_post and
tanh | clamp, and the same launches inside dmel_bigvgan_forward / _items.

  * torch.equal to dmel_aa_snake_f32 followed by dmel_conv_post_f32 (the items forms for items), tanh, clamp and none;
  * T on both sides of the kernel's 1000-output tile (1008 activation columns less a 4-column halo on either side) and of the 1008 /
    3 x 1008 seams of the activation kernel it is compared with; C = 1, 8, 32 and 33; one and three items; rows on and off the 16-byte
    boundary (T of every residue mod 4, x 4 bytes off);
  * other tap counts (1, 3, 9, 257: the generic tap loop and its widest halo), 259 taps refused;
  * items: NaN behind every item in x, zeros behind it in y, a canary around y;
  * a NaN / an infinity inside an item reaches exactly the outputs it reaches through the two launches;
  * the whole vocoder with DMEL_SNAKE_HEAD3 / DMEL_POST_FUSED unset equals both set to 0, and the profiler's launch counts drop by
    exactly two per stage (three "aa_snake" launches become one) and by one for the tail (its "aa_snake" launch goes; the one launch
    that is left is counted under "small", as conv_post was)."""
import math

import pytest
import torch

from test_gpu_conv_matrix import check, lib, stream
from test_gpu_snake_head3 import CANARY, T_LIST, p, view
from test_gpu_vocoder_ops_matrix import taps32

pytestmark = pytest.mark.gpu

POST_TILE = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_the_sizes_cover_the_seams():
    assert any(t < POST_TILE for t in T_LIST) and {1007, 1008, 1009, 2016, 2017, 3023, 3024, 3025} <= set(T_LIST)
    assert any(2 * POST_TILE < t <= 2 * POST_TILE + 17 for t in T_LIST) and any(t > 4 * POST_TILE for t in T_LIST)


def operands(dev, B, C, K, T, logscale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, T, generator=g) * 2
    draw = (lambda: torch.randn(C, generator=g) * 0.5) if logscale else (lambda: torch.rand(C, generator=g) + 0.5)
    a, b = draw(), draw()
    w = torch.randn(C, K, generator=g) * (0.5 / math.sqrt(C * K))
    return x.to(dev), a.to(dev), b.to(dev), w.to(dev)


def two_launches(dev, x, a, b, w, bias, act, logscale, lens=None):
    B, C, T = x.shape
    K = w.shape[1]
    ua = torch.full_like(x, float("nan"))
    y = torch.full((B, 1, T), CANARY, device=dev)
    t = taps32()
    if lens is None:
        check(lib().dmel_aa_snake_f32(p(x), p(ua), p(a), p(b), p(t), p(t), logscale, B, C, T, stream()), "aa_snake")
        check(lib().dmel_conv_post_f32(p(ua), p(w), bias, act, p(y), B, C, K, T, stream()), "conv_post")
    else:
        check(lib().dmel_aa_snake_items_f32(p(x), p(ua), p(a), p(b), p(t), p(t), logscale, B, C, T, p(lens), stream()), "aa_snake_items")
        check(lib().dmel_conv_post_items_f32(p(ua), p(w), bias, act, p(y), B, C, K, T, p(lens), stream()), "conv_post_items")
    return y


def one_launch(dev, x, a, b, w, bias, act, logscale, lens=None, xoff=0, yoff=0):
    B, C, T = x.shape
    K = w.shape[1]
    _, xv = view(dev, x.shape, xoff, float("nan"))
    xv.copy_(x)
    base, y = view(dev, (B, 1, T), yoff, CANARY)
    t = taps32()
    args = [p(xv), p(a), p(b), p(t), p(t), logscale, p(w), bias, act, p(y), B, C, K, T]
    if lens is None:
        check(lib().dmel_snake_post_forward(*args, stream()), "snake_post")
    else:
        check(lib().dmel_snake_post_forward_items(*args, p(lens), stream()), "snake_post_items")
    torch.cuda.synchronize()
    off = (y.data_ptr() - base.data_ptr()) // 4
    assert bool((base[:off] == CANARY).all() and (base[off + y.numel():] == CANARY).all()), "written outside the output"
    return y


def same(got, want):
    """equal bits where finite, non-finite in the same places"""
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("T", T_LIST)
def test_one_launch_has_the_bits_of_the_two(dev, T):
    bad = []
    for C in (1, 8, 32, 33):
        for B in (1, 3):
            logscale = (C + B) % 2
            x, a, b, w = operands(dev, B, C, 7, T, logscale, T * 17 + C + B)
            for act, bias in ((2, 0.1), (3, -0.2), (0, 0.0)):
                want = two_launches(dev, x, a, b, w, bias, act, logscale)
                for xoff, yoff in ((0, 0), (1, 3)):
                    got = one_launch(dev, x, a, b, w, bias, act, logscale, xoff=xoff, yoff=yoff)
                    if not torch.equal(got, want):
                        bad.append(f"C {C} B {B} act {act} offsets {xoff} {yoff}: {int((got != want).sum())} of {want.numel()} differ")
    assert not bad, f"T {T}: " + "; ".join(bad[:8])


def test_snake_and_a_clamp_that_clamps(dev):
    """beta NULL (Snake), and weights large enough that the clamp is active"""
    x, a, _, w = operands(dev, 2, 8, 7, 2500, 1, 5)
    w = w * 8
    want = two_launches(dev, x, a, None, w, 0.0, 3, 1)
    assert 0.02 < float((want.abs() == 1).float().mean()) < 0.98
    assert torch.equal(one_launch(dev, x, a, None, w, 0.0, 3, 1), want)


@pytest.mark.parametrize("K", [1, 3, 9, 257])
def test_other_tap_counts(dev, K):
    for T in (5, 999, 2 * (1008 - 2 * ((K // 2 + 3) & ~3)) + 1):
        x, a, b, w = operands(dev, 2, 5, K, T, 1, K + T)
        want = two_launches(dev, x, a, b, w, 0.05, 2, 1)
        assert torch.equal(one_launch(dev, x, a, b, w, 0.05, 2, 1), want), (K, T)


def test_refusals(dev):
    x, a, b, w = operands(dev, 1, 2, 259, 300, 1, 1)
    y = torch.zeros(1, 1, 300, device=dev)
    t = taps32()
    L = lib()
    assert L.dmel_snake_post_forward(p(x), p(a), p(b), p(t), p(t), 1, p(w), 0.0, 2, p(y), 1, 2, 259, 300, stream()) != 0
    assert b"taps" in L.dmel_last_error()
    ok = [p(x), p(a), p(b), p(t), p(t), 1, p(w), 0.0, 2, p(y), 1, 2, 7, 300]
    check(L.dmel_snake_post_forward(*ok, stream()), "snake_post")
    for i, v in ((0, None), (1, None), (6, None), (9, None), (8, 1), (12, 4), (13, 0)):      # NULL, act 1, even K, T = 0
        args = list(ok)
        args[i] = v
        assert L.dmel_snake_post_forward(*args, stream()) != 0, i
    assert L.dmel_snake_post_forward_items(*ok, None, stream()) != 0
    torch.cuda.synchronize()


LENS = [0, 1, 2, 3, 4, 999, 1000, 1001, 1004, 1008, 1009, 2000, 2001, 3025, 3028]


@pytest.mark.parametrize("pitch,xoff", [(3028, 0), (3029, 0), (3028, 1)], ids=["aligned", "odd_pitch", "x_off"])
def test_items(dev, pitch, xoff):
    B = len(LENS)
    lens = torch.tensor(LENS, dtype=torch.int64, device=dev)
    for C, act in ((32, 2), (3, 3)):
        x, a, b, w = operands(dev, B, C, 7, pitch, 1, pitch + C)
        for i, n in enumerate(LENS):
            x[i, :, n:] = float("nan")
        want = two_launches(dev, x, a, b, w, 0.1, act, 1, lens)
        got = one_launch(dev, x, a, b, w, 0.1, act, 1, lens, xoff=xoff)
        for i, n in enumerate(LENS):
            assert bool(torch.isfinite(got[i]).all()), (C, i, n)
            assert torch.equal(got[i], want[i]), (C, i, n, int((got[i] != want[i]).sum()))
            assert bool((got[i, :, n:] == 0).all()), (C, i, n)


def test_non_finite_samples_reach_the_same_outputs(dev):
    B, C, T = 3, 8, 3028
    lens_l = [T, 2017, 1003]
    lens = torch.tensor(lens_l, dtype=torch.int64, device=dev)
    x, a, b, w = operands(dev, B, C, 7, T, 1, 77)
    # the first and last column, either side of the 1000-output tile seam, the last columns of the shorter items
    spots = [(0, 0, 0), (0, 3, 500), (0, 7, 996), (0, 1, 1008), (0, 2, T - 1), (1, 0, 1000), (1, 5, 2016), (2, 4, 1002), (2, 0, 9)]
    for k, (i, c, t) in enumerate(spots):
        assert t < lens_l[i]
        x[i, c, t] = float("nan") if k % 2 == 0 else float("inf")
    xi = x.clone()
    for i, n in enumerate(lens_l):
        xi[i, :, n:] = float("nan")
    for act in (2, 0):
        for xx, ln in ((x, None), (xi, lens)):
            want = two_launches(dev, xx, a, b, w, 0.0, act, 1, ln)
            got = one_launch(dev, xx, a, b, w, 0.0, act, 1, ln)
            hit = ~torch.isfinite(want)
            assert bool(hit.any()) and float(hit.float().mean()) < 0.05          # a few columns around every spot, nothing else
            assert same(got, want), (act, ln is not None, int((torch.isnan(got) != torch.isnan(want)).sum()))


# ------------------------------------------------------------------------------------ the whole vocoder
@pytest.mark.parametrize("name", ["bigvgan_tiny", "bigvgan_tiny_ampblock2"])
def test_vocoder_with_and_without_the_one_launch_forms(dev, golden, monkeypatch, name):
    from dmel_codec_amd import _lib
    from test_gpu_vocoder_items import model
    m, h = model(name, golden, dev)
    stages = len(h.upsample_rates)
    g = torch.Generator().manual_seed(3)
    mel = torch.randn(3, h.num_mels, 131, generator=g).to(dev)
    lens = [131, 5, 126]
    m.set_streams(1)
    try:
        def run():
            out = []
            for kw in ({}, {"lengths": lens}):
                _lib.prof_reset()
                _lib.prof_enable(True)
                y = m(mel, **kw).clone()
                _lib.prof_enable(False)
                out.append((y, _lib.prof_read("aa_snake")["launches"], _lib.prof_read("small")["launches"]))
            _lib.prof_reset()
            return out
        monkeypatch.delenv("DMEL_SNAKE_HEAD3", raising=False)
        monkeypatch.delenv("DMEL_POST_FUSED", raising=False)
        fused = run()
        monkeypatch.setenv("DMEL_SNAKE_HEAD3", "0")
        monkeypatch.setenv("DMEL_POST_FUSED", "0")
        plain = run()
        monkeypatch.delenv("DMEL_POST_FUSED")
        tail_only = run()
        for (yf, sf, qf), (yp, sp, qp), (yt, st, qt) in zip(fused, plain, tail_only):
            assert torch.equal(yf, yp) and torch.equal(yt, yp) and bool(torch.isfinite(yp).all())
            # the tail: an "aa_snake" and a "small" launch become one launch, counted under "small"
            assert (st, qt) == (sp - 1, qp), (st, qt, sp, qp)
            # the heads: three "aa_snake" launches per stage become one
            assert (sf, qf) == (st - 2 * stages, qt), (sf, qf, st, qt)
    finally:
        m.set_streams(3)
