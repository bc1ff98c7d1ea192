"""Three activations of one tensor in one launch (dmel_aa_snake3_forward / _items, aa_snake.hip): the heads of the three AMP blocks behind an
up-sampler of BigVGAN.  Every output must be torch.equal to a launch of dmel_aa_snake_f32 (dmel_aa_snake_items_f32) with its parameters.

  * T on both sides of the 1008-output tile and of the three-tile workgroup, of every residue mod 4 (both row alignments);
  * one, three and 32 channels, one and three items, log-scale and linear parameters, SnakeBeta and Snake (beta NULL) in one launch;
  * one parameter set with alpha = 5000 on a channel: arguments of sin^2 on both sides of 8192 inside one wave;
  * the launcher admits mixed alignment -- an output takes 16-byte stores when it, x and the rows are 16-byte aligned, dword stores
    otherwise: one output 4 bytes off while the others are aligned, x off (every access dword), every output off by another amount;
  * items: ragged lengths with NaN behind them in x and a canary behind them in every output."""
import math

import pytest
import torch

from test_gpu_conv_matrix import check, lib, stream
from test_gpu_vocoder_ops_matrix import taps32

pytestmark = pytest.mark.gpu

TILE = 1008
T_LIST = [1, 2, 7, 64, 301, 1007, 1008, 1009, 2016, 2017, 3023, 3024, 3025, 4033]
CANARY = -777.0
OFFSETS = [(0, (0, 0, 0)), (0, (0, 1, 0)), (1, (0, 0, 0)), (0, (1, 2, 3))]      # floats behind a 16-byte boundary: x, (y0, y1, y2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_the_sizes_cover_the_seams():
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1, 4 * TILE + 1} <= set(T_LIST)
    assert {t % 4 for t in T_LIST} == {0, 1, 2, 3}


def params(C, logscale, dev, seed):
    """three (alpha, beta): SnakeBeta, Snake (beta None), SnakeBeta with one large alpha"""
    g = torch.Generator().manual_seed(seed)
    draw = (lambda: torch.randn(C, generator=g) * 0.5) if logscale else (lambda: torch.rand(C, generator=g) + 0.5)
    sets = [(draw(), draw()), (draw(), None), (draw(), draw())]
    sets[2][0][C // 2] = math.log(5000.0) if logscale else 5000.0
    return [(a.to(dev), b.to(dev) if b is not None else None) for a, b in sets]


def view(dev, shape, off, fill):
    """a tensor of `shape` that starts `off` floats behind a 16-byte boundary inside a canary-filled allocation"""
    n = math.prod(shape)
    base = torch.full((n + 16,), fill, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    return base, base[4 + off:4 + off + n].view(shape)


def p(t):
    return t.data_ptr() if t is not None else None


def one(dev, x, a, b, logscale, lens=None):
    y = torch.full_like(x, CANARY)
    B, C, T = x.shape
    if lens is None:
        check(lib().dmel_aa_snake_f32(p(x), p(y), p(a), p(b), p(taps32()), p(taps32()), logscale, B, C, T, stream()), "aa_snake")
    else:
        check(lib().dmel_aa_snake_items_f32(p(x), p(y), p(a), p(b), p(taps32()), p(taps32()), logscale, B, C, T, p(lens), stream()), "aa_snake_items")
    return y


def three(dev, x, sets, logscale, xoff, yoffs, lens=None):
    """the one-launch form into guarded outputs; x NaN-guarded"""
    B, C, T = x.shape
    xb, xv = view(dev, x.shape, xoff, float("nan"))
    xv.copy_(x)
    outs = [view(dev, x.shape, o, CANARY) for o in yoffs]
    args = [p(xv)] + [p(v) for _, v in outs] + [q for a, b in sets for q in (p(a), p(b))] + [p(taps32()), p(taps32()), logscale, B, C, T]
    if lens is None:
        check(lib().dmel_aa_snake3_forward(*args, stream()), "aa_snake3")
    else:
        check(lib().dmel_aa_snake3_forward_items(*args, p(lens), stream()), "aa_snake3_items")
    torch.cuda.synchronize()
    for base, v in outs:
        n = v.numel()
        off = (v.data_ptr() - base.data_ptr()) // 4
        assert bool((base[:off] == CANARY).all() and (base[off + n:] == CANARY).all()), "an output was written outside the tensor"
    return [v for _, v in outs]


@pytest.mark.parametrize("T", T_LIST)
def test_each_output_has_the_bits_of_its_own_launch(dev, T):
    bad = []
    for C in (1, 3, 32):
        for B in (1, 3):
            for logscale in (0, 1):
                g = torch.Generator().manual_seed(T * 131 + C * 7 + B)
                x = (torch.randn(B, C, T, generator=g) * 2).to(dev)
                sets = params(C, logscale, dev, T + C)
                want = [one(dev, x, a, b, logscale) for a, b in sets]
                if T >= 64:      # both sin^2 branches: the large-alpha channel has arguments on either side of 8192
                    arg = (x[:, C // 2] * 5000.0).abs()
                    assert bool((arg > 8192).any() and (arg < 8192).any())
                for xoff, yoffs in OFFSETS:
                    got = three(dev, x, sets, logscale, xoff, yoffs)
                    for k in range(3):
                        if not torch.equal(got[k], want[k]):
                            bad.append(f"C {C} B {B} logscale {logscale} offsets {xoff} {yoffs} output {k}: "
                                       f"{int((got[k] != want[k]).sum())} of {want[k].numel()} differ")
    assert not bad, f"T {T}: " + "; ".join(bad[:8])


LENS = [0, 1, 2, 5, 1007, 1008, 1009, 3023, 3024, 3025, 3028]


@pytest.mark.parametrize("pitch,xoff,yoffs", [(3028, 0, (0, 0, 0)), (3029, 0, (0, 0, 0)), (3028, 0, (0, 1, 0)), (3028, 1, (0, 0, 0))],
                         ids=["aligned", "odd_pitch", "y1_off", "x_off"])
def test_items_equal_the_items_launch_of_each_output(dev, pitch, xoff, yoffs):
    assert {1, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1, 3028} <= set(LENS) and {n % 4 for n in LENS} == {0, 1, 2, 3}
    B, C = len(LENS), 3
    lens = torch.tensor(LENS, dtype=torch.int64, device=dev)
    for logscale in (0, 1):
        g = torch.Generator().manual_seed(pitch + logscale)
        x = torch.randn(B, C, pitch, generator=g) * 2
        for b, n in enumerate(LENS):
            x[b, :, n:] = float("nan")                     # nothing may read the columns at or beyond an item's length
        x = x.to(dev)
        sets = params(C, logscale, dev, pitch)
        want = [one(dev, x, a, b, logscale, lens) for a, b in sets]
        got = three(dev, x, sets, logscale, xoff, yoffs, lens)
        for k in range(3):
            for b, n in enumerate(LENS):
                assert bool(torch.isfinite(got[k][b, :, :n]).all()), (logscale, k, b, n)
                assert torch.equal(got[k][b, :, :n], want[k][b, :, :n]), (logscale, k, b, n)
                assert bool((got[k][b, :, n:] == CANARY).all()), (logscale, k, b, n, "written at or beyond the item's length")


def test_bad_arguments_are_refused(dev):
    x = torch.zeros(1, 2, 8, device=dev)
    y = [torch.zeros_like(x) for _ in range(3)]
    a = torch.zeros(2, device=dev)
    t = taps32()
    L = lib()
    ok = [p(x), p(y[0]), p(y[1]), p(y[2]), p(a), None, p(a), None, p(a), None, p(t), p(t), 0, 1, 2, 8]
    check(L.dmel_aa_snake3_forward(*ok, stream()), "aa_snake3")
    for i, v in ((0, None), (2, None), (6, None), (2, p(y[0])), (3, p(x)), (15, 0)):      # NULL x / output / alpha, aliased outputs, T = 0
        args = list(ok)
        args[i] = v
        assert L.dmel_aa_snake3_forward(*args, stream()) != 0, i
    assert L.dmel_aa_snake3_forward_items(*ok, None, stream()) != 0
    torch.cuda.synchronize()
