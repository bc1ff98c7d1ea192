"""The one-launch transposed convolution (strides 2, 4, 8: one weight image with every phase, rows phase-minor, taps d = -1, 0, +1 with the
unused tap zero, 8- / 16-byte stores) against the two phase-major launches it replaces, which DMEL_UPSTAGE_ONE_LAUNCH=0 keeps in the same
process: torch.equal, through the C ABI, into the NaN-prefilled outputs between sentinel guards of test_gpu_conv_matrix (a sample no store
reached stays NaN, a store past either end breaks a guard) and from inputs between NaN bands (a read past x that reaches an accumulator
poisons it: the third tap reads one column further than the two launches did).

The two-launch path itself is held to float64 at every tile by test_gpu_vocoder_ops_matrix.py; nothing here is a tolerance.

Shapes: 40 rows (a 32-row strip that is part padding), 24 rows (less than one strip), the real stage-4 pair; T = 1, 31, 32, 33 (edge tiles
on every tile width) and 97 (one full 96-column tile per wave plus an edge column: the vector-store body and the scalar one in one launch)."""
import ctypes as C
import math

import pytest
import torch

from test_gpu_conv_matrix import GUARD, NAN, SENTINEL, In, Out, TILES, check, lib, stream

pytestmark = pytest.mark.gpu

CASES = [(8, 16, 8), (8, 24, 5), (4, 16, 12), (2, 24, 12), (2, 64, 32)]          # (u, Cin, Cout)
LENGTHS = [1, 31, 32, 33, 97]
BATCHES = [1, 3]
PRECISIONS = {"np3": 0, "np2": 3, "np1": 1, "fp32mfma": 2}                       # DMEL_PRECISION_*: the three splits and the native fp32 kernel


def case_id(c):
    return f"u{c[0]}-{c[1]}x{c[2]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def operands(case, T, B):
    u, Cin, Cout = case
    g = torch.Generator().manual_seed(u * 7919 + Cin * 104729 + Cout * 31 + T * 3 + B)
    w = (torch.randn(Cin, Cout, 2 * u, generator=g) / math.sqrt(Cin * 2)).contiguous()
    b = (torch.randn(Cout, generator=g) * 0.1).contiguous()
    return w, b, torch.randn(B, Cin, T, generator=g)


class ConvT:
    def __init__(self, case, w, b, precision):
        u, Cin, Cout = case
        self.h = C.c_void_p()
        check(lib().dmel_conv_transpose1d_create(C.byref(self.h), w.data_ptr(), b.data_ptr(), Cin, Cout, 2 * u, u), "conv_transpose1d_create")
        check(lib().dmel_conv_transpose1d_set_precision(self.h, precision))

    def close(self):
        lib().dmel_conv_transpose1d_destroy(self.h)


class OutAt(Out):
    """Out whose first element lies `off` floats behind a 16-byte boundary."""

    def __init__(self, shape, dev, off):
        self.n = math.prod(shape)
        self.whole = torch.empty(self.n + 2 * GUARD + 4, dtype=torch.float32, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.base = self.whole[off:off + self.n + 2 * GUARD]
        self.base.view(torch.int32).fill_(SENTINEL)
        self.t = self.base[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        self.poison()


def forward(ct, x, shape, dev, what, one, monkeypatch, lens=None, off=0):
    """One forward into a fresh guarded output; one = False: the two phase-major launches."""
    if one:
        monkeypatch.delenv("DMEL_UPSTAGE_ONE_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("DMEL_UPSTAGE_ONE_LAUNCH", "0")
    B, Cout, Tu = shape
    y = OutAt(shape, dev, off)
    T = x.t.shape[2]
    if lens is None:
        check(lib().dmel_conv_transpose1d_forward(ct.h, x.ptr(), y.ptr(), B, T, stream()), what)
    else:
        check(lib().dmel_conv_transpose1d_forward_items(ct.h, x.ptr(), y.ptr(), B, T, lens.data_ptr(), stream()), what)
    out = y.check(what).clone()
    x.check(what)
    return out


@pytest.mark.parametrize("prec", list(PRECISIONS), ids=list(PRECISIONS))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_launch_equals_two_launches(dev, monkeypatch, case, prec):
    """every length and batch: the one launch torch.equal to the two, at each precision"""
    u, Cin, Cout = case
    for T in LENGTHS:
        for B in BATCHES:
            w, b, x = operands(case, T, B)
            ct = ConvT(case, w, b, PRECISIONS[prec])
            try:
                xin = In(x, dev)
                what = f"{case_id(case)} T{T} B{B} {prec}"
                two = forward(ct, xin, (B, Cout, T * u), dev, what + " two launches", False, monkeypatch)
                one = forward(ct, xin, (B, Cout, T * u), dev, what + " one launch", True, monkeypatch)
                assert torch.equal(one, two), (what, float((one - two).abs().max()))
            finally:
                ct.close()


@pytest.mark.parametrize("prec", list(PRECISIONS), ids=list(PRECISIONS))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_item_lengths_in_one_batch(dev, monkeypatch, case, prec):
    """in_len = {0, 1, T - 1, T} in one batch (dmel_conv_transpose1d_forward_items): equal to the two launches; the empty item is its bias,
    the full one what the call without lengths gives, the one a column short is not"""
    u, Cin, Cout = case
    T, B = 97, 4
    w, b, x = operands(case, T, B)
    ct = ConvT(case, w, b, PRECISIONS[prec])
    try:
        xin = In(x, dev)
        host = [0, 1, T - 1, T]
        lens = torch.tensor(host, dtype=torch.int64, device=dev)
        what = f"{case_id(case)} items {prec}"
        two = forward(ct, xin, (B, Cout, T * u), dev, what + " two launches", False, monkeypatch, lens)
        one = forward(ct, xin, (B, Cout, T * u), dev, what + " one launch", True, monkeypatch, lens)
        assert torch.equal(one, two), (what, float((one - two).abs().max()))
        assert torch.equal(one[0], b.to(dev)[:, None].expand(Cout, T * u)), "an empty item is its bias"
        whole = forward(ct, xin, (B, Cout, T * u), dev, what + " no lengths", True, monkeypatch)
        assert torch.equal(one[3], whole[3]) and not torch.equal(one[2], whole[2]), "a full-length item reads all of x, a shorter one does not"
    finally:
        ct.close()


@pytest.mark.parametrize("off", [1, 2], ids=["off1", "off2"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_unaligned_output_takes_scalar_stores(dev, monkeypatch, case, off):
    """an output that starts one float (4-byte aligned only) or two floats (8-byte aligned: still vector stores at u = 2) into its buffer"""
    u, Cin, Cout = case
    for T, B in ((33, 1), (97, 3)):
        w, b, x = operands(case, T, B)
        ct = ConvT(case, w, b, PRECISIONS["np2"])
        try:
            xin = In(x, dev)
            what = f"{case_id(case)} T{T} B{B} output {off} floats behind a 16-byte boundary"
            ref = forward(ct, xin, (B, Cout, T * u), dev, what + " two launches, aligned", False, monkeypatch)
            got = forward(ct, xin, (B, Cout, T * u), dev, what, True, monkeypatch, off=off)
            assert torch.equal(got, ref), what
        finally:
            ct.close()


@pytest.mark.parametrize("prec", ["np3", "np2", "np1"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_forced_tile_equals_the_automatic_one(dev, monkeypatch, case, prec):
    u, Cin, Cout = case
    T, B = 97, 3
    w, b, x = operands(case, T, B)
    ct = ConvT(case, w, b, PRECISIONS[prec])
    try:
        xin = In(x, dev)
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
        auto = forward(ct, xin, (B, Cout, T * u), dev, f"{case_id(case)} {prec} automatic tile", True, monkeypatch)
        for tile in TILES:
            monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))
            got = forward(ct, xin, (B, Cout, T * u), dev, f"{case_id(case)} {prec} tile {tile}", True, monkeypatch)
            assert torch.equal(got, auto), (case, prec, tile)
    finally:
        ct.close()
