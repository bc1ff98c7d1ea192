"""Every tile, operand split, halo class and epilogue of the convolution kernels, and every weight- / bias-gradient branch,
against a float64 evaluation of the same operation -- through the C ABI, with guarded buffers.

Checking discipline (shared by every test here):
  * outputs are views into one larger allocation with GUARD floats before and after them; the output is filled with NaN and the
    guard with a sentinel bit pattern before every launch; afterwards no NaN may be left (a store that never happened), the guard
    must be bit-unchanged (a store past either end) and the output finite;
  * inputs (x, dy) sit between NaN bands: a read past either end that reaches an accumulator poisons the result instead of
    being multiplied by a zero-padded weight and vanishing;
  * errors are bounded PER ELEMENT, |y - ref| <= tau * A with A = conv1d(|x|, |w|) + |b| in float64 -- the natural scale of each
    output's rounding error -- so a wrong value in a small output is not hidden by a large one elsewhere (conftest.rel_err is
    normalised by the global maximum).  tau per mode is in TAU below, each at most 2^-16; the measured max |y - ref| / A of every
    mode is report()ed at the end of the module;
  * results that must not depend on the tile (the automatic choice, the eight forced tiles, the producer / consumer kernel) are
    compared with torch.equal.

Arithmetic modes of a forward handle (dmel_conv_set_precision): 0 = FP32 -> NP = 3 (six-product bf16 split), 3 = FP32_F16X2 ->
NP = 2 (fp16 split), 1 = BF16 -> NP = 1 (bf16 operands; reference computed from the RNE-rounded operands)."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, report
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

TOL = 1e-4
DMEL_EUNSUPPORTED = -2
GUARD = 2048                     # floats on each side of a buffer: 8 KiB
SENTINEL = 0x5A5AA5A5            # guard bit pattern of outputs (a finite float, 1.5e16: no kernel writes it by accident)
NAN = float("nan")

# Per-element bound |y - ref| <= tau * A, per mode: 4x the largest max |y - ref| / A measured on the MI355X over this module's cases
# (fwd NP=3 2.8e-7, NP=2 2.9e-7, NP=1 1.2e-7 against its rounded operands, dx 4.8e-7, dw 2.8e-7, db 5.9e-8), rounded up.  Ceiling 2^-16 =
# 1.5e-5 for every one of them.  Dropping a first-order partial product of a split (a1 b2: up to 2^-8 |ab|) or staging an operand at bf16
# lands far above (test_forward_automatic_tile_meets_fp64_bound checks the latter on every shape).
TAU_CEIL = 2.0 ** -16
TAU = {
    "fwd NP=3": 1.2e-6,
    "fwd NP=2": 1.2e-6,
    "fwd NP=1": 5e-7,
    "dx NP=3": 2e-6,
    "dw": 1.2e-6,
    "db": 2.5e-7,
}
assert all(t <= TAU_CEIL for t in TAU.values())
MEASURED = {}                    # mode -> largest max |y - ref| / A seen by this module's tests


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def measured_error_report():
    yield
    for mode in TAU:
        if mode in MEASURED:
            report(f"conv matrix, {mode}: max |y - ref| / A = {MEASURED[mode]:.3e}  (tau {TAU[mode]:.2e}, ceiling 2^-16 = {TAU_CEIL:.2e})")


def lib():
    from dmel_codec_amd import _lib
    return _lib.lib()


def check(rc, what=""):
    from dmel_codec_amd import _lib
    _lib.check(rc, what)


def stream():
    from dmel_codec_amd import _lib
    return _lib.stream_ptr()


# ------------------------------------------------------------------------------------ guarded buffers
class Out:
    """A device output of `shape` as a view into one allocation with GUARD floats of SENTINEL before and after it."""

    def __init__(self, shape, dev):
        self.n = math.prod(shape)
        self.base = torch.empty(self.n + 2 * GUARD, dtype=torch.float32, device=dev)
        self.base.view(torch.int32).fill_(SENTINEL)
        self.t = self.base[GUARD:GUARD + self.n].view(shape)
        self.poison()

    def poison(self):
        self.t.fill_(NAN)
        return self

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        if self.base.is_cuda:
            torch.cuda.synchronize()
        bits = self.base.view(torch.int32)
        guard = torch.cat([bits[:GUARD], bits[GUARD + self.n:]])
        bad = int((guard != SENTINEL).sum())
        assert bad == 0, f"{what}: {bad} guard words around the output were written"
        holes = int(torch.isnan(self.t).sum())
        assert holes == 0, f"{what}: {holes} of {self.n} output elements were never written (still NaN)"
        assert bool(torch.isfinite(self.t).all()), f"{what}: non-finite output"
        return self.t


class In:
    """A device input holding `data`, between two bands of GUARD NaNs."""

    def __init__(self, data, dev):
        self.n = data.numel()
        self.base = torch.full((self.n + 2 * GUARD,), NAN, dtype=torch.float32, device=dev)
        self.t = self.base[GUARD:GUARD + self.n].view(data.shape)
        self.t.copy_(data)
        self.bits = self.base.view(torch.int32).clone()

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        if self.base.is_cuda:
            torch.cuda.synchronize()
        assert torch.equal(self.base.view(torch.int32), self.bits), f"{what}: an input or its NaN guard was written"


def ratio(y, ref, A):
    """max |y - ref| / A over all elements (float64; where A == 0 any error is infinite)."""
    err = (y.detach().double().cpu() - ref).abs()
    return float((err / A.clamp_min(1e-300)).max())


def assert_bound(y, ref, A, mode, what=""):
    r = ratio(y, ref, A)
    MEASURED[mode] = max(MEASURED.get(mode, 0.0), r)
    assert r <= TAU[mode], f"{what}: max |y - ref| / A = {r:.3e} > tau {TAU[mode]:.2e} ({mode})"
    return r


class Conv:
    """A dmel_conv handle (weights uploaded once), destroyed by close()."""

    def __init__(self, w, b, dil):
        self.Cout, self.Cin, self.k = w.shape
        self.h = C.c_void_p()
        self.w, self.b = w.contiguous(), b.contiguous() if b is not None else None
        check(lib().dmel_conv_create(C.byref(self.h), self.w.data_ptr(), self.b.data_ptr() if self.b is not None else None,
                                     self.Cout, self.Cin, self.k, dil), "dmel_conv_create")

    def close(self):
        lib().dmel_conv_destroy(self.h)


# ------------------------------------------------------------------------------------ forward tile matrix
# (Cout, Cin, k, dilation, T, B).  Halo = (k - 1) * dilation selects the kernel's staging class: 0, 16 (<= 16) or 64 (<= 64).
# Together: Cout 1 / 31 / 33 / 100 / 129 / 257 / 300 (ragged against 32 / 64 / 128 / 256-row tiles), Cin 8 / 17 / 24 / 130 (one 8-channel
# group, half a 16-channel K step, ragged chunks), T 1, 2, 31-33, 95-97, 127-129, 255-257, 3001 (below the halo, ragged against every
# BN in {32, 64, 96, 128, 256}, many column tiles), B 1 and 3, and a 1120 x 560 weight set (> 2.5 MB: the XCD-chunked 1-D grid, with
# padded workgroups on the tiles whose work list is not a multiple of 8).
FWD_SHAPES = [
    (1, 8, 1, 1, 257, 3),           # halo 0
    (31, 8, 1, 1, 128, 3),          # halo 0
    (257, 130, 1, 1, 95, 3),        # halo 0
    (31, 24, 3, 1, 2, 1),           # halo 2
    (129, 17, 3, 1, 96, 1),         # halo 2
    (300, 17, 3, 1, 256, 1),        # halo 2 (producer / consumer kernel eligible)
    (33, 130, 11, 1, 1, 1),         # halo 10, T below the halo
    (33, 17, 11, 1, 97, 3),         # halo 10
    (100, 130, 17, 1, 129, 1),      # halo 16 exactly
    (129, 24, 9, 2, 33, 3),         # halo 16 exactly
    (100, 8, 17, 1, 32, 3),         # halo 16 exactly
    (257, 17, 7, 9, 255, 1),        # halo 54
    (33, 24, 7, 9, 127, 1),         # halo 54
    (1, 24, 7, 9, 3001, 1),         # halo 54, long row
    (300, 8, 9, 8, 31, 3),          # halo 64 exactly, T below the halo
    (64, 130, 3, 32, 256, 1),       # halo 64 exactly
    (1120, 560, 3, 2, 64, 1),       # halo 4, XCD-chunked grid
]
NPS = {1: 1, 2: 3, 3: 0}            # NP -> DMEL_PRECISION_* that selects it on a dmel_conv handle
TILES = range(8)


def halo_class(k, dil):
    h = (k - 1) * dil
    return 0 if h == 0 else 16 if h <= 16 else 64


def shape_id(s):
    Cout, Cin, k, dil, T, B = s
    return f"h{halo_class(k, dil)}-{Cout}x{Cin}k{k}d{dil}-T{T}-B{B}"


@functools.lru_cache(maxsize=None)
def fwd_case(shape):
    """CPU fp32 operands and the float64 references of one forward shape."""
    Cout, Cin, k, dil, T, B = shape
    g = torch.Generator().manual_seed(Cout * 7919 + Cin * 104729 + k * 31 + dil * 17 + T * 3 + B)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(B, Cin, T, generator=g)
    pad = dil * (k - 1) // 2

    def refs(xx, ww):
        ref = F.conv1d(xx.double(), ww.double(), b.double(), dilation=dil, padding=pad)
        A = F.conv1d(xx.double().abs(), ww.double().abs(), None, dilation=dil, padding=pad) + b.double().abs()[None, :, None]
        return ref, A

    ref, A = refs(x, w)
    ref1, A1 = refs(x.bfloat16().float(), w.bfloat16().float())        # NP = 1: the RNE-rounded operands, exact products
    dy = torch.randn(B, Cout, T, generator=g)
    dx = torch.nn.grad.conv1d_input(x.shape, w.double(), dy.double(), dilation=dil, padding=pad)
    Adx = torch.nn.grad.conv1d_input(x.shape, w.double().abs(), dy.double().abs(), dilation=dil, padding=pad)
    return dict(w=w, b=b, x=x, dy=dy, ref={3: ref, 2: ref, 1: ref1}, A={3: A, 2: A, 1: A1}, dx=dx, Adx=Adx)


def forward(dev, case, shape, np_, what):
    """One dmel_conv_forward launch into a fresh guarded output; returns the checked output."""
    Cout, Cin, k, dil, T, B = shape
    conv = Conv(case["w"], case["b"], dil)
    try:
        check(lib().dmel_conv_set_precision(conv.h, NPS[np_]))
        x = In(case["x"], dev)
        y = Out((B, Cout, T), dev)
        check(lib().dmel_conv_forward(conv.h, x.ptr(), y.ptr(), B, T, stream()), what)
        out = y.check(what).clone()
        x.check(what)
        return out
    finally:
        conv.close()


_AUTO = {}


def auto_forward(dev, monkeypatch, shape, np_):
    """The automatically chosen tile's output (DMEL_CONV_PC=0: the conv_bf16_kernel tile, not the producer / consumer kernel)."""
    key = (shape, np_)
    if key not in _AUTO:
        monkeypatch.setenv("DMEL_CONV_PC", "0")
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
        _AUTO[key] = forward(dev, fwd_case(shape), shape, np_, f"{shape_id(shape)} NP={np_} automatic tile")
    return _AUTO[key]


@pytest.mark.parametrize("np_", [1, 2, 3], ids=lambda n: f"np{n}")
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=shape_id)
def test_forward_automatic_tile_meets_fp64_bound(dev, monkeypatch, shape, np_):
    """The automatic tile choice within tau * A of float64, guards intact; NP = 2: the producer / consumer kernel (DMEL_CONV_PC=2, which
    also takes the small launches; shapes it does not accept fall back to conv_bf16_kernel) bit-identical to it.  NP = 1: the
    bf16-operand result must VIOLATE the NP = 3 bound somewhere -- the bar tells an fp32-grade result from a degraded one."""
    case = fwd_case(shape)
    y = auto_forward(dev, monkeypatch, shape, np_)
    assert_bound(y, case["ref"][np_], case["A"][np_], f"fwd NP={np_}", f"{shape_id(shape)} NP={np_}")
    if np_ == 1:
        assert ratio(y, case["ref"][3], case["A"][3]) > TAU["fwd NP=3"], "bf16 operands pass the fp32-grade bound: the bound is blind"
    if np_ == 2:
        monkeypatch.setenv("DMEL_CONV_PC", "2")
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
        y_pc = forward(dev, case, shape, np_, f"{shape_id(shape)} producer / consumer")
        assert torch.equal(y_pc, y), float((y_pc - y).abs().max())


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"tile{t}")
@pytest.mark.parametrize("np_", [1, 2, 3], ids=lambda n: f"np{n}")
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=shape_id)
def test_forward_forced_tile_is_bit_identical(dev, monkeypatch, shape, np_, tile):
    """DMEL_CONV_TILE_BF16 forces a tile (read per call; DMEL_CONV_PC=0 keeps the producer / consumer kernel out).  Every tile accumulates
    K in the same order (pick_tile_bf16), which the streaming decoder's bit-identity rests on: torch.equal to the automatic choice."""
    y0 = auto_forward(dev, monkeypatch, shape, np_)
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))
    y = forward(dev, fwd_case(shape), shape, np_, f"{shape_id(shape)} NP={np_} tile {tile}")
    assert torch.equal(y, y0), (tile, float((y - y0).abs().max()))


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=shape_id)
def test_backward_data_every_tile_meets_fp64_bound(dev, monkeypatch, shape):
    """dmel_conv_backward_data (the forward kernel on the transposed, tap-reversed weight image; NP = 3 for gradients) against float64
    autograd dx, A = conv_transpose(|dy|, |w|); every forced tile torch.equal to the automatic one."""
    Cout, Cin, k, dil, T, B = shape
    case = fwd_case(shape)
    conv = Conv(case["w"], case["b"], dil)
    try:
        dy = In(case["dy"], dev)
        monkeypatch.setenv("DMEL_CONV_PC", "0")
        outs = []
        for tile in [None, *TILES]:
            if tile is None:
                monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
            else:
                monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))
            dx = Out((B, Cin, T), dev)
            what = f"{shape_id(shape)} dx tile {tile}"
            check(lib().dmel_conv_backward_data(conv.h, dy.ptr(), dx.ptr(), B, T, stream()), what)
            outs.append(dx.check(what).clone())
            dy.check(what)
        assert_bound(outs[0], case["dx"], case["Adx"], "dx NP=3", shape_id(shape))
        for tile, o in zip(TILES, outs[1:]):
            assert torch.equal(o, outs[0]), (tile, float((o - outs[0]).abs().max()))
    finally:
        conv.close()


@pytest.mark.parametrize("np_", [1, 2, 3], ids=lambda n: f"np{n}")
@pytest.mark.parametrize("k,dil", [(3, 33), (67, 1)], ids=["k3d33", "k67d1"])
def test_forward_refuses_a_halo_beyond_64(dev, monkeypatch, np_, k, dil):
    """(taps - 1) * dilation > 64 does not fit the LDS halo: DMEL_EUNSUPPORTED, and nothing is written.  (65 itself is not reachable with
    the odd tap counts dmel_conv_create accepts; 66 is the smallest halo past the limit.)"""
    g = torch.Generator().manual_seed(k * 100 + dil)
    w = torch.randn(40, 24, k, generator=g) / math.sqrt(24 * k)
    b = torch.randn(40, generator=g)
    conv = Conv(w, b, dil)
    try:
        check(lib().dmel_conv_set_precision(conv.h, NPS[np_]))
        x = In(torch.randn(2, 24, 150, generator=g), dev)
        for pc in ("0", "2"):
            monkeypatch.setenv("DMEL_CONV_PC", pc)
            y = Out((2, 40, 150), dev)
            rc = lib().dmel_conv_forward(conv.h, x.ptr(), y.ptr(), 2, 150, stream())
            torch.cuda.synchronize()
            assert rc == DMEL_EUNSUPPORTED, rc
            assert "exceeds" in lib().dmel_last_error().decode(), lib().dmel_last_error()
            assert bool(torch.isnan(y.t).all()), "a refused launch wrote its output"
            assert bool((y.base.view(torch.int32)[:GUARD] == SENTINEL).all() and (y.base.view(torch.int32)[-GUARD:] == SENTINEL).all())
            x.check("refused launch")
    finally:
        conv.close()


# ------------------------------------------------------------------------------------ paired epilogues and module features, per tile
def randomise(module, seed, scale=1.0):
    """O(1) weights so every term of the arithmetic matters (as test_gpu_parity.randomise)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf == "weight_g":
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (scale / p[0].numel() ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)


WN_LAYERS, WN_T, WN_LENS = 4, 97, [97, 50, 0, 96]


@functools.lru_cache(maxsize=None)
def wavenet_case():
    """A decoder-like WaveNet (conditioned: the two-segment GATE launch; RESSKIP with skip accumulation) at the fp16-split precision, with
    ragged lengths that include an empty item, and its float64 oracle output."""
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    torch.manual_seed(61)
    m = WaveNet(input_channels=64, output_channels=24, residual_channels=64, residual_layers=WN_LAYERS, dilation_cycle=4, condition_channels=64)
    randomise(m, 62)
    m.set_precision("fp32_f16x2")
    g = torch.Generator().manual_seed(63)
    N = len(WN_LENS)
    x, c = torch.randn(N, 64, WN_T, generator=g), torch.randn(N, 64, WN_T, generator=g)
    lens = torch.tensor(WN_LENS)
    mask = ref_cpu.sequence_mask(lens, WN_T)[:, None, :].double()
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ref = ref_cpu.wavenet_forward(sd, "", x.double() * mask, WN_LAYERS, condition=c.double()) * mask
    return m, x, c, lens, ref


_WN_DEFAULT = {}


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"tile{t}")
@pytest.mark.parametrize("presplit", ["0", "1"], ids=["presplit_off", "presplit_on"])
def test_wavenet_forced_tile_is_bit_identical(dev, monkeypatch, presplit, tile):
    """GATE (two-segment condition input, sigmoid * tanh), RESSKIP (residual / skip with skip accumulation), in_len / out_len masks and,
    with DMEL_WAVENET_PRESPLIT=1, the pre-split yp outputs -- on the layered path (DMEL_WAVENET_FUSED=0) with every tile forced: torch.equal
    to the default run, and within the parity bar of the float64 oracle."""
    m, x, c, lens, ref = wavenet_case()
    m = m.to(dev)
    xd, cd, ld = x.to(dev), c.to(dev), lens.to(dev)
    monkeypatch.setenv("DMEL_WAVENET_FUSED", "0")
    monkeypatch.setenv("DMEL_WAVENET_PRESPLIT", presplit)
    if presplit not in _WN_DEFAULT:
        monkeypatch.delenv("DMEL_CONV_PC", raising=False)
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
        y0 = m(xd, condition=cd, in_lengths=ld, out_lengths=ld)
        torch.cuda.synchronize()
        assert rel_err(y0, ref) < TOL, rel_err(y0, ref)
        _WN_DEFAULT[presplit] = y0.clone()
    y0 = _WN_DEFAULT[presplit]
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))
    y = m(xd, condition=cd, in_lengths=ld, out_lengths=ld)
    torch.cuda.synchronize()
    assert torch.equal(y, y0), (tile, float((y - y0).abs().max()))
    assert rel_err(y, ref) < TOL
    assert bool((y[2] == 0).all()) and bool((y[1, :, WN_LENS[1]:] == 0).all())


_VOC = {}


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"tile{t}")
@pytest.mark.parametrize("name", ["bigvgan_tiny", "bigvgan_tiny_ampblock2"])
def test_bigvgan_forced_tile_is_bit_identical(dev, golden, monkeypatch, name, tile):
    """The whole vocoder (AMPBlock1 / AMPBlock2: residual add, out_div and accumulate of the AMP branch sums; the transposed-conv phases)
    with every tile forced: torch.equal to the default run, and within TOL of the reference's golden audio."""
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
    g = golden(name)
    if name not in _VOC:
        m = BigVGAN(AttrDict(dict(g.meta["h"])))
        m.load_state_dict(g.sd)
        m = m.to(dev)
        monkeypatch.delenv("DMEL_CONV_PC", raising=False)
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
        y0 = m(g.ins["mel"].to(dev))
        torch.cuda.synchronize()
        assert rel_err(y0, g.outs["audio"]) < TOL
        _VOC[name] = (m, y0.clone())
    m, y0 = _VOC[name]
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))
    y = m(g.ins["mel"].to(dev))
    torch.cuda.synchronize()
    assert torch.equal(y, y0), (name, tile, float((y - y0).abs().max()))
    assert rel_err(y, g.outs["audio"]) < TOL


# ------------------------------------------------------------------------------------ weight- and bias-gradient branch matrix
# Branch table: test_weight_gradient_branch_meets_fp64_bound.__doc__.
WGRAD_BRANCHES = ("ipc", "flat", "k0", "f16", "grouped")
BGRAD_BRANCHES = ("flat1", "flat-atomic", "pieces1", "pieces-atomic")
# the lines of conv_bwd.hip the mirror below transcribes (tests/test_cpu_abi.py fails if one of them changes)
WGRAD_PREDICATE_SOURCE = (
    "a.ipc = a.T <= 32 ? kWgK / a.T : 1;",
    "const bool split = a.ipc == 1 && a.xstride <= 2 && a.T >= 256;",
    "((a.T + kWgK - 1) / kWgK) * kWgK * 10 > a.T * 11",
    "const bool grouped = split && a.dil == 1 && a.taps % 3 == 0;",
    "if (T < 256) {",
    "const int total = B * ((T + kBgPiece - 1) / kBgPiece);",
    "const int splits = std::max(1, std::min(total, 2048 / std::max(1, Cout)));",
    "constexpr int kWgK = 64;",
    "constexpr int kBgPiece = 2048;",
)


def wgrad_branch(k, dil, T):
    ipc = 64 // T if T <= 32 else 1
    split = ipc == 1 and T >= 256
    if split:
        return "grouped" if dil == 1 and k % 3 == 0 else "f16"
    if ipc > 1:
        return "ipc"
    return "flat" if ((T + 63) // 64) * 64 * 10 > T * 11 else "k0"


def bgrad_branch(Cout, B, T):
    total = B * ((T + 2047) // 2048)
    splits = max(1, min(total, 2048 // Cout))
    return ("flat" if T < 256 else "pieces") + ("-atomic" if splits > 1 else "1")


# (Cout, Cin, k, dilation, T, B); channel counts 1 / 17 / 64 / 65 / 130 against the 64 x 64 tile
WGRAD_CASES = [
    (17, 65, 3, 1, 1, 3),           # ipc 64, B not a multiple of it
    (64, 17, 5, 2, 7, 10),          # ipc 9, B = 10
    (130, 1, 3, 1, 32, 3),          # ipc 2
    (65, 64, 3, 1, 33, 2),          # flat
    (1, 130, 7, 3, 92, 3),          # flat
    (17, 17, 1, 1, 193, 2),         # flat
    (1100, 1, 1, 1, 92, 2),         # flat; db of > 1024 channels: one split, no atomics
    (64, 65, 3, 2, 64, 2),          # <0>
    (130, 17, 5, 1, 128, 1),        # <0>
    (17, 1, 3, 1, 250, 3),          # <0>
    (65, 130, 1, 1, 255, 2),        # <0>
    (64, 17, 7, 3, 256, 2),         # fp16 split
    (17, 65, 1, 1, 257, 3),         # fp16 split
    (130, 64, 7, 3, 1000, 1),       # fp16 split
    (1100, 1, 1, 1, 300, 2),        # fp16 split; db pieces, one split
    (17, 17, 3, 1, 256, 1),         # grouped, slices == 1
    (65, 64, 9, 1, 300, 2),         # grouped
    (17, 1, 3, 1, 4097, 2),         # grouped, many slices
    (64, 17, 9, 1, 4097, 2),        # grouped, many slices
]


def wgrad_id(s):
    Cout, Cin, k, dil, T, B = s
    return f"{wgrad_branch(k, dil, T)}-db_{bgrad_branch(Cout, B, T)}-{Cout}x{Cin}k{k}d{dil}-T{T}-B{B}"


@pytest.mark.parametrize("shape", WGRAD_CASES, ids=wgrad_id)
def test_weight_gradient_branch_meets_fp64_bound(dev, shape):
    """dmel_conv_backward_weight on every branch of launch_wgrad_any / launch_bgrad: dw and db NaN-prefilled and guarded, within tau * A of
    float64 autograd (A = wgrad(|x|, |dy|), sum |dy|); a second call into the same buffers overwrites them -- bit-equal on the grouped path
    (no atomics), within the bound on the atomic ones.  The test id names the weight- and bias-gradient branch of each case:

    Branches of launch_wgrad_any (csrc/conv_bwd.hip) as dmel_conv_backward_weight reaches them (fp32 handle, unit input stride, no A/B knob):

      branch    kernel                                   condition in conv_bwd.hip
      ipc       conv_wgrad_kernel<1>                     ipc = T <= 32 ? kWgK / T : 1 > 1, i.e. T <= 32 (several items per 64-sample step)
      flat      conv_wgrad_kernel<2>                     !split && ipc == 1 && T < 256 && ceil(T / 64) * 64 * 10 > T * 11 (flat_shape)
      k0        conv_wgrad_kernel<0>                     33 <= T < 256 and not flat_shape (<= 10 % padding in the last step)
      f16       conv_wgrad_split_kernel<1,1,1,64,2>      split = ipc == 1 && T >= 256, not grouped (fp16 split after absmax_kernel)
      grouped   conv_wgrad_f16g_kernel<1> + reduce       split && dil == 1 && taps % 3 == 0 (three-tap groups, wgrad_reduce_kernel)

    launch_bgrad / conv_bgrad_kernel: total = B * ceil(T / 2048) pieces, splits = max(1, min(total, 2048 / Cout)):
      flat1     T < 256, splits == 1 (direct store)      flat-atomic  T < 256, splits > 1 (zeroed, then atomicAdd)
      pieces1   T >= 256, splits == 1                    pieces-atomic T >= 256, splits > 1
    """
    Cout, Cin, k, dil, T, B = shape
    g = torch.Generator().manual_seed(Cout * 131 + Cin * 7 + k + T * 3 + B)
    w = torch.randn(Cout, Cin, k, generator=g) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(B, Cin, T, generator=g)
    dy = torch.randn(B, Cout, T, generator=g)
    pad = dil * (k - 1) // 2
    x64, dy64 = x.double(), dy.double()
    ref_dw = torch.nn.grad.conv1d_weight(x64, w.shape, dy64, dilation=dil, padding=pad)
    A_dw = torch.nn.grad.conv1d_weight(x64.abs(), w.shape, dy64.abs(), dilation=dil, padding=pad)
    ref_db, A_db = dy64.sum((0, 2)), dy64.abs().sum((0, 2))
    conv = Conv(w, b, dil)
    try:
        xd, dyd = In(x, dev), In(dy, dev)
        dw, db = Out((Cout, Cin, k), dev), Out((Cout,), dev)
        first = None
        for call in (1, 2):           # the second call lands on the first one's results: overwritten, not accumulated
            what = f"{wgrad_id(shape)} call {call}"
            check(lib().dmel_conv_backward_weight(conv.h, xd.ptr(), dyd.ptr(), dw.ptr(), db.ptr(), B, T, stream()), what)
            dw.check(what + " dw")
            db.check(what + " db")
            xd.check(what)
            dyd.check(what)
            assert_bound(dw.t, ref_dw, A_dw, "dw", what)
            assert_bound(db.t, ref_db, A_db, "db", what)
            if first is None:
                first = dw.t.clone()
            elif wgrad_branch(k, dil, T) == "grouped":
                assert torch.equal(dw.t, first), "the grouped weight gradient is not reproducible bit for bit"
    finally:
        conv.close()
