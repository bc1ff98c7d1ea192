"""The kernels a vocoder forward / backward launches besides the plain "same" convolution -- the transposed convolution (phased launches of
the convolution kernel), conv_post and its backward, the anti-aliased activation and its backward -- against float64 evaluations of the same
fp32 operands, through the C ABI, with the guarded buffers and the per-element bound |y - ref| <= tau * A of test_gpu_conv_matrix.py.

  1. Transposed convolution: the same kernels as the conv matrix, so its TAU, unchanged.  A = conv_transpose1d(|x|, |w|) + |b|.
  2. conv_post / 3. activation: tau_mode = min(FACTOR * R_mode, ceiling), with R_mode the largest max |y32 - ref64| / A of the fp32 CPU
     reference (torch / oracle.ref_cpu in float32) over this module's cases.  The R_mode are recorded below as constants;
     test_reference_ratios_do_not_exceed_the_recorded_ones (CPU) recomputes them.  No bound is taken from a kernel under test.
     FACTOR = 8: the kernel's sin^2 has a documented 2.5e-7 maximum absolute error, about four times a correctly rounded sinf squared, and the
     kernels sum in another order than the reference.  Ceilings: 2^-19 for the activation's y and dx (the 6 + 12 chained fmas plus 2.5e-7 come
     to about 1.5e-6 worst case; the smallest filter tap is 2.03e-3), 2^-16 for conv_post and the parameter gradients (the conv matrix's ceiling
     for reductions of this length).

The scale A of every mode is written next to its reference (post_case, aa_bounds).  Nothing is masked out of any comparison.
Results that must not depend on where a tile starts (decode_stream runs the vocoder on a window and crops) are compared with torch.equal.
"""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import report
from oracle import ref_cpu
from test_gpu_conv_matrix import GUARD, NPS, SENTINEL, TAU, TILES, In, Out, check, lib, ratio, stream

# ------------------------------------------------------------------------------------ tolerances of sections 2 and 3
# R_mode: largest max |y32 - ref64| / A of the fp32 CPU reference over this module's cases, rounded up by 5-10 % (recomputed and asserted by
# test_reference_ratios_do_not_exceed_the_recorded_ones; the measured values are in its docstring).  No kernel needed more than FACTOR = 8;
# the kernels' own maxima on the MI355X: post fwd 1.7e-7, post dx 1.9e-7, snake fwd 1.6e-7, snake dx 1.5e-7, snake da/db 2.6e-8
# (profiles/vocoder_ops_matrix.txt).  What the bounds exclude: a dropped outer filter tap (2.03e-3 of a sample against a bound of 1.4e-6 of
# the absolute-tap sum: ~100x above it wherever that sample is not tiny), a halo one sample short at a 1024 seam (the seam outputs lose or misplace one of
# their K or 12 products: 1e-3 .. 0.5 of A), a transposed-conv phase left unwritten (its columns stay NaN).
R = {
    "post fwd": 1.4e-7,
    "post dx": 2.0e-7,
    "snake fwd": 1.7e-7,
    "snake dx": 1.5e-7,
    "snake da/db": 2.8e-8,
}
FACTOR = {"post fwd": 8, "post dx": 8, "snake fwd": 8, "snake dx": 8, "snake da/db": 8}
CEIL = {"post fwd": 2.0 ** -16, "post dx": 2.0 ** -16, "snake fwd": 2.0 ** -19, "snake dx": 2.0 ** -19, "snake da/db": 2.0 ** -16}


def tau(mode):
    return TAU[mode[6:]] if mode.startswith("convT ") else min(FACTOR[mode] * R[mode], CEIL[mode])


MEASURED = {}                    # mode -> largest max |y - ref| / A seen by this module's GPU tests


def hold(y, ref, A, mode, what=""):
    r = ratio(y, ref, A)
    MEASURED[mode] = max(MEASURED.get(mode, 0.0), r)
    print(f"{what}: {mode} max |y - ref| / A = {r:.3e} (tau {tau(mode):.2e})")
    assert r <= tau(mode), f"{what}: max |y - ref| / A = {r:.3e} > tau {tau(mode):.2e} ({mode})"
    return r


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def measured_error_report():
    yield
    for mode in sorted(MEASURED):
        report(f"vocoder ops matrix, {mode}: max |y - ref| / A = {MEASURED[mode]:.3e}  (tau {tau(mode):.2e})")


def untouched(out):
    """A refused launch left its guarded output as it was: all NaN, guards intact."""
    torch.cuda.synchronize()
    bits = out.base.view(torch.int32)
    return bool(torch.isnan(out.t).all()) and bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + out.n:] == SENTINEL).all())


# ==================================================================================== 1. transposed convolution
CONVT_PAIRS = [(16, 8), (40, 24), (70, 33), (130, 31)]      # phases * Cout ragged against 32-row tiles, Cin split mid K step
CONVT_T = [1, 2, 31, 32, 33, 95, 96, 97, 127, 128, 129, 255, 256, 257, 1001]


def convt_cases():
    """(u, Cin, Cout, T, B): every T with every stride, the Ts dealt round over the four handles of a stride (shifted by one per stride);
    every handle gets T = 1 and a T above 256; B alternates 1 and 3; the real pair 512 -> 256 at u = 8."""
    cases = []
    for ui, u in enumerate((2, 4, 8)):
        per = [[1] for _ in CONVT_PAIRS]
        for i, T in enumerate(CONVT_T[1:]):
            per[(i + ui) % 4].append(T)
        for p, ts in enumerate(per):
            if max(ts) <= 256:
                ts.append(257 if (p + ui) % 2 else 1001)
            for T in ts:
                cases.append((u, *CONVT_PAIRS[p], T, 1 if len(cases) % 2 else 3))
    cases += [(8, 512, 256, 1, 3), (8, 512, 256, 97, 1), (8, 512, 256, 257, 1)]
    return cases


CONVT_CASES = convt_cases()


def convt_id(s):
    u, Cin, Cout, T, B = s
    return f"u{u}-{Cin}x{Cout}-T{T}-B{B}"


@functools.lru_cache(maxsize=None)
def convt_case(shape):
    """CPU fp32 operands and the float64 references of one transposed-convolution case."""
    u, Cin, Cout, T, B = shape
    g = torch.Generator().manual_seed(u * 7919 + Cin * 104729 + Cout * 31 + T * 3 + B)
    w = torch.randn(Cin, Cout, 2 * u, generator=g) / math.sqrt(Cin * 2)
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(B, Cin, T, generator=g)
    dy = torch.randn(B, Cout, T * u, generator=g)

    def refs(xx, ww):
        ref = F.conv_transpose1d(xx.double(), ww.double(), b.double(), stride=u, padding=u // 2)
        A = F.conv_transpose1d(xx.double().abs(), ww.double().abs(), None, stride=u, padding=u // 2) + b.double().abs()[None, :, None]
        return ref, A

    ref, A = refs(x, w)
    ref1, A1 = refs(x.bfloat16().float(), w.bfloat16().float())        # NP = 1: the RNE-rounded operands, exact products
    x64 = x.double().requires_grad_()
    (F.conv_transpose1d(x64, w.double(), b.double(), stride=u, padding=u // 2) * dy.double()).sum().backward()
    Adx = F.conv1d(dy.double().abs(), w.double().abs(), None, stride=u, padding=u // 2)    # the same operation on |dy|, |w|
    assert Adx.shape == x.shape
    return dict(w=w, b=b, x=x, dy=dy, ref={3: ref, 2: ref, 1: ref1}, A={3: A, 2: A, 1: A1}, dx=x64.grad, Adx=Adx)


class ConvT:
    """A dmel_conv_transpose handle, destroyed by close()."""

    def __init__(self, case, u):
        self.w, self.b = case["w"].contiguous(), case["b"].contiguous()
        Cin, Cout, k = self.w.shape
        self.h = C.c_void_p()
        check(lib().dmel_conv_transpose1d_create(C.byref(self.h), self.w.data_ptr(), self.b.data_ptr(), Cin, Cout, k, u), "conv_transpose1d_create")

    def close(self):
        lib().dmel_conv_transpose1d_destroy(self.h)


def force_tile(monkeypatch, tile):
    monkeypatch.setenv("DMEL_CONV_PC", "0")
    if tile is None:
        monkeypatch.delenv("DMEL_CONV_TILE_BF16", raising=False)
    else:
        monkeypatch.setenv("DMEL_CONV_TILE_BF16", str(tile))


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [3, 2, 1], ids=lambda n: f"np{n}")
@pytest.mark.parametrize("shape", CONVT_CASES, ids=convt_id)
def test_conv_transpose_forward_every_tile(dev, monkeypatch, shape, np_):
    """dmel_conv_transpose1d_forward (two phased launches that write interleaved columns: a column no phase wrote stays NaN) within the conv
    matrix's tau * A of float64; every forced tile torch.equal to the automatic one; NP = 1 must violate the NP = 3 bound somewhere."""
    u, Cin, Cout, T, B = shape
    case = convt_case(shape)
    ct = ConvT(case, u)
    try:
        check(lib().dmel_conv_transpose1d_set_precision(ct.h, NPS[np_]))
        x = In(case["x"], dev)
        outs = []
        for tile in [None, *TILES]:
            force_tile(monkeypatch, tile)
            what = f"{convt_id(shape)} NP={np_} tile {tile}"
            y = Out((B, Cout, T * u), dev)
            check(lib().dmel_conv_transpose1d_forward(ct.h, x.ptr(), y.ptr(), B, T, stream()), what)
            outs.append(y.check(what).clone())
            x.check(what)
        hold(outs[0], case["ref"][np_], case["A"][np_], f"convT fwd NP={np_}", convt_id(shape))
        if np_ == 1:
            assert ratio(outs[0], case["ref"][3], case["A"][3]) > TAU["fwd NP=3"], "bf16 operands pass the fp32-grade bound: the bound is blind"
        for tile, o in zip(TILES, outs[1:]):
            assert torch.equal(o, outs[0]), (tile, float((o - outs[0]).abs().max()))
    finally:
        ct.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONVT_CASES, ids=convt_id)
def test_conv_transpose_backward_data_every_tile(dev, monkeypatch, shape):
    """dmel_conv_transpose1d_backward_data (u / 2 launches of two strided segments, the later ones accumulating into dx) within tau * A of
    float64 autograd; the first call packs the images, the second finds them: torch.equal; every forced tile torch.equal to the automatic."""
    u, Cin, Cout, T, B = shape
    case = convt_case(shape)
    ct = ConvT(case, u)
    try:
        dy = In(case["dy"], dev)
        outs = []
        for tile in [None, None, *TILES]:
            force_tile(monkeypatch, tile)
            what = f"{convt_id(shape)} dx call {len(outs) + 1} tile {tile}"
            dx = Out((B, Cin, T), dev)
            check(lib().dmel_conv_transpose1d_backward_data(ct.h, dy.ptr(), dx.ptr(), B, T, stream()), what)
            outs.append(dx.check(what).clone())
            dy.check(what)
        hold(outs[0], case["dx"], case["Adx"], "convT dx NP=3", convt_id(shape))
        assert torch.equal(outs[1], outs[0]), "the call that packed the images and the next one differ"
        for tile, o in zip(TILES, outs[2:]):
            assert torch.equal(o, outs[0]), (tile, float((o - outs[0]).abs().max()))
    finally:
        ct.close()


# ==================================================================================== 2. conv_post
ACTS = {"none": 0, "tanh": 2, "clamp": 3}
# (C, K, B, T, act, seed).  T around the 256-sample thread stride and the 1024-sample tile (kPostTile), K = 7 with every T.  The seeds of the
# clamp cases are the first ones at which no float64 pre-activation lies within 1e-3 of +-1 and both clamped and unclamped samples exist
# (test_conv_post_clamp_cases_keep_their_margin); the others are arbitrary.
POST_CASES = [
    (32, 7, 1, 1, "tanh", 0), (5, 7, 3, 2, "none", 0), (24, 7, 1, 3, "tanh", 0), (1, 7, 3, 7, "clamp", 0),
    (32, 7, 3, 255, "clamp", 1), (5, 7, 1, 256, "tanh", 0), (24, 7, 3, 257, "none", 0), (1, 7, 1, 1021, "tanh", 0),
    (32, 7, 1, 1022, "none", 0), (5, 7, 3, 1023, "clamp", 19), (24, 7, 1, 1024, "tanh", 0), (32, 7, 3, 1025, "clamp", 13),
    (1, 7, 3, 1026, "none", 0), (5, 7, 1, 1027, "tanh", 0), (24, 7, 3, 2048, "clamp", 32), (32, 7, 1, 2051, "tanh", 0),
    (5, 3, 1, 1, "none", 0), (32, 3, 3, 2, "tanh", 0), (1, 3, 1, 257, "clamp", 0), (24, 3, 3, 1024, "none", 0),
    (5, 3, 1, 1025, "tanh", 0), (32, 3, 3, 2051, "clamp", 349),
    (24, 1, 3, 1, "tanh", 0), (1, 1, 1, 3, "none", 0), (32, 1, 1, 256, "clamp", 0), (5, 1, 3, 1023, "tanh", 0),
    (1, 1, 3, 1027, "clamp", 3), (24, 1, 1, 2048, "none", 0),
]
CLAMP_MARGIN = 1e-3


def post_id(s):
    Cc, K, B, T, act, _ = s
    return f"{act}-C{Cc}k{K}-T{T}-B{B}"


def post_act(act, pre):
    return {"none": lambda v: v, "tanh": torch.tanh, "clamp": lambda v: v.clamp(-1, 1)}[act](pre)


def post_operands(shape):
    """fp32 operands of one case: pre-activations of standard deviation about 1.5, so that tanh bends and the clamp cuts part of them."""
    Cc, K, B, T, act, seed = shape
    g = torch.Generator().manual_seed(seed * 1000003 + Cc * 7919 + K * 131 + B * 17 + T)
    w = torch.randn(Cc, K, generator=g) * (1.5 / math.sqrt(Cc * K))
    x = torch.randn(B, Cc, T, generator=g)
    bias = float(torch.tensor(0.3, dtype=torch.float32))
    dy = torch.randn(B, 1, T, generator=g)
    u = torch.rand(B, 1, T, generator=g) * 2 - 1
    ysaved = (u * 1.5).clamp(-1, 1) if act == "clamp" else u * 0.999      # an arbitrary saved output in (-1, 1); the clamp's reaches +-1 exactly
    return w, x, bias, dy, ysaved


def post_pre64(shape):
    Cc, K, B, T, act, seed = shape
    w, x, bias, _, _ = post_operands(shape)
    return F.conv1d(x.double(), w.double()[None], torch.tensor([bias], dtype=torch.float64), padding=K // 2)


def post_dact(act, y):
    """act' from the saved output, in y's dtype."""
    if act == "tanh":
        return 1 - y * y
    if act == "clamp":
        return (y.abs() < 1).to(y.dtype)
    return torch.ones_like(y)


@functools.lru_cache(maxsize=None)
def post_case(shape):
    """Operands, float64 references with their scales A, and the fp32 CPU reference's results.
    forward:  A = conv1d(|x|, |w|) + |bias| + |ref|  (the second term covers the rounding of tanhf)
    backward: A = conv_transpose1d(|dy| * (1 + y^2), |w|) for tanh (the rounding of 1 - y^2), conv_transpose1d(|dy * act'|, |w|) otherwise"""
    Cc, K, B, T, act, seed = shape
    w, x, bias, dy, ysaved = post_operands(shape)
    pad = K // 2
    ref = post_act(act, post_pre64(shape))
    A = F.conv1d(x.double().abs(), w.double().abs()[None], None, padding=pad) + abs(bias) + ref.abs()
    y32 = post_act(act, F.conv1d(x, w[None], torch.tensor([bias]), padding=pad))
    g64 = dy.double() * post_dact(act, ysaved.double())
    dx = F.conv_transpose1d(g64, w.double()[None], padding=pad)
    gabs = dy.double().abs() * (1 + ysaved.double() ** 2) if act == "tanh" else g64.abs()
    Adx = F.conv_transpose1d(gabs, w.double().abs()[None], padding=pad)
    dx32 = F.conv_transpose1d(dy * post_dact(act, ysaved), w[None], padding=pad)
    return dict(w=w, x=x, bias=bias, dy=dy, ysaved=ysaved, ref=ref, A=A, y32=y32, dx=dx, Adx=Adx, dx32=dx32)


def clamp_margin_ok(shape):
    pre = post_pre64(shape)
    return (float((pre.abs() - 1).abs().min()) > CLAMP_MARGIN, bool((pre.abs() > 1).any()), bool((pre.abs() < 1).any()))


def test_conv_post_clamp_cases_keep_their_margin():
    """The derivative and the value AT +-1 are a convention, not arithmetic: every clamp case keeps its float64 pre-activations more than 1e-3
    away from +-1, and has clamped and unclamped samples.  (CPU.)"""
    clamp = [s for s in POST_CASES if s[4] == "clamp"]
    assert len(clamp) >= 8
    for s in clamp:
        assert clamp_margin_ok(s) == (True, True, True), (post_id(s), clamp_margin_ok(s))
    for s in SHIFT_POST_CASES:
        if s[4] == "clamp":
            assert clamp_margin_ok(s) == (True, True, True), (post_id(s), clamp_margin_ok(s))


def post_forward(dev, shape, x, w, bias, what):
    Cc, K, B, T, act, _ = shape
    xd, wd = In(x, dev), In(w, dev)
    y = Out((x.shape[0], 1, x.shape[2]), dev)
    check(lib().dmel_conv_post_f32(xd.ptr(), wd.ptr(), bias, ACTS[act], y.ptr(), x.shape[0], Cc, K, x.shape[2], stream()), what)
    out = y.check(what).clone()
    xd.check(what)
    wd.check(what)
    return out


def post_backward(dev, shape, ysaved, dy, w, what):
    Cc, K, B, T, act, _ = shape
    yd = In(ysaved, dev) if act != "none" else None                   # none: y may be NULL
    dyd, wd = In(dy, dev), In(w, dev)
    dx = Out((dy.shape[0], Cc, dy.shape[2]), dev)
    check(lib().dmel_conv_post_backward_f32(yd.ptr() if yd else None, dyd.ptr(), wd.ptr(), ACTS[act], dx.ptr(), dy.shape[0], Cc, K, dy.shape[2],
                                            stream()), what)
    out = dx.check(what).clone()
    for buf in (yd, dyd, wd):
        if buf is not None:
            buf.check(what)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", POST_CASES, ids=post_id)
def test_conv_post_forward(dev, shape):
    case = post_case(shape)
    y = post_forward(dev, shape, case["x"], case["w"], case["bias"], post_id(shape))
    hold(y, case["ref"], case["A"], "post fwd", post_id(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", POST_CASES, ids=post_id)
def test_conv_post_backward(dev, shape):
    """dmel_conv_post_backward_f32 on an arbitrary saved output y in (-1, 1) (the clamp's reaching +-1 exactly, where act' = 0)."""
    case = post_case(shape)
    dx = post_backward(dev, shape, case["ysaved"], case["dy"], case["w"], post_id(shape))
    hold(dx, case["dx"], case["Adx"], "post dx", post_id(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("Cc,K,msg", [(4097, 3, "too large"), (8, 4, "bad shape")], ids=["lds_over_48k", "even_k"])
def test_conv_post_refuses(dev, Cc, K, msg):
    """C * K * 4 > 48 KiB (the weight table does not fit the LDS) and an even K: an error, forward and backward, nothing written."""
    B, T = 2, 40
    g = torch.Generator().manual_seed(Cc + K)
    x, w = In(torch.randn(B, Cc, T, generator=g), dev), In(torch.randn(Cc, K, generator=g), dev)
    yv, dy = In(torch.rand(B, 1, T, generator=g) - 0.5, dev), In(torch.randn(B, 1, T, generator=g), dev)
    for act in ACTS.values():
        y = Out((B, 1, T), dev)
        rc = lib().dmel_conv_post_f32(x.ptr(), w.ptr(), 0.1, act, y.ptr(), B, Cc, K, T, stream())
        assert rc < 0 and msg in lib().dmel_last_error().decode(), (rc, lib().dmel_last_error())
        assert untouched(y), "a refused conv_post wrote its output"
        dx = Out((B, Cc, T), dev)
        rc = lib().dmel_conv_post_backward_f32(yv.ptr(), dy.ptr(), w.ptr(), act, dx.ptr(), B, Cc, K, T, stream())
        assert rc < 0 and msg in lib().dmel_last_error().decode(), (rc, lib().dmel_last_error())
        assert untouched(dx), "a refused conv_post_backward wrote its output"
    for buf in (x, w, yv, dy):
        buf.check("refused conv_post")


SHIFT_L = 1100
SHIFT_POST_S = (1, 1021, 1024)
SHIFT_POST_CASES = [(24, 7, 2, 2200, "none", 0), (24, 7, 2, 2200, "tanh", 0), (24, 7, 2, 2200, "clamp", 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHIFT_POST_CASES, ids=post_id)
def test_conv_post_is_shift_invariant(dev, shape):
    """y(x)[..., s + 3 : s + L - 3] is torch.equal to the run on the window x[..., s : s + L], cropped by 3 on each side -- wherever the
    window starts against the 1024-sample tile; the same for dx(y, dy)."""
    Cc, K, B, T, act, _ = shape
    case = post_case(shape)
    y = post_forward(dev, shape, case["x"], case["w"], case["bias"], post_id(shape))
    hold(y, case["ref"], case["A"], "post fwd", post_id(shape))
    dx = post_backward(dev, shape, case["ysaved"], case["dy"], case["w"], post_id(shape))
    hold(dx, case["dx"], case["Adx"], "post dx", post_id(shape))
    for s in SHIFT_POST_S:
        win = lambda t: t[..., s:s + SHIFT_L].contiguous()
        yw = post_forward(dev, shape, win(case["x"]), case["w"], case["bias"], f"{post_id(shape)} window at {s}")
        assert torch.equal(yw[..., 3:-3], y[..., s + 3:s + SHIFT_L - 3]), (s, float((yw[..., 3:-3] - y[..., s + 3:s + SHIFT_L - 3]).abs().max()))
        dxw = post_backward(dev, shape, win(case["ysaved"]), win(case["dy"]), case["w"], f"{post_id(shape)} window at {s}")
        assert torch.equal(dxw[..., 3:-3], dx[..., s + 3:s + SHIFT_L - 3]), (s, float((dxw[..., 3:-3] - dx[..., s + 3:s + SHIFT_L - 3]).abs().max()))


# ==================================================================================== 3. anti-aliased activation
AA_B, AA_C = 2, 3
AA_KINDS = ("snakebeta_log", "snakebeta_lin", "snake_log")
AA_T_HALO = [1, 2, 3, 5, 6, 7, 11, 12, 13]            # at and below the 6-sample halo: both replicate pads fold onto the same samples
AA_T_TILE = list(range(1018, 1031))                   # the 1024 seam: a last tile shorter than the halo, the near-end samples over two tiles
AA_T_GROUP = list(range(2042, 2055))                  # the forward's workgroup seam (2 x 1024)
AA_T = AA_T_HALO + AA_T_TILE + AA_T_GROUP + [3073, 4097]
AA_T_LARGE = [5, 1030, 2049, 4097]                    # lengths of the large-argument forward cases
# linear-scale SnakeBeta with a large alpha on the middle channel, x = 2 randn: at 3000 about a sixth of that channel's arguments lie above
# the 8192 of snake_n's large-argument path (nearly every wave of the channel mixes both kinds, the other channels' waves are all small);
# at 1600 about one in 200 (two waves in three all small, the others mixed: a shifted window deals the lanes into other waves)
LARGE_ALPHA = {"large_lin": 3000.0, "sparse_lin": 1600.0}
LARGE_CASES = [(k, T) for k in LARGE_ALPHA for T in AA_T_LARGE]


@functools.lru_cache(maxsize=None)
def taps32():
    return ref_cpu.aa_filter12().view(-1).contiguous()


def aa_up(x, f):
    """UpSample1d of ref_cpu.activation1d with the taps f (1, 1, 12): replicate pad 5 / 5, x2 transposed convolution with gain 2, crop 15 / 15."""
    c = x.shape[1]
    h = 2 * F.conv_transpose1d(F.pad(x, (5, 5), mode="replicate"), f.expand(c, -1, -1), stride=2, groups=c)
    return h[..., 15:-15]


def aa_down(v, f):
    """DownSample1d of ref_cpu.activation1d: replicate pad 5 / 6, 12-tap low-pass at stride 2."""
    c = v.shape[1]
    return F.conv1d(F.pad(v, (5, 6), mode="replicate"), f.expand(c, -1, -1), stride=2, groups=c)


def aa_operands(kind, T, B=AA_B):
    g = torch.Generator().manual_seed((AA_KINDS + tuple(LARGE_ALPHA)).index(kind) * 100003 + T)
    x = torch.randn(B, AA_C, T, generator=g) * 2
    dy = torch.randn(B, AA_C, T, generator=g)
    logscale = kind.endswith("_log")
    snake = kind.startswith("snake_")
    alpha = torch.randn(AA_C, generator=g) * 0.5 if logscale else torch.rand(AA_C, generator=g) + 0.5
    beta = None if snake else (torch.randn(AA_C, generator=g) * 0.5 if logscale else torch.rand(AA_C, generator=g) + 0.5)
    if kind in LARGE_ALPHA:
        alpha[1] = LARGE_ALPHA[kind]
    return x, dy, alpha, beta, logscale, snake


def aa_reference(x, dy, alpha, beta, logscale, snake, dtype, grads=True):
    """y, dx, dalpha, dbeta of the oracle's six-op Activation1d in `dtype` (gradients by autograd, with respect to the STORED parameters)."""
    xx, a = x.to(dtype, copy=True).requires_grad_(grads), alpha.to(dtype, copy=True).requires_grad_(grads)
    b = beta.to(dtype, copy=True).requires_grad_(grads) if beta is not None else None
    y = ref_cpu.activation1d(xx, a, b if b is not None else a, taps32().view(1, 1, -1).to(dtype), None, logscale=logscale, snake=snake)
    if not grads:
        return y.detach(), None, None, None
    (y * dy.to(dtype)).sum().backward()
    return y.detach(), xx.grad, a.grad, b.grad if b is not None else None


def aa_bounds(x, dy, alpha, beta, logscale, snake, grads=True):
    """The scales A (float64) of y, dx and the parameter gradients.  With |f| the absolute taps, a / inv_b the effective parameters:
      U    = up_abs(|x|)                                               bounds |u|
      A_y  = down_abs(U * (1 + a * inv_b) + inv_b)                     v = u + inv_b sin^2(a u); a * inv_b * U carries the rounding of the argument
      DV   = down_abs^T(|dy|)                                          bounds |dv|
      A_dx = up_abs^T(DV * (1 + a * inv_b * (1 + 2 a U)))              du = dv (1 + a inv_b sin(2 a u))
      A_da = J_a * sum inv_b * DV * U * (1 + 2 a U)                    per channel; J = exp(stored parameter) in log scale, else 1
      A_db = J_b * sum inv_b^2 * DV * (1 + 2 a U)
    Snake (beta := alpha) receives both sums on its one parameter.  The transposes are vector-Jacobian products of the abs-tap maps."""
    f = taps32().view(1, 1, -1).double().abs()
    a = alpha.double()
    b = a if beta is None else beta.double()
    J_a, J_b = (a.exp(), b.exp()) if logscale else (torch.ones_like(a), torch.ones_like(b))
    if logscale:
        a, b = a.exp(), b.exp()
    a, inv_b = a.abs().view(1, -1, 1), (1.0 / (b + 1e-9)).abs().view(1, -1, 1)
    U = aa_up(x.double().abs(), f)
    A_y = aa_down(U * (1 + a * inv_b) + inv_b, f)
    if not grads:
        return A_y, None, None, None
    v0 = torch.zeros_like(U).requires_grad_()
    DV, = torch.autograd.grad(aa_down(v0, f), v0, dy.double().abs())
    x0 = torch.zeros_like(U[..., ::2]).requires_grad_()
    A_dx, = torch.autograd.grad(aa_up(x0, f), x0, DV * (1 + a * inv_b * (1 + 2 * a * U)))
    A_da = J_a * (inv_b * DV * U * (1 + 2 * a * U)).sum((0, 2))
    A_db = J_b * (inv_b * inv_b * DV * (1 + 2 * a * U)).sum((0, 2))
    if snake:
        return A_y, A_dx, A_da + A_db, None
    return A_y, A_dx, A_da, A_db


@functools.lru_cache(maxsize=None)
def aa_case(kind, T):
    x, dy, alpha, beta, logscale, snake = aa_operands(kind, T)
    grads = kind in AA_KINDS                           # the large-argument cases are forward only
    ref = aa_reference(x, dy, alpha, beta, logscale, snake, torch.float64, grads)
    ref32 = aa_reference(x, dy, alpha, beta, logscale, snake, torch.float32, grads)
    return dict(x=x, dy=dy, alpha=alpha, beta=beta, logscale=logscale, snake=snake, ref=ref, ref32=ref32,
                A=aa_bounds(x, dy, alpha, beta, logscale, snake, grads))


def aa_forward(dev, x, alpha, beta, logscale, what):
    B, Cc, T = x.shape
    xd, ad, bd = In(x, dev), In(alpha, dev), In(beta, dev) if beta is not None else None
    y = Out((B, Cc, T), dev)
    check(lib().dmel_aa_snake_f32(xd.ptr(), y.ptr(), ad.ptr(), bd.ptr() if bd else None, taps32().data_ptr(), taps32().data_ptr(), int(logscale),
                                  B, Cc, T, stream()), what)
    out = y.check(what).clone()
    for buf in (xd, ad, bd):
        if buf is not None:
            buf.check(what)
    return out


def aa_backward(dev, case, what, params=True, add=None):
    """dmel_aa_snake_backward_f32 (params) or dmel_aa_snake_backward_input_f32 into guarded outputs: (dx, dalpha, dbeta)."""
    B, Cc, T = case["x"].shape
    beta = case["beta"]
    xd, dyd, ad = In(case["x"], dev), In(case["dy"], dev), In(case["alpha"], dev)
    bd = In(beta, dev) if beta is not None else None
    rd = In(add, dev) if add is not None else None
    dx = Out((B, Cc, T), dev)
    da = Out((Cc,), dev) if params else None
    db = Out((Cc,), dev) if params and beta is not None else None
    t, ls = taps32(), int(case["logscale"])
    if params:
        check(lib().dmel_aa_snake_backward_f32(xd.ptr(), dyd.ptr(), dx.ptr(), ad.ptr(), bd.ptr() if bd else None, da.ptr(), db.ptr() if db else None,
                                               t.data_ptr(), t.data_ptr(), ls, B, Cc, T, stream()), what)
    else:
        check(lib().dmel_aa_snake_backward_input_f32(xd.ptr(), dyd.ptr(), rd.ptr() if rd else None, dx.ptr(), ad.ptr(), bd.ptr() if bd else None,
                                                     t.data_ptr(), t.data_ptr(), ls, B, Cc, T, stream()), what)
    outs = [o.check(what).clone() if o is not None else None for o in (dx, da, db)]
    for buf in (xd, dyd, ad, bd, rd):
        if buf is not None:
            buf.check(what)
    return outs


def aa_id(kind, T):
    return f"{kind}-T{T}"


AA_CASES = [(k, T) for k in AA_KINDS for T in AA_T]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T", AA_CASES + LARGE_CASES, ids=lambda v: str(v))
def test_activation_forward(dev, kind, T):
    """aa_snake_kernel into a NaN-filled guarded output (an unwritten tail shows), every element within tau * A_y of float64.  large_lin /
    sparse_lin: one channel with a large alpha next to ordinary ones, arguments up to about 2e4 -- the large-argument path of snake_n."""
    case = aa_case(kind, T)
    if kind in LARGE_ALPHA and T >= 2049:
        arg = (aa_up(case["x"].double(), taps32().view(1, 1, -1).double()) * case["alpha"].double().view(1, -1, 1)).abs()
        frac = float((arg[:, 1] > 8192).float().mean())
        assert (0.05 < frac < 0.5 if kind == "large_lin" else 0 < frac < 0.01) and float(arg[:, 0].max()) < 100, frac
    y = aa_forward(dev, case["x"], case["alpha"], case["beta"], case["logscale"], aa_id(kind, T))
    hold(y, case["ref"][0], case["A"][0], "snake fwd", aa_id(kind, T))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T", AA_CASES, ids=lambda v: str(v))
def test_activation_backward(dev, kind, T):
    """aa_snake_bwd_kernel<true>: dx per element, dalpha / dbeta per channel, all guarded; then aa_snake_bwd_kernel<false>
    (dmel_aa_snake_backward_input_f32) at the seam and halo lengths: dx torch.equal to the full backward's, and dx + r in fp32 with `add`."""
    case = aa_case(kind, T)
    _, dx64, da64, db64 = case["ref"]
    _, A_dx, A_da, A_db = case["A"]
    dx, da, db = aa_backward(dev, case, aa_id(kind, T))
    hold(dx, dx64, A_dx, "snake dx", aa_id(kind, T))
    hold(da, da64, A_da, "snake da/db", aa_id(kind, T) + " dalpha")
    if db64 is not None:
        hold(db, db64, A_db, "snake da/db", aa_id(kind, T) + " dbeta")
    if T in AA_T_HALO or T in AA_T_TILE:
        dxi, _, _ = aa_backward(dev, case, aa_id(kind, T) + " input only", params=False)
        assert torch.equal(dxi, dx), float((dxi - dx).abs().max())
        r = torch.randn(case["x"].shape, generator=torch.Generator().manual_seed(T))
        dxr, _, _ = aa_backward(dev, case, aa_id(kind, T) + " input only + add", params=False, add=r)
        assert torch.equal(dxr.cpu(), dx.cpu() + r), float((dxr.cpu() - (dx.cpu() + r)).abs().max())


SHIFT_AA_S = (1, 5, 1019, 1024, 2047)
SHIFT_AA_T = 3200


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["snakebeta_log", *LARGE_ALPHA])
def test_activation_forward_is_shift_invariant(dev, kind):
    """What VQGAN.decode_stream rests on: y(x)[..., s + 6 : s + L - 6] is torch.equal to the run on the window x[..., s : s + L] cropped by 6,
    wherever the window starts against the 1024-sample tiles and the 64-lane waves -- also when a wave holds large and small arguments."""
    case = aa_case(kind, SHIFT_AA_T)
    y = aa_forward(dev, case["x"], case["alpha"], case["beta"], case["logscale"], f"{kind} full row")
    hold(y, case["ref"][0], case["A"][0], "snake fwd", f"{kind} T{SHIFT_AA_T}")
    bad = []
    for s in SHIFT_AA_S:
        yw = aa_forward(dev, case["x"][..., s:s + SHIFT_L].contiguous(), case["alpha"], case["beta"], case["logscale"], f"{kind} window at {s}")
        a, b = yw[..., 6:-6], y[..., s + 6:s + SHIFT_L - 6]
        if not torch.equal(a, b):
            per_channel = [int((a[:, c] != b[:, c]).sum()) for c in range(AA_C)]
            bad.append(f"s={s}: {int((a != b).sum())} of {a.numel()} elements differ (per channel {per_channel}), max |diff| {float((a - b).abs().max()):.3e}")
    assert not bad, f"{kind}: the output depends on where the window starts: " + "; ".join(bad)


# ==================================================================================== the recorded reference ratios
def reference_ratios():
    """mode -> largest max |y32 - ref64| / A of the fp32 CPU reference over this module's cases."""
    out = {m: 0.0 for m in R}

    def take(mode, y32, ref, A):
        out[mode] = max(out[mode], ratio(y32, ref, A))

    for s in POST_CASES + SHIFT_POST_CASES:
        c = post_case(s)
        take("post fwd", c["y32"], c["ref"], c["A"])
        take("post dx", c["dx32"], c["dx"], c["Adx"])
    for kind, T in AA_CASES + LARGE_CASES + [(k, SHIFT_AA_T) for k in ("snakebeta_log", *LARGE_ALPHA)]:
        c = aa_case(kind, T)
        take("snake fwd", c["ref32"][0], c["ref"][0], c["A"][0])
        if c["ref"][1] is not None:
            take("snake dx", c["ref32"][1], c["ref"][1], c["A"][1])
            take("snake da/db", c["ref32"][2], c["ref"][2], c["A"][2])
            if c["ref"][3] is not None:
                take("snake da/db", c["ref32"][3], c["ref"][3], c["A"][3])
    return out


def test_reference_ratios_do_not_exceed_the_recorded_ones():
    """The fp32 CPU reference (torch / oracle.ref_cpu in float32) against float64, in units of A, over every case of sections 2 and 3: none
    above the recorded R_mode the kernel bounds are multiples of (nor below half of it: a stale constant), and every bound at or below its
    ceiling.  Measured: post fwd 1.291e-7, post dx 1.878e-7, snake fwd 1.558e-7, snake dx 1.420e-7, snake da/db 2.610e-8.  (CPU.)"""
    got = reference_ratios()
    for mode, r in got.items():
        print(f"R[{mode!r}] measured {r:.3e}, recorded {R[mode]:.2e}, tau {tau(mode):.2e}")
        assert 0.5 * R[mode] <= r <= R[mode], (mode, r, R[mode])
        assert tau(mode) <= CEIL[mode]
