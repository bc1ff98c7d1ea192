"""The two one-launch WaveNet kernels -- wavenet_fused_kernel (csrc/wavenet_fused.hip: the whole encoder stack in one launch) and
wavenet_stream_kernel (csrc/wavenet_stream.hip: a streaming push in one launch, plain and per-item) -- at every edge of their
eligibility, through the C ABI, with the guarded buffers of test_gpu_conv_matrix.py.  Their contract is the BITS of the layered path.

  1. Whole sequence (CASES): a covering table over the residual width (every chunk count, widths of every residue mod 4 next to a
     chunk boundary, the last eligible width), the raw input width (none, one channel, 8 | 9 around the staging group, 16 = the
     eligibility edge), depth 1 and 2 (the weight prefetch runs past the last block before the first has finished), every dilation
     cycle and every T next to a 32-column seam of the fifteen-wave layout, the halo or the largest dilation.  Every case runs without
     lengths, with equal lengths and with in_lengths != out_lengths, the lengths drawn from {0, 1, T/2, T-1, T, T+5}; each run with
     DMEL_WAVENET_FUSED unset (exactly one launch) and set to 0 (more than 2 L launches): torch.equal, y exactly 0 at and behind
     min(out_len, T), x behind in_lengths never read (1e30 there changes no bit), and within two bounds of a float64 evaluation of
     oracle.ref_cpu.wavenet_forward on the same fp32 operands: conftest.rel_err < TOL (normalised by the global maximum) and, per
     (item, channel) row, max_t |y - y64| / max_t |y64| <= min(8 R, TOL).  R is the largest such per-row ratio of the oracle ITSELF
     evaluated in float32 over these cases -- a constant below that tests/test_wavenet_one_launch_cpu.py recomputes; the factor 8 is
     that of test_gpu_vocoder_ops_matrix.py (six partial products per block summed in another order than the reference's, expf and
     tanhf with their own error).  No bound is taken from a kernel under test.
     So that no row is left out of the per-row bound, no row's max |y64| may lie below 1e-3 of its run's global maximum (checked by the
     CPU test): a row of one valid column (T = 1, a length of 1) is a single number, and a random stack puts some of those near zero.
     The skip_projection bias -- the last term added to every output -- is therefore drawn from +-[2, 3], several times the size of
     the signal under it (build_stack): every row maximum is at least a third of its run's global one (0.372 measured), and an error
     of the size of the signal -- a wrong column or channel -- still stands orders of magnitude above the bound.
  2. Dispatch edges (EDGES): stacks and lengths just outside the predicate must take the layered path (more than one launch) and meet
     rel_err < TOL; a batch that is no multiple of group_repeat is refused when lengths are given; 33 blocks run layered through
     dmel_wavenet_stream_step_ex and are refused by dmel_wavenet_stream_step_items.
  3. Streaming (STREAM_STACKS): pushes of 1, 96, 97 (one sub-step exactly at the limit and one of a single column), 7, a re-base,
     8 and the final step(s), on two buffer sets: after every step all L + 1 history levels, skip and y of the one-launch step equal those
     of the layered step and what was valid before the step has the bits of a copy taken before it, and at the end y equals
     dmel_wavenet_forward of the whole input.  What a call writes is NaN before it; what the header says a call may not rely on --
     every level at and behind its frontier, x behind next[0] -- holds 1e30 in the one-launch set.  Then the same pushes as three
     utterances of one per-item launch (rotated against each other, one idle every second step, one re-based) against
     dmel_wavenet_stream_step_items_layered step by step and each utterance's own single run."""
import ctypes as C
import functools
import time

import pytest
import torch

from conftest import rel_err, report
from oracle import ref_cpu
from test_gpu_conv_matrix import GUARD, SENTINEL, TOL, In, Out, check, lib, stream
from test_gpu_parity import randomise

pytestmark = pytest.mark.gpu

NAN = float("nan")
HUGE = 1e30                      # what stands where a call may not read
DMEL_EUNSUPPORTED = -2
N_ITEMS, GROUP = 4, 2            # whole-sequence cases: four items, two per utterance (lengths index n // GROUP)

# R: the largest per-row ratio max_t |y32 - y64| / max_t |y64| of oracle.ref_cpu.wavenet_forward in float32 against float64 over
# CASES x MODES, rounded up by 5-10 % (recomputed by tests/test_wavenet_one_launch_cpu.py; the measured value is in its docstring).
R = 1.25e-6
FACTOR = 8
ROW_TOL = min(FACTOR * R, TOL)
ROW_FLOOR = 1e-3                 # no row's max |y64| below this fraction of its run's global maximum

# ------------------------------------------------------------------------------------ the eligibility predicate, mirrored
# eligible(), MAX_T, MAX_STREAM_L and SUBSTEP transcribe lines of csrc/modules.hip, ops.h, wavenet_fused.hip and wavenet_stream.hip:
# ONE_LAUNCH_PREDICATE_SOURCE in tests/test_cpu_abi.py holds them and fails when one changes
MAX_T, MAX_STREAM_L, SUBSTEP = 96, 32, 96


def eligible(C_res, Cin, Ccond, has_out, cycle):
    """WaveNetFused::ok (dmel_wavenet_finalize).  Cin None: no input projection."""
    return 32 < C_res <= 80 and not Ccond and not has_out and (Cin is None or Cin <= 16) and (cycle == 0 or cycle <= 4)


def chunks(C_res):
    return (C_res + 15) // 16


def t_class(T):
    return 0 if T <= 32 else 1 if T <= 64 else 2


# ------------------------------------------------------------------------------------ 1. the whole-sequence table
# (residual channels, raw input channels or None, blocks, dilation_cycle, T); the covering properties are asserted by
# tests/test_wavenet_one_launch_cpu.py
CASES = [
    (33, 8, 1, 0, 1), (33, 16, 5, 1, 2), (33, None, 4, 1, 33), (33, 10, 5, 2, 65), (33, None, 4, 2, 7),
    (47, 10, 20, 2, 8), (47, 1, 1, 1, 9), (47, 1, 20, 0, 63), (47, None, 20, 2, 95), (47, None, 3, 2, 15),
    (48, 10, 4, 4, 16), (48, 9, 4, 0, 17), (48, 16, 1, 2, 64), (48, None, 20, 2, 96), (48, 8, 20, 4, 31),
    (49, 16, 4, 3, 32), (49, 16, 5, 0, 1), (49, 1, 20, 1, 33), (49, 8, 1, 3, 65), (49, 9, 5, 4, 2),
    (63, 1, 5, 3, 7), (63, 8, 4, 4, 8), (63, 10, 3, 2, 63), (63, 8, 5, 3, 95), (63, 10, 1, 4, 9),
    (64, 9, 2, 0, 15), (64, None, 3, 1, 16), (64, 8, 3, 4, 64), (64, 1, 20, 4, 96), (64, None, 3, 0, 17),
    (65, 10, 20, 0, 31), (65, 16, 2, 1, 32), (65, 9, 20, 3, 33), (65, 1, 4, 3, 65), (65, 1, 5, 3, 1),
    (70, 8, 3, 3, 2), (70, 16, 4, 4, 7), (70, 8, 2, 2, 63), (70, 9, 20, 1, 95), (70, 10, 3, 3, 8),
    (79, 1, 3, 0, 9), (79, 1, 5, 4, 15), (79, 9, 4, 3, 64), (79, 9, 2, 3, 96), (79, None, 20, 3, 16),
    (80, 10, 5, 4, 17), (80, 9, 3, 4, 31), (80, 16, 3, 3, 33), (80, None, 3, 2, 65), (80, 16, 2, 4, 32),
]
MODES = ("none", "equal", "differ")
LEN_KINDS = ("0", "1", "T/2", "T-1", "T", "T+5")


def length_of(kind, T):
    return {"0": 0, "1": 1, "T/2": T // 2, "T-1": T - 1, "T": T, "T+5": T + 5}[kind]


def case_length_kinds(i, mode):
    """-> (kinds of in_lengths, kinds of out_lengths), one per utterance, or (None, None): rotated through LEN_KINDS by the case index"""
    k = lambda j: LEN_KINDS[(i + j) % len(LEN_KINDS)]
    if mode == "none":
        return None, None
    if mode == "equal":
        return (k(0), k(3)), (k(0), k(3))
    return (k(0), k(2)), (k(1), k(4))


def case_lengths(i, mode):
    T = CASES[i][4]
    ik, ok = case_length_kinds(i, mode)
    if ik is None:
        return None, None
    return [length_of(a, T) for a in ik], [length_of(a, T) for a in ok]


def case_id(i):
    C_res, Cin, L, cycle, T = CASES[i]
    return f"C{C_res}-in{Cin}-L{L}-cyc{cycle}-T{T}"


@functools.lru_cache(maxsize=None)
def build_stack(C_res, Cin, L, cycle, Ccond=None, Cout=None):
    """-> (the WaveNet mirror on the CPU, its float64 state dict).  test_gpu_parity.randomise weights; the skip_projection bias
    from +-[2, 3] (see the module docstring)."""
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    seed = C_res * 1009 + (Cin or 0) * 101 + L * 13 + cycle + 7 * (Ccond or 0) + 3 * (Cout or 0)
    torch.manual_seed(seed)
    m = WaveNet(input_channels=Cin, output_channels=Cout, residual_channels=C_res, residual_layers=L, dilation_cycle=cycle,
                condition_channels=Ccond)
    randomise(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        b = m.skip_projection.conv.bias
        b.copy_((2.0 + torch.rand(b.shape, generator=g)) * (torch.randint(0, 2, b.shape, generator=g) * 2 - 1))
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    return m, sd


def masks(lens, T, dtype):
    """(N, 1, T) mask of per-utterance lengths clamped to [0, T], or 1.0"""
    if lens is None:
        return 1.0
    clamped = torch.tensor(lens).clamp(0, T)
    return ref_cpu.sequence_mask(clamped, T).repeat_interleave(GROUP, dim=0)[:, None, :].to(dtype)


@functools.lru_cache(maxsize=None)
def case_input(i):
    C_res, Cin, L, cycle, T = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randn(N_ITEMS, Cin or C_res, T, generator=g)


@functools.lru_cache(maxsize=None)
def case_reference(i, mode, dtype=torch.float64):
    """oracle.ref_cpu.wavenet_forward of case i in `dtype` on the fp32 operands: the input times the in-mask, the output times the
    out-mask (computed once per run and shared)."""
    C_res, Cin, L, cycle, T = CASES[i]
    _, sd = build_stack(C_res, Cin, L, cycle)
    if dtype != torch.float64:
        sd = {k: v.to(dtype) for k, v in sd.items()}
    il, ol = case_lengths(i, mode)
    x = case_input(i).to(dtype)
    return ref_cpu.wavenet_forward(sd, "", x * masks(il, T, dtype), L, cycle) * masks(ol, T, dtype)


def row_ratio(y, y64, out_lens):
    """-> (largest max_t |y - y64| / max_t |y64| over the (item, channel) rows with a non-empty valid range,
           smallest row max |y64| / global max |y64| over the same rows); (0, 1) when every row is empty"""
    y, T = y.detach().double().cpu(), y64.shape[2]
    valid = torch.ones(y64.shape[0], dtype=torch.bool) if out_lens is None else \
        (torch.tensor(out_lens).clamp(0, T) > 0).repeat_interleave(GROUP)
    if not bool(valid.any()):
        return 0.0, 1.0
    err = (y - y64).abs().amax(dim=2)[valid]
    top = y64.abs().amax(dim=2)[valid]
    return float((err / top.clamp_min(1e-300)).max()), float(top.min() / y64.abs().max())


# ------------------------------------------------------------------------------------ guarded buffers beyond Out / In
class Lens:
    """int64 lengths on the device between two bands of -7: a read past either end masks a whole item"""
    BAND = 64

    def __init__(self, values, dev):
        n = len(values)
        self.base = torch.full((n + 2 * self.BAND,), -7, dtype=torch.int64, device=dev)
        self.t = self.base[self.BAND:self.BAND + n]
        self.t.copy_(torch.tensor(values, dtype=torch.int64))
        self.bits = self.base.clone()

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        assert torch.equal(self.base, self.bits), f"{what}: the lengths or their guard were written"


def ptr(b):
    return None if b is None else b.ptr()


def guards_intact(out, what):
    """the SENTINEL bands of an Out whose payload is not wholly written by the call (state buffers, scratch)"""
    torch.cuda.synchronize()
    bits = out.base.view(torch.int32)
    bad = int((bits[:GUARD] != SENTINEL).sum()) + int((bits[GUARD + out.n:] != SENTINEL).sum())
    assert bad == 0, f"{what}: {bad} guard words were written"


class Prof:
    """conv_igemm launches of the calls made inside the block"""

    def __enter__(self):
        from dmel_codec_amd import _lib
        _lib.prof_reset()
        _lib.prof_enable(True)
        return self

    def __exit__(self, *exc):
        from dmel_codec_amd import _lib
        torch.cuda.synchronize()
        self.launches = _lib.prof_read("conv_igemm")["launches"]
        _lib.prof_enable(False)
        _lib.prof_reset()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


MEASURED = {"row": 0.0, "rel": 0.0, "one": set(), "layered_min_over_2L": 1e9, "runs": 0}


@pytest.fixture(scope="module", autouse=True)
def measured_report():
    t0 = time.time()
    yield
    if MEASURED["runs"]:
        report(f"wavenet one-launch matrix: {MEASURED['runs']} whole-sequence runs; largest per-row max_t |y - y64| / max_t |y64| = "
               f"{MEASURED['row']:.3e}  (R {R:.2e}, tolerance min({FACTOR} R, {TOL:g}) = {ROW_TOL:.2e}); largest rel_err = {MEASURED['rel']:.3e} "
               f"(bar {TOL:g}); launches with DMEL_WAVENET_FUSED unset {sorted(MEASURED['one'])}, set to 0 at least "
               f"{MEASURED['layered_min_over_2L']:.2f} x 2 L")
    report(f"wavenet one-launch matrix: module wall time {time.time() - t0:.1f} s")


def native(m, dev):
    with torch.cuda.device(dev):
        return m.native()


def forward(dev, m, x, T, il, ol, group, what, cond=None, N=N_ITEMS):
    """One dmel_wavenet_forward into a fresh NaN-filled guarded y (the header: the call writes all of it) -> (rc, y, launches); every
    guard and the bits of every input are checked."""
    h = native(m, dev)
    nbytes = lib().dmel_wavenet_workspace_bytes(h, N, T)
    ws = Out(((nbytes + 3) // 4,), dev)
    y = Out((N, m.output_channels, T), dev)
    with Prof() as prof:
        rc = lib().dmel_wavenet_forward(h, x.ptr(), ptr(cond), y.ptr(), N, T, ptr(il), ptr(ol), group, ws.ptr(), nbytes, stream())
    guards_intact(ws, what + " workspace")
    for b in (x, cond, il, ol):
        if b is not None:
            b.check(what)
    return rc, y, prof.launches


@pytest.mark.parametrize("i", range(len(CASES)), ids=case_id)
def test_whole_sequence_kernel_equals_the_layered_path_and_meets_both_fp64_bounds(dev, monkeypatch, i):
    C_res, Cin, L, cycle, T = CASES[i]
    assert eligible(C_res, Cin, None, False, cycle) and T <= MAX_T
    m, _ = build_stack(C_res, Cin, L, cycle)
    x_cpu = case_input(i)
    for mode in MODES:
        what = f"{case_id(i)} lengths {mode}"
        il_v, ol_v = case_lengths(i, mode)
        il = Lens(il_v, dev) if il_v is not None else None
        ol = Lens(ol_v, dev) if ol_v is not None else None
        inputs = [In(x_cpu, dev)]
        if il_v is not None:
            # behind in_lengths the header reads x as x * 0: a second input with 1e30 there must give the same bits
            poisoned = x_cpu.clone()
            for n in range(N_ITEMS):
                poisoned[n, :, max(0, il_v[n // GROUP]):] = HUGE
            inputs.append(In(poisoned, dev))
        outs = []
        for x in inputs:
            monkeypatch.delenv("DMEL_WAVENET_FUSED", raising=False)
            rc, y1, n1 = forward(dev, m, x, T, il, ol, GROUP, what + " one launch")
            check(rc, what)
            monkeypatch.setenv("DMEL_WAVENET_FUSED", "0")
            rc, y0, n0 = forward(dev, m, x, T, il, ol, GROUP, what + " layered")
            check(rc, what)
            monkeypatch.delenv("DMEL_WAVENET_FUSED")
            assert n1 == 1 and n0 > 2 * L, f"{what}: {n1} launch(es) with the kernel, {n0} layered (2 L = {2 * L})"
            MEASURED["one"].add(n1)
            MEASURED["layered_min_over_2L"] = min(MEASURED["layered_min_over_2L"], n0 / (2 * L))
            a, b = y1.check(what + " one launch"), y0.check(what + " layered")
            assert torch.equal(a, b), f"{what}: {int((a != b).sum())} elements differ from the layered path, max {float((a - b).abs().max()):.3e}"
            outs.append(a)
        if len(outs) == 2:
            assert torch.equal(outs[0], outs[1]), f"{what}: x behind in_lengths was read ({int((outs[0] != outs[1]).sum())} elements moved)"
        y = outs[0]
        if ol_v is not None:
            for n in range(N_ITEMS):
                lim = min(max(ol_v[n // GROUP], 0), T)
                assert bool((y[n, :, lim:] == 0).all()), f"{what}: item {n} is not exactly 0 at and behind {lim}"
        y64 = case_reference(i, mode)
        e = rel_err(y, y64)
        r, floor = row_ratio(y, y64, ol_v)
        print(f"{what}: launches {n1} / {n0}, rel_err {e:.3e}, per-row {r:.3e} (tolerance {ROW_TOL:.2e}), smallest row / global maximum {floor:.3f}")
        MEASURED["rel"], MEASURED["row"] = max(MEASURED["rel"], e), max(MEASURED["row"], r)
        MEASURED["runs"] += 1
        assert floor >= ROW_FLOOR
        assert e < TOL, f"{what}: rel_err {e:.3e}"
        assert r <= ROW_TOL, f"{what}: per-row max_t |y - y64| / max_t |y64| = {r:.3e} > {ROW_TOL:.2e}"


# ------------------------------------------------------------------------------------ 2. the dispatch edges
# name -> (stack kwargs, T): each one step outside the predicate (eligible() / T <= MAX_T say so), so the layered path must run
EDGES = {
    "C32": (dict(C_res=32, Cin=10, L=3, cycle=4), 40),
    "C81": (dict(C_res=81, Cin=10, L=3, cycle=4), 40),
    "T97": (dict(C_res=70, Cin=10, L=3, cycle=4), 97),
    "Cin17": (dict(C_res=70, Cin=17, L=3, cycle=4), 40),
    "cycle5": (dict(C_res=70, Cin=10, L=5, cycle=5), 40),
    "condition8": (dict(C_res=70, Cin=10, L=3, cycle=4, Ccond=8), 40),
    "output20": (dict(C_res=70, Cin=10, L=3, cycle=4, Cout=20), 40),
}


def edge_is_outside(name):
    kw, T = EDGES[name]
    return not (eligible(kw["C_res"], kw["Cin"], kw.get("Ccond"), kw.get("Cout") is not None, kw["cycle"]) and T <= MAX_T)


@pytest.mark.parametrize("name", list(EDGES))
def test_a_stack_outside_the_predicate_takes_the_layered_path(dev, monkeypatch, name):
    kw, T = EDGES[name]
    assert edge_is_outside(name)
    monkeypatch.delenv("DMEL_WAVENET_FUSED", raising=False)
    m, sd = build_stack(**kw)
    g = torch.Generator().manual_seed(len(name) + T)
    x = torch.randn(N_ITEMS, kw["Cin"], T, generator=g)
    c = torch.randn(N_ITEMS, kw["Ccond"], T, generator=g) if kw.get("Ccond") else None
    lens = [T, T // 2]
    il, ol = Lens(lens, dev), Lens(lens, dev)
    rc, y, launches = forward(dev, m, In(x, dev), T, il, ol, GROUP, name, cond=In(c, dev) if c is not None else None)
    check(rc, name)
    assert launches > 1, f"{name}: {launches} launch: the one-launch kernel took a stack outside its predicate"
    mask = masks(lens, T, torch.float64)
    ref = ref_cpu.wavenet_forward(sd, "", x.double() * mask, kw["L"], kw["cycle"], condition=c.double() if c is not None else None) * mask
    e = rel_err(y.check(name), ref)
    assert e < TOL, (name, e)


def test_a_batch_that_is_no_multiple_of_group_repeat_is_refused_when_lengths_are_given(dev, monkeypatch):
    """The kernels index the lengths by n / group_repeat: N = 3 with group_repeat = 2 would read behind a table of N / 2 entries."""
    monkeypatch.delenv("DMEL_WAVENET_FUSED", raising=False)
    m, _ = build_stack(70, 10, 3, 4)
    T = 40
    x = In(torch.randn(3, 10, T, generator=torch.Generator().manual_seed(3)), dev)
    for il, ol in ((Lens([T], dev), None), (None, Lens([T], dev)), (Lens([T], dev), Lens([T], dev))):
        rc, y, launches = forward(dev, m, x, T, il, ol, GROUP, "N = 3, group_repeat = 2", N=3)
        assert rc < 0 and launches == 0, (rc, launches)
        assert "group_repeat" in lib().dmel_last_error().decode()
        assert bool(torch.isnan(y.t).all()), "a refused call wrote y"
        guards_intact(y, "refused call")
    rc, y, launches = forward(dev, m, x, T, None, None, GROUP, "N = 3 without lengths", N=3)      # nothing is indexed: served
    check(rc)
    assert launches == 1
    y.check("N = 3 without lengths")


# ------------------------------------------------------------------------------------ 3. streaming
STREAM_T, STREAM_CAP, STREAM_LENS = 230, 256, [230, 181]
PUSHES = (1, 96, 97, 7, 8)       # new level-0 columns per step; the re-base comes after the fourth
# (residual channels, raw input channels or None, blocks, dilation_cycle)
STREAM_STACKS = [
    (33, None, 1, 0), (47, 1, 2, 1), (49, 9, 3, 2), (65, 16, 5, 3), (79, None, 20, 4), (80, 16, 32, 4), (80, 1, 2, 1), (49, 9, 20, 4),
]


def stack_id(s):
    return f"C{s[0]}-in{s[1]}-L{s[2]}-cyc{s[3]}"


class Row:
    """The frontiers of one utterance in absolute frames, and the absolute frame of its column 0."""

    def __init__(self, L, cycle):
        self.L, self.prev, self.origin = L, [0] * (L + 1), 0
        self.dils = [2 ** (i % cycle) if cycle else 1 for i in range(L)]

    def frontiers(self, upto, final):
        nxt = [upto]
        for l, d in enumerate(self.dils):
            nxt.append(upto if final else max(self.prev[l + 1], nxt[-1] - d))
        return nxt

    def rel(self, absolute):
        return [p - self.origin for p in absolute]


class Bufs:
    """The state of R utterances x `group` items for the streaming entries, every buffer an Out (guards on both sides).  `fill` is what
    stands wherever the header says a call may not rely on the contents: at and behind every level's frontier."""

    def __init__(self, m, R, group, cap, fill, dev):
        self.m, self.R, self.G, self.N, self.cap, self.fill, self.dev = m, R, group, R * group, cap, fill, dev
        self.L, self.C = len(m.residual_layers), m.residual_channels
        self.has_in = m.input_projection is not None
        N, C_res, L = self.N, self.C, self.L
        self.x = Out((N, m.input_channels, cap), dev) if self.has_in else None
        self.hist, self.skip, self.y = Out((L + 1, N, C_res, cap), dev), Out((N, C_res, cap), dev), Out((N, C_res, cap), dev)
        self.scratch = Out((2 * N * C_res * cap + 2 * N + R * (2 * (L + 1) + 1),), dev)
        for b in self.state():
            b.t.fill_(fill)

    def state(self):
        return [b for b in (self.x, self.hist, self.skip, self.y) if b is not None]

    def items(self, r):
        return slice(r * self.G, (r + 1) * self.G)

    def prepare(self, r, row, nxt, x_abs):
        """before a step of utterance r to the absolute frontiers nxt: the new input in, NaN where the call writes, `fill` where it may
        not read"""
        sl, o = self.items(r), row.origin
        p, n = row.rel(row.prev), row.rel(nxt)
        src = x_abs[sl, :, o:o + n[0]]
        if self.has_in:
            self.x.t[sl, :, :n[0]] = src
            self.x.t[sl, :, n[0]:] = self.fill
        else:
            self.hist.t[0, sl, :, :n[0]] = src
        for l in range(self.L + 1):
            self.hist.t[l, sl, :, n[l]:] = self.fill
            if l > 0 or self.has_in:
                self.hist.t[l, sl, :, p[l]:n[l]] = NAN
        self.skip.t[sl, :, p[1]:n[1]] = NAN
        self.skip.t[sl, :, n[1]:] = self.fill
        self.y.t[sl, :, p[self.L]:n[self.L]] = NAN
        self.y.t[sl, :, n[self.L]:] = self.fill

    def rebase(self, r, row):
        """drop every column of utterance r the next steps cannot read: the last level's window reaches back max-dilation columns"""
        new_origin = max(0, row.prev[self.L] - 8)
        shift = new_origin - row.origin
        if shift > 0:
            sl = self.items(r)
            for b in self.state():
                v = b.t[..., sl, :, :]
                v[..., :self.cap - shift] = v[..., shift:].clone()
        return new_origin

    def valid(self, r, row):
        """the columns of utterance r that hold results: level l up to its frontier, skip up to level 1's, y up to level L's"""
        sl, f = self.items(r), row.rel(row.prev)
        return [self.hist.t[l, sl, :, :f[l]] for l in range(self.L + 1)] + [self.skip.t[sl, :, :f[1]], self.y.t[sl, :, :f[self.L]]]

    def tails(self, r, row):
        sl, f = self.items(r), row.rel(row.prev)
        return [self.hist.t[l, sl, :, f[l]:] for l in range(self.L + 1)] + [self.skip.t[sl, :, f[1]:], self.y.t[sl, :, f[self.L]:]]

    def snapshot(self):
        return [b.t.clone() for b in (self.hist, self.skip, self.y)]

    def assert_history_kept(self, snap, r, before, what):
        """what was valid before the step (level l in front of its old frontier `before[l]`, skip and y in front of level L's) still has the
        bits of the copy taken before the call"""
        sl, L = self.items(r), self.L
        for l in range(L + 1):
            assert torch.equal(self.hist.t[l, sl, :, :before[l]], snap[0][l, sl, :, :before[l]]), f"{what}: level {l} was rewritten in front of its frontier"
        assert torch.equal(self.skip.t[sl, :, :before[L]], snap[1][sl, :, :before[L]]), f"{what}: skip was rewritten where its sum was complete"
        assert torch.equal(self.y.t[sl, :, :before[L]], snap[2][sl, :, :before[L]]), f"{what}: y was rewritten in front of its frontier"

    def check(self, what):
        for b in self.state() + [self.scratch]:
            guards_intact(b, what)


def names(L):
    return [f"level {l}" for l in range(L + 1)] + ["skip", "y"]


def assert_same_state(a, ra, b, rb, row, what):
    """utterance ra of buffer set a against utterance rb of set b, both at `row`: no NaN left (a column the call should have written), the
    valid columns equal, the columns at and behind the frontiers still the set's fill (nothing written there)"""
    for name, u, v in zip(names(row.L), a.valid(ra, row), b.valid(rb, row)):
        assert not bool(torch.isnan(u).any()), f"{what}: {name}: a column the step should have written is still NaN"
        assert torch.equal(u, v), f"{what}: {name} differs in {int((u != v).sum())} elements"
    for s, r in ((a, ra), (b, rb)):
        for name, u in zip(names(row.L), s.tails(r, row)):
            assert bool((u == s.fill).all()), f"{what}: {name} was written at or behind its frontier"


def out_lengths(rows, lengths, dev):
    return torch.tensor([max(0, n - row.origin) for row, n in zip(rows, lengths)], dtype=torch.int64, device=dev)


def step_ex(bufs, row, nxt, lengths, group):
    """dmel_wavenet_stream_step_ex: one row of frontiers for all items of the set; lengths per `group` items, in absolute frames"""
    tab = C.c_int64 * (bufs.L + 1)
    ol = torch.tensor([max(0, n - row.origin) for n in lengths], dtype=torch.int64, device=bufs.dev)
    assert len(lengths) * group == bufs.N
    h = native(bufs.m, bufs.dev)
    return lib().dmel_wavenet_stream_step_ex(h, ptr(bufs.x), bufs.hist.ptr(), bufs.skip.ptr(), None, bufs.y.ptr(), bufs.scratch.ptr(), bufs.N,
                                             bufs.cap, tab(*row.rel(row.prev)), tab(*row.rel(nxt)), ol.data_ptr(), group, row.origin, stream())


def step_items(bufs, rows, nxts, lengths, layered):
    L, R = bufs.L, len(rows)
    tab = C.c_int64 * (R * (L + 1))
    ol = out_lengths(rows, lengths, bufs.dev)
    fn = lib().dmel_wavenet_stream_step_items_layered if layered else lib().dmel_wavenet_stream_step_items
    h = native(bufs.m, bufs.dev)
    return fn(h, ptr(bufs.x), bufs.hist.ptr(), bufs.skip.ptr(), None, bufs.y.ptr(), bufs.scratch.ptr(), bufs.N, bufs.cap,
              tab(*sum((row.rel(row.prev) for row in rows), [])), tab(*sum((row.rel(n) for row, n in zip(rows, nxts)), [])),
              ol.data_ptr(), bufs.G, (C.c_int64 * R)(*[row.origin for row in rows]), stream())


def stream_input(stack, N, dev):
    C_res, Cin, L, cycle = stack
    g = torch.Generator().manual_seed(C_res + 7 * L)
    return torch.randn(N, Cin or C_res, STREAM_T, generator=g).to(dev)


def whole_forward(dev, m, x_abs, lengths, group):
    """dmel_wavenet_forward of the whole input (T > 96: the layered path), the output mask of the streaming step"""
    rc, y, _ = forward(dev, m, In(x_abs.cpu(), dev), STREAM_T, None, Lens(lengths, dev), group, "whole input", N=x_abs.shape[0])
    check(rc)
    return y.check("whole input")


def plain_ops(variant):
    """(upto, final) of the lockstep sequence; "rebase" between the fourth and the fifth push.  Variant 0 ends with a final step that
    carries the last 21 columns and a second final call that has nothing left; variant 1 reaches T mid-stream on the upper levels and
    finishes them in a final call with no new level-0 column."""
    ops, upto = [], 0
    for k, n in enumerate(PUSHES):
        if k == 4:
            ops.append("rebase")
        upto += n
        ops.append((upto, False))
    return ops + [(STREAM_T, variant == 0), (STREAM_T, True)]


@pytest.mark.parametrize("k", range(len(STREAM_STACKS)), ids=lambda k: stack_id(STREAM_STACKS[k]))
def test_one_launch_push_equals_the_layered_push_after_every_step(dev, monkeypatch, k):
    stack = STREAM_STACKS[k]
    C_res, Cin, L, cycle = stack
    assert eligible(C_res, Cin, None, False, cycle) and L <= MAX_STREAM_L
    m, _ = build_stack(*stack)
    x_abs = stream_input(stack, N_ITEMS, dev)
    one, lay = Bufs(m, 1, N_ITEMS, STREAM_CAP, HUGE, dev), Bufs(m, 1, N_ITEMS, STREAM_CAP, 0.0, dev)
    row = Row(L, cycle)
    monkeypatch.delenv("DMEL_WAVENET_STREAM_FUSED", raising=False)
    for step, op in enumerate(plain_ops(k % 2)):
        what = f"{stack_id(stack)} step {step} {op}"
        if op == "rebase":
            o = one.rebase(0, row)
            assert o == lay.rebase(0, row) and o > 0
            row.origin = o
            continue
        upto, final = op
        nxt = row.frontiers(upto, final)
        one.prepare(0, row, nxt, x_abs)
        lay.prepare(0, row, nxt, x_abs)
        snap, before = one.snapshot(), row.rel(row.prev)
        with Prof() as p1:
            check(step_ex(one, row, nxt, STREAM_LENS, GROUP), what)
        monkeypatch.setenv("DMEL_WAVENET_STREAM_FUSED", "0")
        with Prof() as p0:
            check(step_ex(lay, row, nxt, STREAM_LENS, GROUP), what + " layered")
        monkeypatch.delenv("DMEL_WAVENET_STREAM_FUSED")
        # sub-steps: a level advances at most SUBSTEP columns per launch, so the push of 97 is two launches: 96 columns and one
        most = max(n - p for n, p in zip(nxt, row.prev))
        assert (p1.launches == min(most, 1) if most <= SUBSTEP else p1.launches >= 2), (what, p1.launches, most)
        if max(n - p for n, p in zip(nxt[1:], row.prev[1:])) > 0:       # a block has new columns: two launches per block, layered
            assert p0.launches > p1.launches, (what, p1.launches, p0.launches)
        assert not (upto, final) == (sum(PUSHES[:3]), False) or p1.launches == 2, (what, p1.launches)
        row.prev = nxt
        assert_same_state(one, 0, lay, 0, row, what)
        one.assert_history_kept(snap, 0, before, what)
        one.check(what)
        lay.check(what)
    assert row.prev == [STREAM_T] * (L + 1) and row.origin > 0
    whole = whole_forward(dev, m, x_abs, STREAM_LENS, GROUP)
    assert torch.equal(one.y.t[:, :, :STREAM_T - row.origin], whole[:, :, row.origin:]), "the streamed y is not the whole-sequence forward"
    for n in range(N_ITEMS):
        lim = max(0, STREAM_LENS[n // GROUP] - row.origin)
        assert bool((one.y.t[n, :, lim:STREAM_T - row.origin] == 0).all())


def utterance_ops(r):
    """The per-utterance sequences of the per-item test (one entry per global step; None = an idle row): the pushes rotated by r.
    Utterance 0 is re-based after its fourth push (origin > 0 next to rows at 0), utterance 1 reaches T mid-stream and ends with a
    final call that adds no level-0 column, utterance 2 is idle in every second step."""
    sizes = PUSHES[r:] + PUSHES[:r]
    ops, upto = [], 0
    for k, n in enumerate(sizes):
        if r == 0 and k == 4:
            ops.append("rebase")
        upto += n
        ops.append((upto, False))
    ops += [(STREAM_T, False), (STREAM_T, True)] if r == 1 else [(STREAM_T, True)]
    if r == 2:
        ops = [o for op in ops for o in (None, op)]
    return ops


ITEM_LENS = [230, 181, 200]


@pytest.mark.parametrize("k", range(len(STREAM_STACKS)), ids=lambda k: stack_id(STREAM_STACKS[k]))
def test_per_item_push_equals_the_layered_per_item_push_and_every_single_run(dev, monkeypatch, k):
    stack = STREAM_STACKS[k]
    C_res, Cin, L, cycle = stack
    m, _ = build_stack(*stack)
    R = 3
    x_abs = stream_input(stack, R * GROUP, dev)
    monkeypatch.delenv("DMEL_WAVENET_STREAM_FUSED", raising=False)
    one, lay = Bufs(m, R, GROUP, STREAM_CAP, HUGE, dev), Bufs(m, R, GROUP, STREAM_CAP, 0.0, dev)
    rows = [Row(L, cycle) for _ in range(R)]
    queues = [utterance_ops(r) for r in range(R)]
    blocks_seen = set()
    step = 0
    while any(queues):
        nxts = []
        for r, q in enumerate(queues):
            if q and q[0] == "rebase":
                q.pop(0)
                o = one.rebase(r, rows[r])
                assert o == lay.rebase(r, rows[r]) and o > 0
                rows[r].origin = o
            op = q.pop(0) if q else None
            nxts.append(list(rows[r].prev) if op is None else rows[r].frontiers(*op))
        what = f"{stack_id(stack)} per-item step {step}"
        for r in range(R):
            one.prepare(r, rows[r], nxts[r], x_abs)
            lay.prepare(r, rows[r], nxts[r], x_abs)
        blocks_seen.add(tuple(-(-max(n - p for n, p in zip(nxts[r], rows[r].prev)) // 32) for r in range(R)))
        snap, before = one.snapshot(), [row.rel(row.prev) for row in rows]
        check(step_items(one, rows, nxts, ITEM_LENS, layered=False), what)
        check(step_items(lay, rows, nxts, ITEM_LENS, layered=True), what + " layered")
        for r in range(R):
            rows[r].prev = nxts[r]
            assert_same_state(one, r, lay, r, rows[r], f"{what} utterance {r}")
            one.assert_history_kept(snap, r, before[r], f"{what} utterance {r}")
        one.check(what)
        lay.check(what)
        step += 1
    assert any(len(set(b)) == R for b in blocks_seen), "no launch had rows of three different block counts"
    assert any(0 in b and max(b) > 0 for b in blocks_seen) and rows[0].origin > 0 and rows[1].origin == rows[2].origin == 0
    # every utterance alone, through dmel_wavenet_stream_step_ex on its own buffers
    for r in range(R):
        alone, row = Bufs(m, 1, GROUP, STREAM_CAP, HUGE, dev), Row(L, cycle)
        xa = x_abs[one.items(r)].contiguous()
        for op in utterance_ops(r):
            if op is None:
                continue
            if op == "rebase":
                row.origin = alone.rebase(0, row)
                continue
            nxt = row.frontiers(*op)
            alone.prepare(0, row, nxt, xa)
            check(step_ex(alone, row, nxt, [ITEM_LENS[r]], GROUP), f"utterance {r} alone")
            row.prev = nxt
        assert row.prev == rows[r].prev and row.origin == rows[r].origin
        assert_same_state(one, r, alone, 0, row, f"{stack_id(stack)} utterance {r} against its single run")
        alone.check(f"utterance {r} alone")


def test_thirty_three_blocks_run_layered_and_the_per_item_entry_refuses_them(dev, monkeypatch):
    """L = kStreamMaxL + 1 on an otherwise eligible stack: dmel_wavenet_stream_step_ex serves it layer by layer (its y is the
    whole-sequence forward), dmel_wavenet_stream_step_items answers DMEL_EUNSUPPORTED with every buffer untouched."""
    stack = (70, 10, MAX_STREAM_L + 1, 4)
    C_res, Cin, L, cycle = stack
    assert eligible(C_res, Cin, None, False, cycle) and L > MAX_STREAM_L
    monkeypatch.delenv("DMEL_WAVENET_STREAM_FUSED", raising=False)
    m, _ = build_stack(*stack)
    x_abs = stream_input(stack, N_ITEMS, dev)
    bufs, row = Bufs(m, 2, GROUP, STREAM_CAP, HUGE, dev), Row(L, cycle)
    before = [b.base.clone() for b in bufs.state()]
    rc = step_items(bufs, [row, Row(L, cycle)], [row.frontiers(40, False)] * 2, STREAM_LENS, layered=False)
    torch.cuda.synchronize()
    assert rc == DMEL_EUNSUPPORTED, rc
    assert all(torch.equal(b.base, a) for b, a in zip(bufs.state(), before)), "a refused per-item step wrote a buffer"
    for upto, final in ((150, False), (STREAM_T, True)):
        nxt = row.frontiers(upto, final)
        for r in range(2):
            bufs.prepare(r, row, nxt, x_abs)
        with Prof() as prof:
            check(step_ex(bufs, row, nxt, STREAM_LENS, GROUP), "33 blocks")
        assert prof.launches > 2 * L, prof.launches
        row.prev = nxt
        bufs.check("33 blocks")
    whole = whole_forward(dev, m, x_abs, STREAM_LENS, GROUP)
    assert torch.equal(bufs.y.t[:, :, :STREAM_T], whole)
