"""The fused STFT / log-mel kernel (csrc/stft_logmel.hip) against float64 at every edge of its geometry, its mel tables and its inputs.

Every accuracy case is one dmel_stft_f32 launch that writes `out` and `linear` together, from audio rows of stride L + 5 whose five
slack words are NaN (reading one poisons a frame), into buffers with a sentinel tail that must come back untouched.  It is judged twice:
against float64 in the frame-energy units of tests/stft_truth.py (e_lin, e_mel), and against the fp32 oracle only to obtain the bar,

    e_gpu <= max(3 e_ref, e_floor),

e_ref being the oracle's own error on the same input in the same test.  3 is what the project grants two different fp32 factorizations
of one transform (test_stft_magnitude_backward_matches_autograd).  e_floor covers inputs on which the oracle happens to land on the
truth (the all-zero clip); it is the kernel's own operation count behind an exact spectrum, not a tuned number:
  linear: the fp32 constant 1e-9f, one add, the 1-ulp v_sqrt -> 2 ulp = 4 eps                                  (stft_truth.floor_lin)
  mel:    + the longest summation chain, 8 fmas per chunk and one add per chunk of the widest band, 1 eps each  (stft_truth.floor_mel)
  log:    + 2 ulp of |log| and the constant 1e-5f, which stft_truth.e_mel takes out element by element before it normalises.
A case over the bar is a finding about the kernel.

The rest of the file holds launches to the BITS of other launches: a frame's arithmetic does not depend on the wave, tile slot,
workgroup or batch row it runs in; window and per-item launches at n_fft 512 / 2048 and launches with dmel_stft_set_exclusive_cu(1)
return what the plain whole-clip launch returns, in `out` and in `linear`."""
import ctypes as C

import pytest
import torch

import stft_truth as st
from conftest import report

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
TAIL = 64
BY_ID = {c.id: c for c in st.FORWARD}
_worst = {"lin": [], "mel": []}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    for kind, rows in _worst.items():       # what the accuracy cases of this session measured: the worst, and the one closest to its bar
        if rows:
            worst, near = max(rows), max(rows, key=lambda r: r[0] / r[2])
            report(f"[stft matrix] {kind}: {len(rows)} cases; worst e_gpu {worst[0]:.2f} (e_ref {worst[1]:.2f}, bar {worst[2]:.2f}) in {worst[3]}; "
                   f"closest to its bar: {near[3]}, e_gpu {near[0]:.2f} = {near[0] / near[2]:.2f} of the bar {near[2]:.2f} (e_ref {near[1]:.2f})")


# ------------------------------------------------------------------------------------ launches
def plan_of(dev, n_fft, hop, win, mel):
    from dmel_codec_amd.torch_ops import _stft_plan
    return _stft_plan(dev, mel.sr, n_fft, win, hop, mel.n_mels, float(mel.f_min), float(mel.f_max or 0.0))


def nan_slack_rows(x, slack, dev):
    buf = torch.full((x.shape[0], x.shape[1] + slack), float("nan"), device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf


def guarded(n, dev):
    return torch.full((n + TAIL,), SENTINEL, device=dev)


def unguard(buf, shape):
    n = 1
    for s in shape:
        n *= s
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "the launch wrote behind the last element of an output"
    return buf[:n].view(*shape)


def whole(dev, n_fft, hop, win, mel, x, lengths=None):
    """one dmel_stft_f32 launch -> (out (B, M, T), linear (B, T, K))"""
    from dmel_codec_amd import _lib
    B, L = x.shape
    T, K, M = L // hop, n_fft // 2 + 1, mel.n_mels
    buf = nan_slack_rows(x, 5, dev)
    out, lin = guarded(B * M * T, dev), guarded(B * T * K, dev)
    with torch.cuda.device(dev):
        p = plan_of(dev, n_fft, hop, win, mel)
        assert _lib.lib().dmel_stft_num_frames(p, L) == T
        _lib.check(_lib.lib().dmel_stft_f32(p, buf.data_ptr(), L + 5, _lib.ptr(lengths), out.data_ptr(), lin.data_ptr(), B, L,
                                            _lib.stream_ptr()), "stft")
    return unguard(out, (B, M, T)), unguard(lin, (B, T, K))


def whole_case(dev, c, x):
    return whole(dev, c.n_fft, c.hop, c.win, c.mel, x)


def window(dev, n_fft, hop, win, mel, rows, s0, first, frames, total, lengths=None):
    """one dmel_stft_window_f32 launch on rows = x[:, s0:s0 + n] -> (out (B, M, frames), linear (B, frames, K))"""
    from dmel_codec_amd import _lib
    B, n = rows.shape
    K, M = n_fft // 2 + 1, mel.n_mels
    buf = nan_slack_rows(rows, 3, dev)
    out, lin = guarded(B * M * frames, dev), guarded(B * frames * K, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_stft_window_f32(plan_of(dev, n_fft, hop, win, mel), buf.data_ptr(), n + 3, n, s0, _lib.ptr(lengths),
                                                   out.data_ptr(), lin.data_ptr(), B, first, frames, total, _lib.stream_ptr()), "stft_window")
    return unguard(out, (B, M, frames)), unguard(lin, (B, frames, K))


def items(dev, n_fft, hop, win, mel, x, wins):
    """one dmel_stft_window_items_f32 launch; wins[b] = (first frame, frames, s0, end of the buffer, total length) of row b of x
    -> (out (B, M, widest), linear (B, widest, K)), both pre-filled with the sentinel"""
    from dmel_codec_amd import _lib
    B, K, M = len(wins), n_fft // 2 + 1, mel.n_mels
    width = max(e - s for _, _, s, e, _ in wins) + 3
    buf = torch.full((B, width), float("nan"), device=dev)       # whatever lies behind an item's valid samples must not be read
    for b, (_, _, s, e, _) in enumerate(wins):
        buf[b, :e - s] = x[b, s:e].to(dev)
    tmax = max(n for _, n, _, _, _ in wins)
    out, lin = guarded(B * M * tmax, dev), guarded(B * tmax * K, dev)
    tab = torch.empty(4 * B, dtype=torch.int64, device=dev)
    I = C.c_int64 * B
    cols = [I(*[w[i] for w in wins]) for i in range(5)]          # first, frames, s0, end, total
    valid = I(*[e - s for _, _, s, e, _ in wins])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dmel_stft_window_items_f32(plan_of(dev, n_fft, hop, win, mel), buf.data_ptr(), width, width, cols[2], valid, None,
                                                         out.data_ptr(), lin.data_ptr(), B, cols[0], cols[1], cols[4], tab.data_ptr(),
                                                         _lib.stream_ptr()), "stft_window_items")
    return unguard(out, (B, M, tmax)), unguard(lin, (B, tmax, K))


def need(n_fft, hop, f0, f1):
    """samples the frames [f0, f1) read when no reflection is involved"""
    pad = (n_fft - hop) // 2
    return max(0, f0 * hop - pad), (f1 - 1) * hop - pad + n_fft


# ------------------------------------------------------------------------------------ 1. accuracy: geometry, mel tables, signals
def judge(c, x, out, lin):
    """both outputs of one launch against float64, the bar from the fp32 oracle on the same input"""
    tr = st.truth(c, x)
    mel32, lin32 = st.oracle32(c, x)
    assert out.shape == mel32.shape and lin.shape == lin32.shape
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lin).all()), "a NaN slack word was read"
    gl, rl = st.e_lin(lin, tr["mag"], tr["norm"]), st.e_lin(lin32, tr["mag"], tr["norm"])
    gm, rm = st.e_mel(out, tr["mag"], tr["norm"], tr["basis"]), st.e_mel(mel32, tr["mag"], tr["norm"], tr["basis"])
    fl, fm = st.floor_lin(), st.floor_mel(tr["basis"])
    report(f"[stft matrix] {c.id}: linear e_gpu {gl:.2f} e_ref {rl:.2f} (floor {fl:.0f}); mel e_gpu {gm:.2f} e_ref {rm:.2f} (floor {fm:.0f})")
    _worst["lin"].append((gl, rl, max(3.0 * rl, fl), c.id))
    _worst["mel"].append((gm, rm, max(3.0 * rm, fm), c.id))
    empty = ~(tr["basis"] != 0).any(dim=1)
    if bool(empty.any()):                                          # a band without a bin is log(1e-5) as fp32, exactly
        assert bool((out[:, empty.to(out.device)] == torch.log(torch.tensor(1e-5))).all()), c.id
    assert gl <= max(3.0 * rl, fl), (c.id, "linear", gl, rl)
    assert gm <= max(3.0 * rm, fm), (c.id, "mel", gm, rm)


@pytest.mark.parametrize("cid", [c.id for c in st.GEOMETRY])
def test_geometry(dev, cid):
    c = BY_ID[cid]
    x = st.signal(c)
    judge(c, x, *whole_case(dev, c, x))


@pytest.mark.parametrize("cid", [c.id for c in st.TABLES])
def test_mel_tables(dev, cid):
    c = BY_ID[cid]
    x = st.signal(c)
    judge(c, x, *whole_case(dev, c, x))


@pytest.mark.parametrize("cid", [c.id for c in st.SIGNALS])
def test_signals(dev, cid):
    c = BY_ID[cid]
    x = st.signal(c)
    judge(c, x, *whole_case(dev, c, x))


def test_lengths_mask_whole_columns_and_nothing_else(dev):
    """lengths = [0, 5 hop + 17, L + 100] on a 33-frame clip: frames at or behind lengths // hop are exactly 0.f, every other column has
    the bits of the launch without lengths, and `linear` does not know about lengths at all"""
    n_fft, hop, T = 1024, 256, 33
    L = T * hop
    x = torch.randn(3, L, generator=torch.Generator().manual_seed(33)) * 0.3
    plain_out, plain_lin = whole(dev, n_fft, hop, n_fft, st.PROD_24K, x)
    lengths = torch.tensor([0, 5 * hop + 17, L + 100], dtype=torch.int64, device=dev)
    out, lin = whole(dev, n_fft, hop, n_fft, st.PROD_24K, x, lengths)
    assert torch.equal(lin, plain_lin)
    for b, keep in enumerate((0, 5, T)):
        assert torch.equal(out[b, :, :keep], plain_out[b, :, :keep]), b
        masked = out[b, :, keep:]
        assert bool((masked.view(torch.int32) == 0).all()), b     # +0.f, bit for bit
    assert float(plain_out.abs().min()) > 0.0


# ------------------------------------------------------------------------------------ 2. a frame's arithmetic does not depend on where it runs
@pytest.mark.parametrize("n_fft", [512, 1024, 2048])
def test_a_frame_is_the_same_wherever_it_runs(dev, n_fft):
    """Frame t of x is frame t - 5 of x[5 hop:] -- another wave, another slot of the 32-frame tile and, at 65 frames, another
    workgroup -- and row 0 of a batch of 1 is row 2 of a batch of 3.  Interior frames (no reflection on either side) agree bit for bit."""
    hop, T, mel = n_fft // 4, 65, st.GEOM_MEL[n_fft]
    g = torch.Generator().manual_seed(n_fft + 5)
    x = torch.randn(1, T * hop, generator=g) * 0.3
    other = torch.randn(3, (T - 5) * hop, generator=g) * 0.3
    other[2] = x[0, 5 * hop:]
    out_a, lin_a = whole(dev, n_fft, hop, n_fft, mel, x)
    out_b, lin_b = whole(dev, n_fft, hop, n_fft, mel, other)
    lo, hi = 7, T - 3                  # frames 7 .. 61 of x = frames 2 .. 56 of the shifted clip: all samples inside both clips
    pad = (n_fft - hop) // 2
    assert (lo - 5) * hop - pad >= 0 and (hi - 1) * hop - pad + n_fft <= T * hop
    assert {t // 32 for t in range(lo, hi)} == {0, 1} and any(t // 32 != (t - 5) // 32 for t in range(lo, hi))
    assert torch.equal(lin_a[0, lo:hi], lin_b[2, lo - 5:hi - 5])
    assert torch.equal(out_a[0, :, lo:hi], out_b[2, :, lo - 5:hi - 5])


# ------------------------------------------------------------------------------------ 3. window and per-item launches at 512 and 2048
def window_setup(n_fft):
    hop, T, mel = n_fft // 4, 48, st.GEOM_MEL[n_fft]
    x = torch.randn(3, T * hop, generator=torch.Generator().manual_seed(n_fft + 48)) * 0.3
    return hop, T, mel, x


@pytest.mark.parametrize("n_fft", [512, 2048])
def test_window_launch_returns_the_bits_of_the_whole_clip(dev, n_fft):
    hop, T, mel, x = window_setup(n_fft)
    x = x[:2]
    Ls = T * hop
    out, lin = whole(dev, n_fft, hop, n_fft, mel, x)

    def same(f0, f1, s0, s1, total):
        o, l = window(dev, n_fft, hop, n_fft, mel, x[:, s0:s1].contiguous(), s0, f0, f1 - f0, total)
        assert torch.equal(o, out[:, :, f0:f1]), (f0, f1, "out")
        assert torch.equal(l, lin[:, f0:f1]), (f0, f1, "linear")

    same(0, 5, 0, need(n_fft, hop, 0, 5)[1], -1)                    # head: left reflection, the end of the signal not known
    lo, hi = need(n_fft, hop, 7, 40)
    assert lo > 0 and hi < Ls
    same(7, 40, lo, hi, -1)                                         # interior: 33 frames from frame 7, two workgroups
    same(T - 4, T, need(n_fft, hop, T - 4, T)[0], Ls, Ls)           # tail: right reflection at the known end


def items_setup():
    """three items at n_fft = 2048: 32 frames from the head, 33 interior frames from frame 7, idle"""
    n_fft = 2048
    hop, T, mel, x = window_setup(n_fft)
    lo, hi = need(n_fft, hop, 7, 40)
    wins = [(0, 32, 0, need(n_fft, hop, 0, 32)[1], -1), (7, 33, lo - 1, hi, -1), (0, 0, 0, 100, -1)]
    return n_fft, hop, mel, x, wins


def test_items_launch_returns_the_bits_of_the_whole_clip(dev):
    n_fft, hop, mel, x, wins = items_setup()
    out, lin = whole(dev, n_fft, hop, n_fft, mel, x)
    o, l = items(dev, n_fft, hop, n_fft, mel, x, wins)
    assert o.shape[2] == l.shape[1] == 33
    for b, (f, n, _, _, _) in enumerate(wins):
        assert torch.equal(o[b, :, :n], out[b, :, f:f + n]), (b, "out")
        assert torch.equal(l[b, :n], lin[b, f:f + n]), (b, "linear")
        assert bool((o[b, :, n:] == SENTINEL).all()) and bool((l[b, n:] == SENTINEL).all()), b      # behind an item's frames; all of the idle item
    assert wins[2][1] == 0 and bool((o[2] == SENTINEL).all()) and bool((l[2] == SENTINEL).all())


# ------------------------------------------------------------------------------------ 4. the 152 KB launch of dmel_stft_set_exclusive_cu(1)
def exclusive(on):
    from dmel_codec_amd import _lib
    _lib.check(_lib.lib().dmel_stft_set_exclusive_cu(int(on)), "stft_set_exclusive_cu")


def test_exclusive_cu_launches_return_the_same_bits(dev):
    """one whole-clip launch per n_fft and one per-item launch with the switch set, against the same launch with it off; one stream"""
    cases = [BY_ID[f"{n}-T33-tail"] for n in (512, 1024, 2048)]
    xs = [st.signal(c) for c in cases]
    n_fft, hop, mel, x, wins = items_setup()
    off = [whole_case(dev, c, v) for c, v in zip(cases, xs)] + [items(dev, n_fft, hop, n_fft, mel, x, wins)]
    exclusive(True)
    try:
        on = [whole_case(dev, c, v) for c, v in zip(cases, xs)] + [items(dev, n_fft, hop, n_fft, mel, x, wins)]
        torch.cuda.synchronize()
    finally:
        exclusive(False)
    for i, ((o0, l0), (o1, l1)) in enumerate(zip(off, on)):
        assert torch.equal(o0, o1) and torch.equal(l0, l1), i


def test_pad_bins_behind_a_weighted_nyquist_bin_are_the_kernels_own_zeros(dev):
    """48 kHz / 512 / 128 bands weighs the Nyquist bin, so the last chunk of the last band reads magnitude slots H + 1 .. H + 7 times a
    zero weight.  The kernel zeroes those seven slots itself; it must not rely on what the LDS held.  Here the LDS holds NaN: with the
    exclusive-CU switch every workgroup starts at LDS offset 0 of its CU, and a 2048-point launch on NaN audio over more workgroups
    than there are CUs leaves NaN in its exchange buffers and magnitude rows (the first 53 KB), which cover the 512-point kernel's pad
    slots (at 10 .. 14 KB).  0 * NaN is NaN: the launch that follows returns the bits of the plain launch only if it zeroed the slots.
    Best effort: that a workgroup starts at LDS offset 0 and finds what the previous kernel left there is how the hardware behaves, not a
    promise of the runtime.  Should LDS ever be cleared or placed elsewhere, this test cannot fail wrongly; it then only repeats
    mel-48k_512_128, and the accuracy cases (which also read pad slots, over whatever the LDS holds) remain the check."""
    c = BY_ID["mel-48k_512_128"]
    x = st.signal(c)
    assert st.mel_properties(st.mel_basis(c.mel))["nyquist"]
    want = whole_case(dev, c, x)
    from dmel_codec_amd import _lib
    nan = torch.full((1024, 32 * 512), float("nan"), device=dev)     # 1024 workgroups of 32 frames
    sink = torch.empty(1024 * 80 * 32, device=dev)
    exclusive(True)
    try:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().dmel_stft_f32(plan_of(dev, 2048, 512, 2048, st.GEOM_MEL[2048]), nan.data_ptr(), nan.shape[1], None,
                                                sink.data_ptr(), None, 1024, nan.shape[1], _lib.stream_ptr()), "stft")
        got = whole_case(dev, c, x)
        torch.cuda.synchronize()
    finally:
        exclusive(False)
    assert bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
