"""The echo rule of encode sessions on the host (utils/echo.py), without a GPU: the config and its bounds, sum8, the scan against a
sample-by-sample transcription of the module's text, its independence of how either stream was cut, the bulk delay, missing and
late far samples, the two freezes, the convergence of the rule on three synthetic far ends, the report, the refusals of the C entry
dmel_echo_items (fake pointers, never read) and the pool's bookkeeping: open(echo=), push(far=), the `echo` key and segments of a
snapshot.  Every comparison of samples and state is bit equality."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot
from dmel_codec_amd.utils import echo
from dmel_codec_amd.utils.echo import EchoConfig

RATE = 24000
f32 = np.float32


def echo_path(seed=5, taps=260, delay=40, gain=0.5):
    """an exponentially decaying random path of `taps` taps behind `delay` zeros, of norm `gain`"""
    h = np.zeros(delay + taps)
    h[delay:] = np.random.default_rng(seed).standard_normal(taps) * np.exp(-np.arange(taps) / 60.0)
    return h * (gain / np.linalg.norm(h))


def far_end(kind, n, seed=1, peak=0.2):
    rng = np.random.default_rng(seed)
    if kind == "white":
        x = rng.standard_normal(n)
    elif kind == "ar1":                                                      # pole 0.95
        v, x, acc = rng.standard_normal(n), np.empty(n), 0.0
        for i in range(n):
            acc = 0.95 * acc + v[i]
            x[i] = acc
    else:                                                                    # 29 harmonics of 120 Hz, 3 Hz amplitude modulation
        t = np.arange(n) / RATE
        x = sum(np.sin(2 * np.pi * 120.0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 30))
        x = x * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
    return (x * (peak / np.abs(x).max())).astype(f32)


def echoed(x, h):
    return np.convolve(x.astype(np.float64), h)[:x.shape[0]].astype(f32)


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------------------ the config
def test_config_bounds_and_round_trip():
    cfg = EchoConfig()
    assert (cfg.taps, cfg.block_samples, cfg.delay_samples, cfg.mu, cfg.eps, cfg.far_floor, cfg.double_talk, cfg.meter) == \
        (1024, 32, 0, 1.0, 1e-6, 1e-3, 0.5, 0.05)
    assert EchoConfig.from_dict(cfg.as_dict()) == cfg and echo.as_config(True) == cfg and echo.as_config(None) is None
    assert echo.as_config(False) is None and echo.as_config(cfg) is cfg
    for bad in (dict(taps=63), dict(taps=100), dict(taps=2112), dict(taps=True), dict(taps=64.0), dict(block_samples=8),
                dict(block_samples=20), dict(block_samples=264), dict(delay_samples=-1), dict(delay_samples=24001), dict(mu=0.0),
                dict(mu=2.0), dict(mu=math.nan), dict(eps=0.0), dict(eps=-1e-6), dict(far_floor=-1.0), dict(far_floor=math.inf),
                dict(double_talk=-0.1), dict(meter=0.0), dict(meter=1.5), dict(eps=1e-60), dict(mu="1")):
        with pytest.raises(ValueError):
            EchoConfig(**bad)
    for fine in (dict(taps=64, block_samples=16), dict(taps=2048, block_samples=256, delay_samples=24000), dict(double_talk=0.0),
                 dict(far_floor=0.0), dict(meter=1.0), dict(mu=1.99)):
        EchoConfig(**fine)
    with pytest.raises(ValueError):
        echo.as_config("on")
    with pytest.raises(TypeError):
        EchoConfig.from_dict(dict(taps=64, tail=3))
    assert EchoConfig(block_samples=24).fparams() == (1.0, float(f32(1e-6)), float(f32(1e-3)), 0.5, float(f32(0.05)), 24.0)
    assert echo.ROW_WORDS == 68112 and echo.STATE_WORDS == 2576 and echo.MAX_AHEAD == 39232


# ------------------------------------------------------------------------------------------------------------ the order
def loop_sum8(v):
    """the module's text, term by term"""
    n, s = len(v), []
    for q in range(8):
        acc = f32(0.0)
        for k in range(q * n // 8, (q + 1) * n // 8):
            acc = f32(acc + v[k])
        s.append(acc)
    return f32(f32(f32(s[0] + s[1]) + f32(s[2] + s[3])) + f32(f32(s[4] + s[5]) + f32(s[6] + s[7])))


def test_sum8_on_a_hand_checked_vector_and_against_the_loop():
    # 16 terms, two per segment: 2^24 + 1 is lost inside a segment, and the tree pairs the segments
    v = np.array([2.0 ** 24, 1, 1, 2.0 ** 24, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, -2.0 ** 25, 14], dtype=f32)
    #   segments: 2^24 (2^24 + 1 is a tie, rounded to even), 2^24 (likewise), 7, 11, 15, 19, 23, -2^25 + 14 (exact: spacing 2)
    #   tree: (2^25 + 18 -> 2^25 + 16, a tie at spacing 4) + (34 + (-2^25 + 37 -> -2^25 + 36, a tie at spacing 2)) = 16 + 70 = 86
    assert echo.sum8(v) == loop_sum8(v) == f32(86.0)
    assert float(v.astype(np.float64).sum()) == 91.0                        # the order shows: the exact sum is another number
    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 8, 9, 63, 64, 79, 95, 1055, 2303):                   # 79 = 64 + 16 - 1, 2303 = 2048 + 256 - 1: uneven segments
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
        assert echo.sum8(x) == loop_sum8(x), n
        if n and n % 8 == 0:
            assert echo._sum8_even(x) == loop_sum8(x)
    m = (rng.standard_normal((5, 3, 64)) * 100).astype(f32)
    got = echo._sum8_even(m)
    assert all(got[i, j] == loop_sum8(m[i, j]) for i in range(5) for j in range(3))


def loop_scan(d, x_at, cfg):
    """the module's text sample by sample, in Python scalars of fp32; x_at(t) -> the far samples pushed when sample t is processed
    (a count: x[:count] of the list `x_at.x`).  -> e, w, counters"""
    L, N, D = cfg.taps, cfg.block_samples, cfg.delay_samples
    mu, eps, floor, dt, meter, fN = (f32(v) for v in cfg.fparams())
    w, xd, e = [f32(0)] * L, {}, []
    sd = se = f32(0)
    adapted = frozen = missing = 0
    for t in range(len(d)):
        j = t - D
        if j < 0:
            xd[t] = f32(0)
        elif j >= x_at(t):
            xd[t], missing = f32(0), missing + 1
        else:
            xd[t] = f32(x_at.x[j])
        yhat = loop_sum8([f32(w[k] * xd.get(t - k, f32(0))) for k in range(L)])
        e.append(f32(d[t] - yhat))
        if (t + 1) % N:
            continue
        t0 = t + 1 - N
        win = [xd.get(j, f32(0)) for j in range(t0 - L + 1, t0 + N)]
        E, mx = loop_sum8([f32(v * v) for v in win]), max(abs(v) for v in win)
        db, eb = [f32(v) for v in d[t0:t0 + N]], e[t0:t0 + N]
        Ed, Ee, md = loop_sum8([f32(v * v) for v in db]), loop_sum8([f32(v * v) for v in eb]), max(abs(v) for v in db)
        if E >= floor and not (dt > 0 and md > f32(dt * mx)):
            step = f32(mu / f32(f32(fN * E) + eps))
            g = [loop_sum8([f32(eb[i] * xd.get(t0 + i - k, f32(0))) for i in range(N)]) for k in range(L)]
            w = [f32(w[k] + f32(step * g[k])) for k in range(L)]
            adapted += 1
        else:
            frozen += 1
        sd, se = f32(sd + f32(meter * f32(Ed - sd))), f32(se + f32(meter * f32(Ee - se)))
    return np.array(e, dtype=f32), np.array(w, dtype=f32), (adapted, frozen, missing, sd, se)


def test_scan_equals_the_rule_written_out_sample_by_sample():
    cfg = EchoConfig(taps=64, block_samples=16, delay_samples=3, far_floor=1e-4)
    n = 150
    x = far_end("white", n, seed=3)
    d = echoed(x, echo_path(seed=2, taps=30, delay=5)) + (np.random.default_rng(4).standard_normal(n) * 0.001).astype(f32)
    # the far end is pushed in three chunks: 60 before sample 0, 50 before sample 70 (samples 63 .. 69 miss theirs), the rest before 100
    pushes = {0: 60, 70: 110, 100: 150}

    def x_at(t):
        return max(c for at, c in pushes.items() if at <= t)
    x_at.x = x
    e_ref, w_ref, (adapted, frozen, missing, sd, se) = loop_scan(d, x_at, cfg)
    st, got, prev = None, [], 0
    for at, nxt in ((0, 70), (70, 100), (100, n)):
        out = echo.scan(d[at:nxt], x[prev:pushes[at]], cfg, st)
        got.append(out[0].numpy())
        st, prev = out[1], pushes[at]
    assert np.array_equal(np.concatenate(got), e_ref)
    words = st.numpy()
    assert np.array_equal(words.view(f32)[echo.O_W:echo.O_W + 64], w_ref) and not words[echo.O_W + 64:echo.O_E].any()
    assert tuple(words[:7]) == (n, n, n % 16, n // 16, adapted, frozen, missing) and missing == 7 - 0 and adapted > 3
    assert words.view(f32)[echo.I_SD] == sd and words.view(f32)[echo.I_SE] == se
    rep = echo.report(st, 16, RATE)
    assert rep.far_missing == 7 and rep.blocks == 9 and rep.adapted_blocks == adapted and rep.total_samples == n and rep.far_ahead == 0


# ------------------------------------------------------------------------------------------------------------ the scan
def run(d, x, cfg, mic_cuts, far_cuts, lead):
    """the clip in pieces: the mic cut at mic_cuts (cyclic), the far end cut at far_cuts (cyclic) and pushed so that it stays at
    least `lead` samples ahead of the mic samples of the step (or is exhausted)"""
    st, es, ins, res, at, fa, i, k = None, [], [], [], 0, 0, 0, 0
    while at < len(d):
        m = min(mic_cuts[i % len(mic_cuts)], len(d) - at)
        i += 1
        f0 = fa
        while fa < min(len(x), at + m + lead):
            fa = min(len(x), fa + far_cuts[k % len(far_cuts)])
            k += 1
        e, st, bi, br = echo.scan(d[at:at + m], x[f0:fa], cfg, st, far_pushed_before=f0)
        es.append(e), ins.append(bi), res.append(br)
        at += m
    return torch.cat(es), st, torch.cat(ins), torch.cat(res)


@pytest.fixture(scope="module")
def clip():
    n = 2500
    x = far_end("ar1", n, seed=7)
    d = echoed(x, echo_path(seed=8, taps=100, delay=20)) + (np.random.default_rng(9).standard_normal(n) * 0.002).astype(f32)
    return d, x


@pytest.mark.parametrize("L,N,delay", [(64, 16, 0), (128, 32, 37), (192, 24, 5)])
def test_any_split_of_either_stream_gives_the_bits_of_one_call(clip, L, N, delay):
    d, x = clip
    cfg = EchoConfig(taps=L, block_samples=N, delay_samples=delay, far_floor=1e-4)
    whole = echo.scan(d, x, cfg)
    assert whole[2].shape[0] == len(d) // N and int(whole[1][echo.I_ADAPTED]) > len(d) // N // 2
    assert not torch.equal(whole[0], torch.from_numpy(d))                   # it cancels
    for mic_cuts, far_cuts, lead in (([1], [5], 0), ([N - 1], [N + 1], 0), ([N], [1000], 7), ([N + 1], [3], N), ([7, 1, 13, 101, 997], [11, 2, 211], 0),
                                     ([3 * N + 5, 1], [17], 300), ([len(d)], [1], 0)):
        if mic_cuts == [1] and L > 64:
            continue                                                         # a call per sample: once is enough
        assert same(run(d, x, cfg, mic_cuts, far_cuts, lead), whole), (mic_cuts, far_cuts, lead)
    # a far push with an empty mic chunk, and a mic chunk with no far samples
    a = echo.scan(np.zeros(0, f32), x[:700], cfg)
    assert a[0].shape == (0,) and int(a[1][echo.I_F]) == 700 and int(a[1][echo.I_T]) == 0
    b = echo.scan(d[:700], None, cfg, a[1])
    c = echo.scan(d[700:], x[700:], cfg, b[1])
    assert torch.equal(torch.cat([b[0], c[0]]), whole[0]) and torch.equal(c[1], whole[1])
    with pytest.raises(ValueError, match="far samples"):
        echo.scan(d[:10], x[:10], cfg, a[1], far_pushed_before=699)


def test_a_zeroed_row_is_the_fresh_state_and_nothing_is_modified(clip):
    d, x = clip
    cfg = EchoConfig(taps=64, block_samples=16)
    st = torch.zeros(echo.ROW_WORDS, dtype=torch.int32)
    assert torch.equal(st, echo.fresh_state())
    d0, x0 = d.copy(), x.copy()
    assert same(echo.scan(d[:500], x[:500], cfg, st), echo.scan(d[:500], x[:500], cfg))
    assert not st.any() and np.array_equal(d, d0) and np.array_equal(x, x0)
    idle = echo.scan(np.zeros(0, f32), None, cfg, st)
    assert torch.equal(idle[1], st) and idle[2].shape == (0,)
    with pytest.raises(ValueError):
        echo.scan(d[:5].astype(np.float64), x[:5], cfg)
    with pytest.raises(ValueError):
        echo.scan(d[:5], x[:5], cfg, st[:100])
    with pytest.raises(ValueError, match="ahead"):
        echo.scan(d[:5], np.zeros(echo.MAX_AHEAD + 1, f32), cfg)


def test_delay_samples_shifts_the_far_end(clip):
    d, x = clip
    D = 37
    with_delay = echo.scan(d, x, EchoConfig(taps=64, block_samples=16, delay_samples=D))
    shifted = echo.scan(d, np.concatenate([np.zeros(D, f32), x]), EchoConfig(taps=64, block_samples=16))
    assert torch.equal(with_delay[0], shifted[0]) and torch.equal(with_delay[2], shifted[2]) and torch.equal(with_delay[3], shifted[3])
    assert torch.equal(with_delay[1][:echo.O_FAR], shifted[1][:echo.O_FAR].clone().index_put_((torch.tensor([echo.I_F]),), torch.tensor(len(x), dtype=torch.int32)))
    # the first D samples have no far sample: xd is 0 there, and that is no missing sample
    assert int(with_delay[1][echo.I_MISSING]) == 0
    assert np.array_equal(with_delay[0].numpy()[:D], d[:D])
    # a path whose bulk delay the taps alone cannot span is reached with delay_samples
    # (white far end: the echo of a path the taps do not reach is uncorrelated with what they see, so nothing is cancelled; within
    # reach the misalignment of a white far end falls by 1 - 1 / (L + N) per block, a factor e^-2 in energy per 80 blocks of 16:
    # over samples 1500 .. 2500 at least e^-2.3, a tenth -- a quarter leaves room for the gradient noise)
    xw = far_end("white", 2500, seed=12)
    dd = echoed(xw, echo_path(seed=3, taps=40, delay=100))
    short = echo.scan(dd, xw, EchoConfig(taps=64, block_samples=16, double_talk=0.0))[0].numpy()
    reach = echo.scan(dd, xw, EchoConfig(taps=64, block_samples=16, delay_samples=95, double_talk=0.0))[0].numpy()
    tail = slice(1500, 2500)
    assert (reach[tail] ** 2).sum() < 0.25 * (dd[tail] ** 2).sum() and (short[tail] ** 2).sum() > 0.5 * (dd[tail] ** 2).sum()


def test_missing_and_late_far_samples(clip):
    d, x = clip
    cfg = EchoConfig(taps=64, block_samples=16, delay_samples=4)
    # no far end at all: every sample from `delay` on misses its far sample, xd is 0, e is d, the blocks are frozen by the far floor
    e, st, _, _ = echo.scan(d[:100], None, cfg)
    assert np.array_equal(e.numpy(), d[:100]) and int(st[echo.I_MISSING]) == 96 and int(st[echo.I_FROZEN]) == 6 and int(st[echo.I_ADAPTED]) == 0
    # the far end arrives late: samples x[0 .. 96) had their turn and are dropped, x[96 ..) keep their places
    late = echo.scan(d[100:400], x[:400], cfg, st)
    holes = x[:400].copy()
    holes[:96] = 0
    ref = echo.scan(d[100:400], holes[96:], cfg, echo.scan(d[:100], holes[:96], cfg)[1])
    assert torch.equal(late[0], ref[0]) and torch.equal(late[2], ref[2])
    assert torch.equal(late[1][echo.I_MISSING + 1:], ref[1][echo.I_MISSING + 1:]) and int(late[1][echo.I_MISSING]) == 96
    rep = echo.report(late[1], 16)
    assert rep.far_missing == 96 and rep.far_samples == 400 and rep.total_samples == 400 and rep.far_ahead == 0
    # a far end that lags inside a call: the samples behind its end are counted once
    lag = echo.scan(d[:300], x[:250], cfg)
    assert int(lag[1][echo.I_MISSING]) == 300 - 4 - 250
    assert echo.report(echo.scan(np.zeros(0, f32), x[:90], cfg)[1]).far_ahead == 90


def test_the_far_floor_and_the_geigel_test_each_freeze_a_constructed_block():
    cfg = EchoConfig(taps=64, block_samples=16, far_floor=1e-3, double_talk=0.5)
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(64) * 0.1).astype(f32)
    d = np.concatenate([np.zeros(1, f32), 0.4 * x[:-1]]).astype(f32)         # a one-tap echo: |d| <= 0.4 max |x|
    # block 0 adapts; block 1: the far end falls silent long enough?  no -- its window still holds block 0: quiet far end from the start instead
    quiet = echo.scan(d[:16] * f32(1e-3), x[:16] * f32(1e-3), cfg)           # E ~ 16 * 1e-8 < far_floor
    assert (int(quiet[1][echo.I_ADAPTED]), int(quiet[1][echo.I_FROZEN])) == (0, 1) and not quiet[1][echo.O_W:echo.O_E].any()
    assert float(echo.sum8((x[:16] * f32(1e-3)) ** 2)) < 1e-3
    fine = echo.scan(d[:16], x[:16], cfg)
    assert (int(fine[1][echo.I_ADAPTED]), int(fine[1][echo.I_FROZEN])) == (1, 0) and fine[1][echo.O_W:echo.O_E].any()
    assert float(echo.sum8(x[:16] ** 2)) >= 1e-3
    # the near end talks in block 1: one sample above half the window's far peak freezes that block alone
    loud = d[:48].copy()
    loud[20] = f32(0.6) * np.abs(x[:32]).max()
    talk = echo.scan(loud, x[:48], cfg)
    assert (int(talk[1][echo.I_ADAPTED]), int(talk[1][echo.I_FROZEN])) == (2, 1)
    off = echo.scan(loud, x[:48], dataclass_replace(cfg, double_talk=0.0))   # 0 disables the test
    assert (int(off[1][echo.I_ADAPTED]), int(off[1][echo.I_FROZEN])) == (3, 0)
    # the frozen block leaves the taps as block 0 left them
    assert torch.equal(echo.scan(loud[:32], x[:32], cfg)[1][echo.O_W:echo.O_E], fine[1][echo.O_W:echo.O_E])


def dataclass_replace(cfg, **kw):
    return EchoConfig(**dict(cfg.as_dict(), **kw))


def erle_db(d, e, lo, hi):
    return 10.0 * math.log10(float((d[lo:hi].astype(np.float64) ** 2).sum()) / float((e[lo:hi].astype(np.float64) ** 2).sum()))


@pytest.mark.parametrize("kind", ["white", "ar1", "voiced"])
def test_the_rule_converges_on_three_synthetic_far_ends(kind):
    """4 s at 24 kHz, peak 0.2, no near end, a 260-tap decaying random path at delay 40 of norm 0.5, L = 512, N = 32, mu = 1: the
    ERLE over seconds 3 .. 4 is at least 10 dB (scan() gives 37.9 dB on white noise, 19.3 dB on AR(1) noise with a pole at 0.95 and
    18.3 dB on 29 harmonics of 120 Hz with 3 Hz amplitude modulation: DESIGN.md)"""
    n = 4 * RATE
    x = far_end(kind, n)
    d = echoed(x, echo_path())
    st, outs = None, []
    for at in range(0, n, 8000):                                             # a third of a second per call: the ring holds 39232 ahead
        outs.append(echo.scan(d[at:at + 8000], x[at:at + 8000], EchoConfig(taps=512, block_samples=32, mu=1.0), st))
        st = outs[-1][1]
    e, bi, br = (torch.cat([o[k] for o in outs]) for k in (0, 2, 3))
    erle = erle_db(d, e.numpy(), 3 * RATE, n)
    print(f"{kind}: ERLE over seconds 3 .. 4 = {erle:.1f} dB; report {echo.report(st)}")
    assert np.isfinite(e.numpy()).all() and erle >= 10.0
    assert bi.shape[0] == n // 32 and abs(10 * math.log10(float(bi[-750:].sum()) / float(br[-750:].sum())) - erle) < 0.01


def test_report_of_a_row():
    assert math.isnan(echo.report(echo.fresh_state()).erle_db) and echo.report(echo.fresh_state()).total_samples == 0
    st = echo.fresh_state()
    fl = st.view(torch.float32)
    st[:7] = torch.tensor([1000, 1500, 8, 31, 20, 11, 3], dtype=torch.int32)
    fl[echo.I_SD], fl[echo.I_SE] = 2.0, 0.02
    rep = echo.report(st[:16], 32, 8000)
    assert (rep.total_samples, rep.far_samples, rep.far_ahead, rep.blocks, rep.adapted_blocks, rep.frozen_blocks, rep.far_missing) == \
        (1000, 1500, 500, 31, 20, 11, 3)
    assert abs(rep.erle_db - 20.0) < 1e-4 and rep.block == 32 and rep.sample_rate == 8000
    fl[echo.I_SE] = 0.0
    assert echo.report(st).erle_db == math.inf
    fl[echo.I_SD], fl[echo.I_SE] = 0.0, 1.0
    assert echo.report(st).erle_db == -math.inf


def test_far_live_and_ring_pieces():
    cfg = EchoConfig(taps=128, block_samples=32, delay_samples=10)
    assert echo.far_live(cfg, 0, 0) == (0, 0) and echo.far_live(cfg, 0, 500) == (0, 500)
    assert echo.far_live(cfg, 1000, 1200) == (992 - 10 - 127, 1200) and echo.far_live(cfg, 1000, 3) == (855, 990)
    assert echo.ring_pieces(855, 1200) == [(855, 345), (0, 0)]
    assert echo.ring_pieces(65536 + 65000, 65536 + 65536 + 100) == [(65000, 536), (0, 100)]
    assert echo.MAX_AHEAD + echo.MAX_DELAY + echo.MAX_TAPS + echo.MAX_BLOCK <= echo.FAR_RING


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_the_entry_refuses_bad_arguments_without_a_gpu():
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    S = 2
    good = dict(first=[3, 0], n=[100, 0], far=[0x1000, None], far_n=[50, 0], ip=[64, 16, 0, 0, 0, 0],
                fp=[1.0, 1e-6, 1e-3, 0.5, 0.05, 16.0] + [0.0] * 6, pitch=echo.ROW_WORDS, out_pitch=7, S=S, samples=0x1000)

    def call(**kw):
        a = dict(good, **kw)
        n = len(a["first"])
        return lib.dmel_echo_items(a["samples"], 4096, a["S"], (C.c_int64 * n)(*a["first"]), (C.c_int64 * n)(*a["n"]),
                                   (C.c_void_p * n)(*a["far"]), (C.c_int64 * n)(*a["far_n"]), (C.c_int32 * (3 * n))(*a["ip"]),
                                   (C.c_float * (6 * n))(*a["fp"]), 0x2000, a["pitch"], 0x3000, 0x4000, a["out_pitch"], 0x5000, None)

    def fp(k, v):
        return good["fp"][:k] + [v] + good["fp"][k + 1:]

    def ip(k, v):
        return good["ip"][:k] + [v] + good["ip"][k + 1:]
    bad = [dict(S=0), dict(S=65536), dict(samples=0x1002), dict(samples=None), dict(pitch=echo.ROW_WORDS - 1), dict(n=[-1, 0]), dict(n=[2 ** 30, 0]),
           dict(far_n=[-1, 0]), dict(far=[None, None]), dict(far=[0x1001, None]), dict(first=[-1, 0]), dict(ip=ip(0, 32)), dict(ip=ip(0, 100)),
           dict(ip=ip(0, 2112)), dict(ip=ip(1, 8)), dict(ip=ip(1, 20)), dict(ip=ip(1, 264)), dict(ip=ip(2, -1)), dict(ip=ip(2, 24001)),
           dict(out_pitch=6), dict(out_pitch=-1), dict(fp=fp(0, 0.0)), dict(fp=fp(0, 2.0)), dict(fp=fp(1, 0.0)), dict(fp=fp(2, -1.0)),
           dict(fp=fp(3, math.nan)), dict(fp=fp(4, 1.5)), dict(fp=fp(4, 0.0)), dict(fp=fp(5, 17.0)), dict(fp=fp(1, math.inf))]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"echo_items" in lib.dmel_last_error(), kw
    assert b"item 0" in lib.dmel_last_error()
    # every item idle: DMEL_OK, nothing launched, the idle item's parameters are not looked at
    assert call(n=[0, 0], far_n=[0, 0], ip=[7] * 6, fp=[math.nan] * 12) == 0
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match="GPU"):
        echo.echo_items(torch.zeros(2, 64), [0, 0], [4, 0], [None, None], [EchoConfig(), None], torch.zeros(2, echo.ROW_WORDS, dtype=torch.int32),
                        torch.zeros(2, 4), torch.zeros(2, 4))


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.ecfg), list(pool._far))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.ecfg, pool._far) == before  # a refused restore takes no slot


def test_pool_bookkeeping_of_sessions_with_a_canceller(codec):
    cfg = EchoConfig(taps=128, block_samples=32, delay_samples=10)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, echo=True, far_room_samples=1000)
    assert not plain_pool.echo_on and pool.echo_on and pool.far_room == 1000 and plain_pool.cap == pool.cap
    assert codec.encode_sessions(2, echo=True).far_room == 24000
    for v in (True, cfg):
        with pytest.raises(ValueError, match="echo=True"):
            plain_pool.open(echo=v)
    assert plain_pool.open_slots == [] and plain_pool.echoes() == {}
    for bad in (dict(echo=cfg), dict(echo=True, far_room_samples=-1), dict(echo=True, far_room_samples=echo.MAX_AHEAD + 1),
                dict(echo=True, far_room_samples=1.5)):
        with pytest.raises(ValueError):
            codec.encode_sessions(2, **bad)                                   # the pool's option is a bool: configs belong to sessions
    with pytest.raises(ValueError):
        pool.open(echo="on")
    with pytest.raises(ValueError, match="level=True"):
        pool.open(echo=True, level=True)                                     # the options are independent
    assert pool.open_slots == []
    a, b, c = pool.open(echo=True), pool.open(), pool.open(echo=cfg)
    assert pool.ecfg == [EchoConfig(), None, cfg] and pool._far == [0, 0, 0]
    reps = pool.echoes()
    assert set(reps) == {a, c} and pool.buf is None and reps[c].block == 32 and reps[c].total_samples == 0 and math.isnan(reps[a].erle_db)
    with pytest.raises(ValueError, match="canceller"):
        pool.echo_blocks(b)
    # push(far=): what can be refused is refused before anything is launched (no device is needed to be refused)
    x = {a: torch.zeros(5), b: torch.zeros(5), c: torch.zeros(0)}
    assert pool._validate_far(x, None) == {}
    with pytest.raises(ValueError, match="echo=True"):
        plain_pool._validate_far({0: torch.zeros(5)}, {0: torch.zeros(5)})
    for far, match in (({b: torch.zeros(5)}, "no canceller"), ({a: torch.zeros(5, dtype=torch.float64)}, "fp32"), ({a: torch.zeros(1, 5)}, "1-D"),
                       ({a: np.zeros(5, f32)}, "fp32"), ({a: torch.zeros(1001)}, "far_room_samples"), ({a: torch.zeros(5, device="meta")}, "audio on")):
        with pytest.raises(ValueError, match=match):
            pool._validate_far(x, far)
    with pytest.raises(ValueError, match="not among the pushed"):
        pool._validate_far({a: torch.zeros(5)}, {c: torch.zeros(5)})
    ok = pool._validate_far(x, {a: torch.zeros(1000), c: torch.zeros(0)})
    assert set(ok) == {a} and pool._far == [0, 0, 0]
    # the snapshot: the keys only where a canceller is on; a fresh session owns the zeroed row, so no words
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["echo"] == EchoConfig().as_dict() and snaps[c].meta["echo"] == cfg.as_dict() and snaps[c].meta["echo_far"] == 0
    assert "echo" not in snaps[b].meta and "echo_far" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without a canceller: the snapshot of a pool without the option
    plain_pool.drop(0)
    assert all(sn.nbytes == 0 and sn.meta["layout"] == [] for sn in snaps.values())
    # the layout of a session that has seen samples: the row without its ring, then the ring's live samples
    meta = copy.deepcopy(snaps[c].meta)
    meta["schedule"]["samples"], meta["echo_far"] = 1000, 1200
    shapes = pool._park_shapes(meta)
    assert shapes[-3:] == [("echo", 1, 2576), ("echo_far.0", 1, 345), ("echo_far.1", 1, 0)]
    assert shapes[:-3] == pool._park_shapes({k: v for k, v in meta.items() if k not in ("echo", "echo_far")})
    meta["schedule"]["samples"], meta["echo_far"] = 0, 40                   # far samples alone: the row counts them
    assert pool._park_shapes(meta)[-3:] == [("echo", 1, 2576), ("echo_far.0", 1, 40), ("echo_far.1", 1, 0)]
    # a pool without the option refuses the key; an echo pool takes snapshots with and without it
    refused(plain_pool, snaps[c], "echo=True")
    assert plain_pool.restore([snaps[b]]) == [0]
    other = codec.encode_sessions(4, max_push_samples=1000, echo=True)
    assert other.restore([snaps[c], snaps[b], snaps[a]]) == [0, 1, 2] and other.ecfg == [cfg, None, EchoConfig(), None]
    assert set(other.echoes()) == {0, 2}
    refused(other, SessionSnapshot(dict(snaps[c].meta, echo=dict(snaps[c].meta["echo"], mu=2.5)), snaps[c].blob), "mu")
    refused(other, SessionSnapshot(dict(snaps[c].meta, echo=dict(snaps[c].meta["echo"], tail=3)), snaps[c].blob), "EchoConfig")
    refused(other, SessionSnapshot(dict(snaps[c].meta, echo_far=-1), snaps[c].blob), "no count")
    refused(pool, SessionSnapshot(dict(snaps[c].meta, echo_far=1001), snaps[c].blob), "far_room_samples")
    other.drop(0)
    assert set(other.echoes()) == {2}
