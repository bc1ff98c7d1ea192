"""The packet-loss concealment rule of encode sessions on the host (utils/conceal.py), without a GPU: the config and its bounds, the
periods found on table-periodic streams, the fade, recovery and mute formulas against a scalar restatement, young and silent
sessions, the independence of how samples and ranges were cut, the quality against zero fill on a voiced-like signal, the map from
lost wire frames to damaged codec-rate samples against brute force, the report, the refusals of the C entry dmel_conceal_items (fake
pointers, never read) and the pool's bookkeeping.  Every comparison of samples and state is bit equality."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot
from dmel_codec_amd.utils import conceal
from dmel_codec_amd.utils.conceal import ConcealConfig
from dmel_codec_amd.utils.echo import sum8
from dmel_codec_amd.utils.resample import sinc_resample_bank

RATE = 24000
W, PMIN, PMAX, H, D, F = 480, 60, 360, 240, 1200, 120
f32 = np.float32


def periodic(period, n=6000, seed=0):
    return np.tile(np.random.default_rng(seed + period).standard_normal(period).astype(f32) * f32(0.2), n // period + 1)[:n].copy()


def voiced(f0, n=36000, seed=0):
    """eight harmonics 0.2 / h of f0, a 3 Hz vibrato of 0.3 cycles, a 2 Hz tremolo of 0.2, noise at 0.003"""
    t = np.arange(n) / RATE
    ph = f0 * t + 0.3 * np.sin(2 * np.pi * 3.0 * t)
    x = sum(0.2 / h * np.sin(2 * np.pi * h * ph) for h in range(1, 9)) * (1.0 + 0.2 * np.sin(2 * np.pi * 2.0 * t))
    return (x + 0.003 * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def scan_cut(x, ranges, cfg, cuts):
    """the same stream in calls of the given sizes, the ranges cut with them"""
    st, ys, ps, qs, at = None, [], [], [], 0
    sizes = list(cuts) + [x.shape[0] - sum(cuts)]
    for k in sizes:
        mine = [(max(lo, at) - at, min(hi, at + k) - at) for lo, hi in ranges if lo < at + k and hi > at]
        y, st, p, q = conceal.scan(x[at:at + k], mine, cfg, st, RATE)
        ys.append(y), ps.append(p), qs.append(q)
        at += k
    return torch.cat(ys), st, torch.cat(ps), torch.cat(qs)


def restated(x, ranges, cfg):
    """the rule of the module one sample at a time in plain scalar code (the search excepted: it is handed over as `search`)"""
    Wn, Pmin, Pmax, Hn, Dn, Fn = cfg.samples(RATE)
    floor, eps, rD, rF = (f32(v) for v in cfg.fparams(RATE))
    lost_at = np.zeros(x.shape[0], dtype=bool)
    for lo, hi in ranges:
        lost_at[lo:hi] = True
    y = np.zeros_like(x)
    phase = P = k = rec = t0 = 0
    c = dict(lost=0, runs=0, muted=0, longest=0, run=0)

    def s(k):
        if P == 0 or k >= Hn + Dn:
            return f32(0.0), True
        v = y[t0 - P + k % P]
        if k < Hn:
            return v, False
        u = f32(k - Hn) * rD
        g = f32(1.0) - u
        return g * v, False

    for t in range(x.shape[0]):
        if lost_at[t]:
            if phase != 1:
                t0, k, P, phase = t, 0, 0, 1
                c["run"], c["runs"] = 0, c["runs"] + 1
                if t >= Wn + Pmax:
                    a = y[t0 - Wn:t0]
                    if sum8(a * a) >= floor:
                        best = f32(0.0)
                        for p in range(Pmin, Pmax + 1):
                            b = y[t0 - Wn - p:t0 - p]
                            cc, e = sum8(a * b), sum8(b * b)
                            q = (cc * cc) / (e + eps) if cc > 0 else f32(0.0)
                            if q > best:
                                best, P = q, p
            y[t], zero = s(k)
            k, c["lost"], c["run"], c["muted"] = k + 1, c["lost"] + 1, c["run"] + 1, c["muted"] + int(zero)
        else:
            if phase == 1:
                c["longest"], phase, rec = max(c["longest"], c["run"]), 2, Fn
            if rec > 0:
                w = f32(Fn - rec + 1) * rF
                sv, _ = s(k)
                d = x[t] - sv
                m = w * d
                y[t] = sv + m
                k, rec = k + 1, rec - 1
                if rec == 0:
                    phase = 0
            else:
                y[t] = x[t]
    return y, c, P


# ------------------------------------------------------------------------------------------------------------ the config
def test_defaults_lengths_and_refusals():
    c = ConcealConfig()
    assert (c.window_ms, c.min_period_ms, c.max_period_ms, c.hold_ms, c.fade_ms, c.recover_ms, c.floor, c.eps) == \
        (20.0, 2.5, 15.0, 10.0, 50.0, 5.0, 1e-4, 1e-12)
    assert c.samples(24000) == (W, PMIN, PMAX, H, D, F) and c.samples(16000) == (320, 40, 240, 160, 800, 80)
    assert c.fparams(24000) == tuple(float(f32(v)) for v in (1e-4, 1e-12, 1 / 1200, 1 / 121))
    assert conceal.ROW_WORDS == 16 + conceal.RING == 4112 and conceal.fresh_state().shape == (4112,)
    assert conceal.as_config(None) is None and conceal.as_config(False) is None and conceal.as_config(True) == c
    assert conceal.as_config(c) is c and ConcealConfig.from_dict(c.as_dict()) == c
    with pytest.raises(ValueError):
        conceal.as_config("on")
    for kw, words in ((dict(window_ms=160.0), "ring"),                       # W + Pmax = 3840 + 360 > 4096
                      (dict(hold_ms=100.0, fade_ms=60.0), "ring"),           # H + D + Pmax = 2400 + 1440 + 360 > 4096
                      (dict(min_period_ms=0.3), "Pmin"),                     # Pmin = 7 < 8
                      (dict(min_period_ms=16.0), "Pmin"),                    # Pmin > Pmax
                      (dict(recover_ms=0.0), "recovery"),                    # F < 1
                      (dict(window_ms=0.0), "window")):
        with pytest.raises(ValueError, match=words):
            ConcealConfig(**kw).samples(24000)
    for kw in (dict(floor=-1.0), dict(eps=0.0), dict(eps=math.nan), dict(hold_ms=math.inf), dict(fade_ms=True), dict(floor=1e-42)):
        with pytest.raises(ValueError):
            ConcealConfig(**kw)
    for rate in (0, -8000, 24000.0, True):
        with pytest.raises(ValueError):
            c.samples(rate)
    x = np.zeros(100, dtype=f32)
    for bad in ([(5, 5)], [(-1, 3)], [(90, 101)], [(10, 20), (20, 30)], [(30, 40), (10, 20)], [(2 * i, 2 * i + 1) for i in range(17)]):
        with pytest.raises(ValueError):
            conceal.scan(x, bad, c)
    with pytest.raises(ValueError):
        conceal.scan(x.astype(np.float64), [], c)
    with pytest.raises(ValueError):
        conceal.scan(x, [], c, torch.zeros(16, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("period, found", [(100, 100), (200, 200), (333, 333), (50, 100)])
def test_a_table_periodic_stream_is_continued_bit_for_bit(period, found):
    """the lag found is the table's period -- for a table of 50, the lowest lag of equal scores at or above Pmin -- so the repetition
    at full level IS the stream, and behind the recovery the stream is untouched"""
    x, cfg = periodic(period), ConcealConfig()
    lo, hi = 2000, 2480
    broken = x.copy()
    broken[lo:hi] = 7.0                                                      # the content of a lost range is ignored
    y, st, periods, scores = conceal.scan(broken, [(lo, hi)], cfg)
    y = y.numpy()
    assert periods.tolist() == [found] and periods.dtype == torch.int32 and scores.dtype == torch.float32 and float(scores[0]) > 0
    assert np.array_equal(y[:lo], x[:lo]) and np.array_equal(y[lo:lo + H], x[lo:lo + H])
    assert np.array_equal(y[hi + F:], x[hi + F:])
    assert np.abs(y[lo:hi + F] - x[lo:hi + F]).max() < 0.25                  # the fade is gentle: 240 of its 1200 samples
    rep = conceal.report(st)
    assert (rep.lost_samples, rep.runs, rep.longest_run, rep.muted_samples, rep.open, rep.period, rep.total_samples) == \
        (480, 1, 480, 0, False, found, 6000)
    assert rep.score == float(scores[0]) and rep.lost_ratio == 480 / 6000 and rep.seconds() == 0.02 and rep.samples(0.5) == 12000


@pytest.mark.parametrize("ranges", [[(2000, 2480)], [(2000, 3700)], [(1500, 1600), (1650, 1700), (3000, 5990)], [(0, 10), (900, 6000)]])
def test_fade_recovery_and_mute_follow_the_formulas(ranges):
    """sample by sample against the scalar restatement: hold, fade, mute behind H + D (counted), the cross-fade of the recovery, a
    loss inside a recovery (a new onset on the ring as it then is), a run at the very start and one that is open at the end"""
    x, cfg = voiced(163.0, 6000), ConcealConfig()
    y, st, periods, scores = conceal.scan(x, ranges, cfg)
    want, c, P = restated(x, ranges, cfg)
    assert np.array_equal(y.numpy().view(np.int32), want.view(np.int32))
    w = st.tolist()
    assert [w[i] for i in (conceal.I_LOST, conceal.I_RUNS, conceal.I_MUTED, conceal.I_LONGEST, conceal.I_RUN, conceal.I_P)] == \
        [c["lost"], c["runs"], c["muted"], c["longest"], c["run"], P]
    assert w[conceal.I_T] == 6000 and len(periods) == len(ranges) and w[13:16] == [0, 0, 0]
    if ranges[0] == (2000, 3700):
        assert c["muted"] == 1700 - H - D and not y[2000 + H + D:3700].any() and y[2000 + H + D - 1] != 0
    if ranges[-1][1] == 6000:
        assert conceal.report(st).open and conceal.report(st).longest_run == max(hi - lo for lo, hi in ranges)


def test_young_and_silent_sessions_and_no_loss():
    cfg = ConcealConfig()
    x = voiced(117.0, 3000)
    y, st, p, q = conceal.scan(x, [], cfg)
    assert np.array_equal(y.numpy().view(np.int32), x.view(np.int32)) and len(p) == 0 and len(q) == 0
    assert st[:16].tolist() == [3000] + [0] * 15
    assert np.array_equal(st[16:].view(torch.float32).numpy()[:3000], x)     # the ring is the output
    # an onset one sample before W + Pmax samples: no search, zeros, all of them muted
    lo = W + PMAX - 1
    y, st, p, q = conceal.scan(x, [(lo, lo + 100)], cfg)
    assert p.tolist() == [0] and q.tolist() == [0.0] and not y[lo:lo + 100].any() and conceal.report(st).muted_samples == 100
    y, st, p, q = conceal.scan(x, [(lo + 1, lo + 101)], cfg)
    assert p.tolist()[0] > 0 and y[lo + 1:lo + 101].any() and conceal.report(st).muted_samples == 0
    # a silent window: energy below the floor
    quiet = x.copy()
    quiet[1000:2000] *= f32(1e-4)
    y, st, p, q = conceal.scan(quiet, [(2000, 2100)], cfg)
    assert p.tolist() == [0] and q.tolist() == [0.0] and not y[2000:2100].any()
    assert float(st[conceal.I_E0:conceal.I_E0 + 1].view(torch.float32)) < 1e-4
    # an empty call leaves the row alone
    y2, st2, _, _ = conceal.scan(np.zeros(0, dtype=f32), [], cfg, st)
    assert torch.equal(st2, st) and y2.shape == (0,)


CUTS = [[2000], [2100], [2480], [2500], [2599, 1], [2100, 300, 50, 30, 1, 1, 1], [1] * 50 + [1949, 7] + [13] * 60, [4500, 300]]


@pytest.mark.parametrize("cuts", CUTS)
def test_any_cut_gives_the_bits_and_the_row_of_one_call(cuts):
    """cuts at an onset, inside a run, at its end, inside a recovery, around a loss inside a recovery, and behind a ring's length"""
    x, cfg = voiced(211.7, 6000), ConcealConfig()
    ranges = [(2000, 2480), (2530, 2560), (3000, 3001), (4400, 5000)]
    one = conceal.scan(x, ranges, cfg)
    cut = scan_cut(x, ranges, cfg, cuts)
    for a, b in zip(one, cut):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_quality_against_zero_fill(capsys):
    """SNR over every gap at least 3 dB, against the 0 dB of zeros: "clearly better than zeros" and no more"""
    cfg, table = ConcealConfig(), []
    for f0 in (87.3, 117.0, 163.0, 211.7, 297.0):
        x = voiced(f0)
        for ms in (10, 20):
            n = ms * RATE // 1000
            ranges = [(at, at + n) for at in (7000, 14011, 21503, 30007)]
            y = conceal.scan(x, ranges, cfg)[0].numpy()
            snr = [10 * math.log10(float(np.sum(x[lo:hi].astype(np.float64) ** 2) / np.sum((x[lo:hi] - y[lo:hi]).astype(np.float64) ** 2)))
                   for lo, hi in ranges]
            table.append((f0, ms, min(snr), max(snr)))
    with capsys.disabled():
        for row in table:
            print("conceal quality: f0 %.1f Hz, %d ms gaps: SNR %.1f .. %.1f dB" % row)
    assert min(r[2] for r in table) >= 3.0, table


# ------------------------------------------------------------------------------------------------------------ damaged
def host_resample(x, orig, new):
    kern, width, down, up = sinc_resample_bank(orig, new)
    n = -(-x.shape[0] // down) + 1
    xp = np.concatenate([np.zeros(width, f32), x, np.zeros(width + down * (n + 1), f32)])
    win = np.lib.stride_tricks.sliding_window_view(xp, kern.shape[1])[::down][:n]
    return (win @ kern.T).reshape(-1)[:-(-up * x.shape[0] // down)]


@pytest.mark.parametrize("orig", [8000, 48000, 44100])
def test_damaged_covers_every_output_a_lost_frame_reaches(orig):
    """brute force: resample a clip and its silence-filled copy; every output that differs lies inside the mapped ranges, and the
    ranges are tight to one group of outputs on either side"""
    rng = np.random.default_rng(orig)
    x = rng.standard_normal(orig // 4).astype(f32)
    wire = [(0, 37), (orig // 50, orig // 50 + orig // 50), (orig // 10, orig // 10 + 1), (x.shape[0] - 100, x.shape[0])]
    filled = x.copy()
    for lo, hi in wire:
        filled[lo:hi] = 0.0
    a, b = host_resample(x, orig, RATE), host_resample(filled, orig, RATE)
    ranges = conceal.damaged(wire, orig, RATE)
    inside = np.zeros(a.shape[0] + 10 ** 4, dtype=bool)
    for lo, hi in ranges:
        assert 0 <= lo < hi
        inside[lo:hi] = True
    differs = np.nonzero(a != b)[0]
    assert differs.size and inside[differs].all()
    assert all(l2 > h1 for (_, h1), (l2, _) in zip(ranges, ranges[1:]))     # sorted, merged: they do not touch
    g = math.gcd(orig, RATE)
    down, up = orig // g, RATE // g
    width = sinc_resample_bank(orig, RATE)[1]
    for (wlo, whi), (lo, hi) in zip(wire, ranges):                           # no wider than the windows: exact in whole groups
        assert lo == max(0, (wlo - width - down) // down + 1) * up and hi == -(-(whi + width) // down) * up
        # nothing in front of lo was unreleased when the loss arrived: its whole window lay in front of the first lost frame
        assert lo // up * down - width + 2 * width + down > wlo and (lo == 0 or (lo // up - 1) * down + width + down <= wlo)


def test_damaged_at_one_rate_and_merging():
    assert conceal.damaged([(5, 9), (100, 200)], RATE, RATE) == [(5, 9), (100, 200)]
    assert conceal.damaged([(100, 200), (5, 9), (9, 12), (150, 260), (7, 7)], 8000, 8000) == [(5, 12), (100, 260)]
    assert conceal.damaged([(160, 320), (330, 340)], 8000, RATE) == [conceal.damaged([(160, 340)], 8000, RATE)[0]]
    with pytest.raises(ValueError):
        conceal.damaged([(5, 3)], RATE, RATE)


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_conceal_entry_refuses_before_it_launches():
    """dmel_conceal_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_conceal_items"][1]) == 16
    fake = 1 << 20
    gi, gf = ConcealConfig().samples(RATE), ConcealConfig().fparams(RATE)

    def call(n_new, first=None, ranges=None, ip=None, fp=None, S=None, samples=fake, stride=9000, state=fake + (1 << 16), sp=conceal.ROW_WORDS,
             per=fake + (1 << 17), score=fake + (1 << 18), pitch=16, table=fake + (1 << 19)):
        n = len(n_new)
        first = [0] * n if first is None else first
        ranges = [[] for _ in range(n)] if ranges is None else ranges
        ip = [gi] * n if ip is None else ip
        fp = [gf] * n if fp is None else fp
        flat = [v for r in ranges for v in ([x for p in r for x in p] + [0] * 32)[:32]]
        rc = lib.dmel_conceal_items(samples, stride, n if S is None else S, (C.c_int64 * n)(*first), (C.c_int64 * n)(*n_new),
                                    (C.c_int32 * n)(*[len(r) for r in ranges]), (C.c_int32 * (32 * n))(*flat),
                                    (C.c_int32 * (6 * n))(*[v for r in ip for v in r]), (C.c_float * (4 * n))(*[v for r in fp for v in r]),
                                    state, sp, per, score, pitch, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    def iw(k, v):
        return [gi, gi[:k] + (v,) + gi[k + 1:]]

    def fw(k, v):
        return [gf, gf[:k] + (v,) + gf[k + 1:]]

    cases = [(dict(n_new=[5, -1]), ("item 1", "new samples")),
             (dict(n_new=[5, 1 << 30]), ("item 1", "new samples")),
             (dict(n_new=[5, 5], first=[0, -1]), ("item 1", "first column")),
             (dict(n_new=[5, 5], first=[1 << 30, 0]), ("item 0", "first column")),
             (dict(n_new=[50, 50], ranges=[[], [(2 * i, 2 * i + 1) for i in range(17)]]), ("item 1", "lost ranges")),
             (dict(n_new=[50, 50], ranges=[[(10, 10)], []]), ("item 0", "range 0")),
             (dict(n_new=[50, 50], ranges=[[], [(-1, 10)]]), ("item 1", "range 0")),
             (dict(n_new=[50, 50], ranges=[[], [(1, 10), (40, 51)]]), ("item 1", "range 1")),
             (dict(n_new=[50, 50], ranges=[[], [(1, 10), (10, 20)]]), ("item 1", "do not touch")),
             (dict(n_new=[50, 50], ranges=[[], [(20, 30), (1, 10)]]), ("item 1", "sorted")),
             (dict(n_new=[50, 50], ranges=[[(1, 2), (3, 4), (5, 6)], []], pitch=2), ("item 0", "pitch")),
             (dict(n_new=[5, 5], ip=iw(0, 484)), ("item 1", "window")),
             (dict(n_new=[5, 5], ip=iw(0, 0)), ("item 1", "window")),
             (dict(n_new=[5, 5], ip=iw(1, 7)), ("item 1", "Pmin")),
             (dict(n_new=[5, 5], ip=iw(1, 361)), ("item 1", "Pmin")),
             (dict(n_new=[5, 5], ip=iw(0, 3744)), ("item 1", "ring")),
             (dict(n_new=[5, 5], ip=iw(3, 2537)), ("item 1", "ring")),
             (dict(n_new=[5, 5], ip=iw(3, -1)), ("item 1", "hold")),
             (dict(n_new=[5, 5], ip=iw(4, -1)), ("item 1", "fade")),
             (dict(n_new=[5, 5], ip=iw(5, 0)), ("item 1", "recovery")),
             (dict(n_new=[5, 5], fp=fw(3, 1.5)), ("item 1", "rF")),
             (dict(n_new=[5, 5], fp=fw(1, 0.0)), ("item 1", "eps")),
             (dict(n_new=[5, 5], sp=conceal.ROW_WORDS - 1), ("state pitch",))]
    for k in range(4):
        for v in (-1.0, math.inf, math.nan):
            cases.append((dict(n_new=[5, 5], fp=fw(k, v)), ("item 1",)))
    for kw, words in cases:
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for S in (0, -1, 65536):
        rc, msg = call([5], S=S)
        assert rc == -1 and "65535" in msg, (S, rc, msg)
    for kw in (dict(samples=None), dict(state=None), dict(per=None), dict(score=None), dict(table=None), dict(samples=fake + 2),
               dict(state=fake + 1), dict(per=fake + 2), dict(score=fake + 1), dict(table=fake + 3), dict(stride=-1), dict(pitch=-1)):
        assert call([5], **kw)[0] == -1, kw
    # idle items: their parameters and ranges are not looked at, and a call of idle items only launches nothing
    assert call([0, 0], first=[-5, -5], ranges=[[(9, 3)], [(1, 2)] * 16], ip=[(0,) * 6] * 2, fp=[(math.nan,) * 4] * 2, pitch=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.ccfg))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.ccfg) == before              # a refused restore takes no slot


def test_pool_bookkeeping_of_concealing_sessions(codec):
    cfg = ConcealConfig(hold_ms=5.0)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, conceal=True, sample_rates=(8000,))
    assert not plain_pool.conceal_on and pool.conceal_on and plain_pool.cap == codec.encode_sessions(2, max_push_samples=4096, conceal=True).cap
    for v in (True, cfg):
        with pytest.raises(ValueError, match="conceal=True"):
            plain_pool.open(conceal=v)
    assert plain_pool.open_slots == [] and plain_pool.concealed() == {}
    with pytest.raises(ValueError):
        pool.open(conceal="on")
    with pytest.raises(ValueError):
        codec.encode_sessions(2, conceal=cfg)                               # the pool's option is a bool: configs belong to sessions
    with pytest.raises(ValueError, match="ring"):
        pool.open(conceal=ConcealConfig(window_ms=160.0))
    assert pool.open_slots == []
    a, b, c = pool.open(conceal=True), pool.open(), pool.open(conceal=cfg, sample_rate=8000, sample_format="ulaw")
    assert pool.ccfg == [ConcealConfig(), None, cfg]
    reps = pool.concealed()                                                 # nothing was pushed: no buffers, no device
    assert set(reps) == {a, c} and pool.buf is None and reps[a] == conceal.report(conceal.fresh_state(), pool.codec_rate)
    with pytest.raises(ValueError, match="concealment"):
        pool.conceal_onsets(b)
    # push(lost=): refused before anything changes, on the host
    x = torch.zeros(480)
    u = torch.zeros(160, dtype=torch.uint8)
    for audio, lost, words in (({b: x}, {b: 480}, "open\\(conceal=\\)"), ({a: x}, {a: -1}, "count"), ({a: x}, {a: 1.5}, "count"),
                               ({a: x}, {a: True}, "count"), ({a: x}, {c: 160}, "not among"), ({a: x}, {a: 4096 - 479}, "max_push_samples"),
                               ({c: u}, {c: 4000}, "max_push_samples")):
        with pytest.raises(ValueError, match=words):
            pool.push(audio, lost=lost)
    with pytest.raises(ValueError, match="conceal=True"):
        plain_pool.push({plain_pool.open(): x}, lost={0: 480})
    plain_pool.drop(0)
    assert pool.buf is None and pool._lost == [[], [], []]
    # the snapshot: the keys only where concealment is on
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["conceal"] == ConcealConfig().as_dict() and snaps[a].meta["conceal_lost"] == [] and "conceal" not in snaps[b].meta
    assert snaps[c].meta["conceal"] == cfg.as_dict() and "conceal_lost" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without the option: the snapshot of a pool without it
    plain_pool.drop(0)
    meta = copy.deepcopy(snaps[a].meta)
    meta["schedule"]["samples"] = 1
    shapes = pool._park_shapes(meta)
    assert shapes[-1] == ("conceal", 1, conceal.ROW_WORDS) and shapes[:-1] == pool._park_shapes({k: v for k, v in meta.items() if k != "conceal"})
    refused(plain_pool, snaps[a], "conceal=True")
    other = codec.encode_sessions(4, max_push_samples=1000, conceal=True)
    assert other.restore([snaps[a], snaps[b]]) == [0, 1] and other.ccfg == [ConcealConfig(), None, None, None]
    refused(other, SessionSnapshot(dict(snaps[a].meta, conceal=dict(snaps[a].meta["conceal"], pitch=3)), snaps[a].blob), "ConcealConfig")
    refused(other, SessionSnapshot(dict(snaps[a].meta, conceal_lost=[[5, 3]]), snaps[a].blob), "conceal_lost")
    refused(other, SessionSnapshot(dict(snaps[a].meta, conceal_lost=[[10, 20], [15, 30]]), snaps[a].blob), "conceal_lost")
    assert set(other.concealed()) == {0}
