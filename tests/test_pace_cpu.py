"""The speaking-rate rule on the host (dmel_codec_amd/utils/pace.py): the properties its docstring promises, the integer helpers a
pool sizes its outputs with, and its quality on a synthetic voiced signal."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import pace
from dmel_codec_amd.utils.echo import sum8

RATE = 1000                                             # at 1000 Hz a millisecond is a sample: hop_ms = H and search_ms = D


def config(H, D, **kw):
    cfg = pace.PaceConfig(hop_ms=float(H), search_ms=float(D), **kw)
    assert cfg.samples(RATE) == (H, D)
    return cfg


def noise(n, seed=0, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def voiced(n, rate=24000, seed=0):
    """harmonics 1 .. 7 of 120 Hz at 1 / h, 5 % vibrato at 3 Hz, 40 % tremolo at 2 Hz, a level of 0.3, white noise at 0.003"""
    t = np.arange(n) / rate
    ph = 2 * np.pi * np.cumsum(120.0 * (1 + 0.05 * np.sin(2 * np.pi * 3 * t))) / rate
    x = sum(np.sin(h * ph) / h for h in range(1, 8)) * (1 + 0.4 * np.sin(2 * np.pi * 2 * t))
    x = x / np.abs(x).max() * 0.3 + 0.003 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def nominal(L, requests, H, initial=1000):
    """a_k of every frame of a stream of L samples, by the definition: a_0 = 0, a_k = a_{k-1} + Ha(rate in force at a_{k-1})"""
    a = []
    at = 0
    while at < L:
        a.append(at)
        r = initial
        for P, permille in requests:
            if P <= at:
                r = permille
        at += (H * r + 500) // 1000
    return a


def length(L, requests, H, initial=1000):
    a = nominal(L, requests, H, initial)
    return (len(a) - 1) * H + min(H, L - a[-1]) if a else 0


def bits(t):
    return (t.numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def in_calls(x, cuts, requests, cfg, check=True):
    """the stream in calls cut at `cuts`, the last one final; with check, the integer helpers are held to what scan did"""
    H, D = cfg.samples(RATE)
    st, at, ints = None, 0, pace.FRESH
    ys, offs, scores, worst = [], [], [], 0
    ends = list(cuts) + [len(x)]
    for i, c in enumerate(ends):
        fin = i == len(ends) - 1
        y, st, o, q = pace.scan(x[at:c], requests, cfg, RATE, state=st, final=fin)
        if check:
            ints, frames, n_out = pace.advance(ints, requests, c - at, fin, H, D, cfg.initial_permille)
            assert ints == pace.ints_of(st) and frames == o.shape[0] == q.shape[0] and n_out == y.shape[0]
            assert int(st[pace.I_HOLD]) == ints[3] - pace.keep_from(ints, H, D, fin)
            assert n_out <= pace.max_out(c - at, H, D)
        worst = max(worst, int(st[pace.I_HOLD]))
        ys.append(y.numpy()), offs.append(o.numpy()), scores.append(q.numpy())
        at = c
    assert worst < 2 * H + 2 * D                                               # the held count
    return np.concatenate(ys), st, np.concatenate(offs), np.concatenate(scores)


@pytest.mark.parametrize("H,D", [(64, 8), (64, 0), (240, 156)])
def test_rate_1000_is_the_identity(H, D):
    cfg = config(H, D)
    for L in (0, 1, H - 1, H, H + 1, 5 * H + 3):
        x = noise(L, L)
        x[:min(L, 3)] = np.float32(-0.0)                                       # the copy keeps a negative zero
        y, st, off, q = pace.scan(x, [], cfg, RATE, final=True)
        assert np.array_equal(bits(y), bits(x)), L
        assert (off.numpy() == 0).all() and (q.numpy() == 0).all() and off.shape[0] == -(-L // H)
        rep = pace.report(st)
        assert (rep.frames, rep.natural, rep.searched, rep.quiet, rep.samples_in, rep.samples_out) == (-(-L // H), -(-L // H), 0, 0, L, L)
        y2, st2, _, _ = in_calls(x, [L // 3, L // 2], [], cfg)
        assert np.array_equal(bits(y2), bits(x)) and torch.equal(st, st2)


@pytest.mark.parametrize("H,D", [(64, 8), (64, 0), (128, 100)])
def test_the_output_length_is_the_integer_formula(H, D):
    cfg = config(H, D)
    L = 31 * H + 17
    x = noise(L, 3)
    for r in (500, 750, 999, 1001, 1500, 2000):
        y = pace.scan(x, [(0, r)], cfg, RATE, final=True)[0]
        assert y.shape[0] == length(L, [(0, r)], H)
        also = pace.scan(x, [], config(H, D, initial_permille=r), RATE, final=True)[0]
        assert np.array_equal(bits(y), bits(also))
    twice = [(5 * H + 1, 1700), (14 * H, 600)]
    y, st, off, _ = pace.scan(x, twice, cfg, RATE, final=True)
    a = nominal(L, twice, H)
    assert y.shape[0] == length(L, twice, H) and off.shape[0] == len(a)
    assert pace.ints_of(st)[:2] == (len(a), a[-1]) and pace.report(st).permille == 600
    assert abs(pace.report(st).ratio - y.shape[0] / L) < 1e-12


@pytest.mark.parametrize("H,D", [(64, 8), (64, 0), (64, 64)])
def test_any_split_gives_the_bits_of_one_call(H, D):
    cfg = config(H, D)
    L = 23 * H + 5
    x = noise(L, 7)
    x[9 * H:11 * H] = 0.0                                                      # a quiet stretch on the way
    g = np.random.default_rng(H + D)
    for requests in ([(0, 1500)], [(0, 700)], [(0, 1010)], [(3 * H, 2000), (10 * H + 3, 500), (15 * H, 1250)]):
        y, st, off, q = pace.scan(x, requests, cfg, RATE, final=True)
        assert pace.report(st).searched > 0 or requests == [(0, 1010)]        # the slow drift stays inside a wide D

        def same(cuts):
            y2, st2, off2, q2 = in_calls(x, cuts, requests, cfg)
            assert np.array_equal(bits(y2), bits(y)) and np.array_equal(off2, off.numpy()) and np.array_equal(bits(q2), bits(q)), cuts
            assert torch.equal(st2, st), cuts

        for _ in range(12):
            same(sorted(g.integers(0, L + 1, size=int(g.integers(1, 9))).tolist()))
        a = nominal(L, requests, H)
        bounds = [H] + [max(a[k - 1] + 2 * H, a[k] + H) + D for k in range(1, len(a))]
        for b in bounds:                                                       # one sample on either side of every readiness bound
            for c in (b - 1, b, b + 1):
                if 0 <= c <= L:
                    same([c])
        same([b for b in bounds if b <= L])
        same([b - 1 for b in bounds if b <= L])


def test_the_tie_rule_smaller_offset_then_the_negative_one():
    # noise read from a table of 24 samples: candidates 24 apart see identical segments, hence identical values q
    H, D, P = 64, 16, 24
    x = np.tile(noise(P, 11), 40)[:12 * H]
    _, st, off, q = pace.scan(x, [(0, 2000)], config(H, D), RATE, final=True)
    # frame 1: t = 64, a_1 = 128: the segments at d = 8 (128 + 8 - 64 = 72 = 3 P) and d = -16 (48 = 2 P) are the template itself
    T = x[64:128]
    q8, q16 = [sum8(T * x[128 + d:192 + d]) ** 2 / (sum8(x[128 + d:192 + d] ** 2) + np.float32(1e-12)) for d in (8, -16)]
    assert q8 == q16 and off[1] == 8 and q[1] == q8
    # a table of 16 samples, a_1 = 88: t - a_1 = -24, so d = -8 and d = 8 both see the template: the negative one wins
    H, D, P = 64, 8, 16
    x = np.tile(noise(P, 12), 60)[:12 * H]
    assert (H * 1375 + 500) // 1000 == 88
    _, st, off, q = pace.scan(x, [(0, 1375)], config(H, D), RATE, final=True)
    T = x[64:128]
    qm, qp = [sum8(T * x[88 + d:152 + d]) ** 2 / (sum8(x[88 + d:152 + d] ** 2) + np.float32(1e-12)) for d in (-8, 8)]
    assert qm == qp and off[1] == -8 and q[1] == qm
    assert pace.report(st).last_offset == int(off[-1]) and pace.report(st).last_score == float(q[-1])


def test_a_template_below_the_floor_is_quiet_and_sits_on_the_nominal_position():
    H, D = 64, 8
    x = noise(12 * H, 5)
    x[:4 * H] *= np.float32(1e-5)                                              # energy of a template: 64 * 9e-12, below 1e-6
    y, st, off, q = pace.scan(x, [(0, 2000)], config(H, D), RATE, final=True)
    rep = pace.report(st)
    assert rep.quiet >= 1 and off[1] == 0 and q[1] == 0 and rep.frames == rep.natural + rep.searched + rep.quiet
    W = pace.weight_table(H)
    m = x[128:192] - x[64:128]
    m = W * m
    assert np.array_equal(bits(y[H:2 * H]), bits(x[64:128] + m))               # frame 1: old at t = 64, new at a_1 = 128
    loud = pace.scan(x, [(0, 2000)], config(H, D, floor=0.0), RATE, final=True)[1]
    assert pace.report(loud).quiet == 0


def test_a_search_of_width_zero():
    H = 64
    x = noise(20 * H + 9, 8)
    y, st, off, q = pace.scan(x, [(0, 1500)], config(H, 0), RATE, final=True)
    rep = pace.report(st)
    assert y.shape[0] == length(x.shape[0], [(0, 1500)], H) and (off.numpy() == 0).all() and rep.searched == rep.frames - 1
    assert int(off.shape[0]) == rep.frames


def test_requests_and_configs_that_are_refused():
    with pytest.raises(ValueError, match="not in front of"):
        pace.check_request((99, 1200), fed=100)
    with pytest.raises(ValueError, match="not in front of"):
        pace.check_request((150, 1200), fed=100, after=151)
    assert pace.check_request((100, 1200), fed=100) == (100, 1200)
    for bad in ((100, 499), (100, 2001), (100, 1200.0), (100.0, 1200), (100, True), 7, (1, 2, 3)):
        with pytest.raises(ValueError):
            pace.check_request(bad)
    x = noise(500, 1)
    with pytest.raises(ValueError):
        pace.scan(x, [(200, 1500), (100, 700)], config(64, 8), RATE, final=True)
    with pytest.raises(ValueError):
        pace.scan(x.astype(np.float64), [], config(64, 8), RATE, final=True)
    for kw in (dict(hop_ms=0.0), dict(eps=0.0), dict(floor=-1.0), dict(initial_permille=2500), dict(initial_permille=1000.0),
               dict(search_ms=float("nan"))):
        with pytest.raises(ValueError):
            pace.PaceConfig(**kw)
    for rate, kw in ((4000, {}), (96000, {}), (24000, dict(search_ms=30.0)), (24000.0, {})):
        with pytest.raises(ValueError):
            pace.PaceConfig(**kw).samples(rate)
    assert pace.PaceConfig().samples(24000) == (240, 156) and pace.PaceConfig().samples(8000) == (80, 52)
    assert pace.PaceConfig().state_words(24000) == 16 + 2 * 240 + 2 * 156
    cfg = pace.PaceConfig(hop_ms=8.0, initial_permille=1250)
    assert pace.PaceConfig.from_dict(cfg.as_dict()) == cfg and pace.as_config(True) == pace.PaceConfig()
    assert pace.as_config(None) is None and pace.as_config(False) is None and pace.as_config(cfg) is cfg
    with pytest.raises(ValueError):
        pace.as_config(1250)


def test_scan_modifies_no_argument_and_an_idle_call_returns_the_state():
    cfg = config(64, 8)
    x = noise(1000, 2)
    x0 = x.copy()
    y, st, _, _ = pace.scan(x, [(0, 1500)], cfg, RATE)
    st0 = st.clone()
    y2, st2, off, q = pace.scan(x[:0], [(0, 1500)], cfg, RATE, state=st)
    assert y2.shape[0] == off.shape[0] == q.shape[0] == 0 and torch.equal(st2, st0) and torch.equal(st, st0)
    pace.scan(x[:300], [(0, 1500)], cfg, RATE, state=st, final=True)
    assert torch.equal(st, st0) and np.array_equal(x, x0)
    assert (st[13:16] == 0).all() and (st[16 + int(st[pace.I_HOLD]):] == 0).all()


def test_max_out_bounds_every_step_from_every_state():
    H, D = 64, 8
    cfg = config(H, D)
    g = np.random.default_rng(4)
    x = noise(40 * H, 9)
    for r in (500, 2000, 1000):
        for _ in range(6):
            cuts = sorted(g.integers(0, x.shape[0] + 1, size=5).tolist())
            in_calls(x, cuts, [(0, r)], cfg)                                   # asserts n_out <= max_out per call
    assert pace.max_out(0, H, D) >= 2 * H


def test_quality_on_a_synthetic_voiced_signal():
    """H = 256, D = 160, 1 s at 24 kHz of the voiced signal above.  Measured with this rule (numpy, sum8):

        permille   length   rms(y) / rms(x)   max |dy| / max |dx|   spectral peak (input: 117.0 Hz)
        1000       24000    1.0000 (bits)     1.0000                117.00
        1500       16064    0.9992            0.9702                119.75
        750        31936    0.9985            1.0000                115.54
        2000       12032    1.0014            0.9714                119.66
        500        47936    0.9960            1.0000                115.54
        1100       21790    1.0003            1.0000                116.73

    Bars: the lengths are the integer formula, exactly.  rms within 0.008 of 1: twice the worst measured deviation (0.0040), as an
    overlap-add of well-matched segments keeps the level and a mismatched one loses or gains tenths.  The largest sample step at
    most 1.01 of the input's: measured never above 1.0000; a click at a joint is a step of the order of the signal level, several
    times the input's largest step, so one percent of slack cannot hide one.  The spectral peak within 5 Hz of the input's: the
    worst measured 2.75 Hz plus one DFT bin of the shortest output (24000 / 12032 = 2.0 Hz); an octave error of the alignment would
    move it by 58 Hz or more."""
    cfg = pace.PaceConfig(hop_ms=256 / 24, search_ms=160 / 24)
    assert cfg.samples(24000) == (256, 160)
    x = voiced(24000)

    def rms(v):
        return float(np.sqrt((v.astype(np.float64) ** 2).mean()))

    def peak(v):
        return float(np.abs(np.fft.rfft(v * np.hanning(v.shape[0]), 1 << 18)).argmax()) * 24000 / (1 << 18)

    y = pace.scan(x, [], cfg, 24000, final=True)[0].numpy()
    assert np.array_equal(bits(y), bits(x))
    step, f_in = float(np.abs(np.diff(x)).max()), peak(x)
    for r, n in ((1500, 16064), (750, 31936), (2000, 12032), (500, 47936), (1100, 21790)):
        y, st, _, _ = pace.scan(x, [(0, r)], cfg, 24000, final=True)
        y = y.numpy()
        figures = (r, y.shape[0], rms(y) / rms(x), float(np.abs(np.diff(y)).max()) / step, peak(y), f_in)
        print("permille %d: length %d, rms ratio %.4f, step ratio %.4f, peak %.2f Hz (input %.2f Hz)" % figures)
        assert y.shape[0] == n == length(24000, [(0, r)], 256)
        assert abs(figures[2] - 1.0) <= 0.008, figures
        assert figures[3] <= 1.01, figures
        assert abs(figures[4] - f_in) <= 5.0, figures
        assert pace.report(st).searched > 0
