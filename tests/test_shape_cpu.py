"""The reply-shaping rule on the host (dmel_codec_amd/utils/shape.py): the commanded gain, the limiter, cut invariance, the ceiling,
lengths, the stop, every refusal of the config and of the C entry (on pointers that are never read), and the pool's bookkeeping that
needs no device."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.models.stream_park import SessionSnapshot
from dmel_codec_amd.utils import shape, tones
from dmel_codec_amd.utils.shape import ShapeConfig

RATE = 24000
EPS = 2.0 ** -24                                       # half an ulp of 1.0f: the relative error of one rounded fp32 operation


def sine(n, amp, f=440.0):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / RATE)).astype(np.float32)


def noise_with_burst(n, seed=0):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 0.2).astype(np.float32)
    x[n // 2:n // 2 + n // 10] *= np.float32(12.0)
    return x


def bits(t):
    return (t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ commanded gain
def test_commanded_gain_against_float64():
    cfg = ShapeConfig()
    reqs = [(100, 2.0, 480), (300, 0.25, 1000), (2000, 0.0, 0), (2500, 3.5, 16384)]
    segs = shape.plan(reqs, cfg)
    c = shape.commanded(segs, cfg.initial_gain, 0, 20000)
    want = np.empty(20000)
    for i in range(20000):
        seg = [sg for sg in segs if sg[0] <= i]
        if not seg:
            want[i] = 1.0
            continue
        P, g0, g1, ramp = seg[-1]
        k = i - P
        want[i] = g1 if k >= ramp else g0 + (g1 - g0) * (0.5 - 0.5 * math.cos(math.pi * (k + 0.5) / ramp))
    # the table is rounded once, then a product and a sum: three roundings of values no larger than max_gain
    assert np.abs(c.astype(np.float64) - want).max() <= 3 * EPS * 2 * cfg.max_gain
    assert all(shape.gain_at(segs, 1.0, i) == c[i] for i in (0, 99, 100, 101, 299, 300, 1299, 1300, 2000, 2499, 2500, 18883, 18884))
    # an interrupted ramp: the second segment starts from the value the first had at its anchor, and that value is on neither end
    assert segs[1][1] == float(shape.gain_at(segs[:1], 1.0, 300)) and 1.0 < segs[1][1] < 2.0
    # ramp = 0 steps at the anchor; behind a ramp the gain is g1 exactly
    assert c[1999] == np.float32(0.25) and c[2000] == 0.0 and c[2499] == 0.0
    assert c[1300] == np.float32(0.25) and (c[1300:2000] == np.float32(0.25)).all() and c[2500 + 16384] == np.float32(3.5)
    # a window of the trajectory is the trajectory
    assert np.array_equal(shape.commanded(segs, 1.0, 777, 3000), c[777:3777])


def test_folding_finished_segments_is_exact():
    cfg = ShapeConfig()
    reqs = [(10, 2.0, 50), (40, 0.5, 100), (500, 1.5, 64), (700, 0.0, 32), (2000, 1.0, 10)]
    segs = shape.plan(reqs, cfg)
    c = shape.commanded(segs, 1.0, 0, 3000)
    for pos in (0, 9, 10, 39, 40, 139, 140, 141, 499, 563, 564, 565, 731, 732, 1999, 2000, 2010, 2500):
        live, base = shape.live(segs, 1.0, pos)
        assert np.array_equal(shape.commanded(live, base, pos, 3000 - pos), c[pos:]), pos
    assert shape.live(segs, 1.0, 2010) == ([], 1.0) and shape.live(segs, 1.0, 141)[0] == segs[2:] and shape.live(segs, 1.0, 141)[1] == 0.5
    # a request folded in later sees the same trajectory
    live, base = shape.live(segs[:2], 1.0, 60)
    assert shape.extend(live, base, (90, 3.0, 5)) == shape.extend(segs[:2], 1.0, (90, 3.0, 5))


# ------------------------------------------------------------------------------------------------------------ the scan
def cut_scan(z, reqs, cfg, pieces, end=None):
    """z in pieces of the given lengths (cycled), the last one final -> (y, state, peaks, gains)"""
    state, ys, pk, gn, at, k = None, [], [], [], 0, 0
    while True:
        n = pieces[k % len(pieces)]
        k += 1
        last = at + n >= len(z)
        y, state, p, g = shape.scan(z[at:at + n], reqs, cfg, RATE, end=end, state=state, final=last)
        ys.append(y), pk.append(p), gn.append(g)
        at += n
        if last:
            return torch.cat(ys), state, torch.cat(pk), torch.cat(gn)


@pytest.mark.parametrize("N", [32, 120])
@pytest.mark.parametrize("limit", [True, False])
def test_cut_invariance(N, limit):
    cfg = ShapeConfig(block_samples=N, limit=limit)
    z = noise_with_burst(11 * N + 17, seed=N)
    reqs = [(5, 2.0, 3 * N), (2 * N, 0.5, N + 3), (6 * N + 1, 3.0, 0)]
    y, st, pk, gn = shape.scan(z, reqs, cfg, RATE, final=True)
    assert y.shape[0] == z.shape[0]
    for pieces in ([1], [N - 1], [N], [N + 1], [3 * N + 5], [0, N - 1, 0, 0, 1, 2 * N]):
        y2, st2, pk2, gn2 = cut_scan(z, reqs, cfg, pieces)
        assert np.array_equal(bits(y2), bits(y)), pieces
        assert torch.equal(st2, st) and np.array_equal(bits(pk2), bits(pk)) and np.array_equal(bits(gn2), bits(gn)), pieces
    # state rows agree in the middle of the stream as well: one call of 5 N + 3 against its cuts
    one = shape.scan(z[:5 * N + 3], reqs, cfg, RATE)
    state, outs = None, []
    for a in range(0, 5 * N + 3, 7):
        o, state, _, _ = shape.scan(z[a:min(a + 7, 5 * N + 3)], reqs, cfg, RATE, state=state)
        outs.append(o)
    assert torch.equal(state, one[1]) and np.array_equal(bits(torch.cat(outs)), bits(one[0]))
    # an idle step returns the state as it is and nothing else
    idle = shape.scan(z[:0], reqs, cfg, RATE, state=one[1])
    assert torch.equal(idle[1], one[1]) and idle[0].numel() == idle[2].numel() == idle[3].numel() == 0


def test_ceiling_holds_exactly():
    cfg = ShapeConfig(block_samples=48)
    ceil = np.float32(cfg.ceiling)
    loud = [(0, 10 ** (12 / 20), 0)]                                         # +12 dB
    for z in (sine(4800, 0.9), sine(4800, 0.5, 3000.0), noise_with_burst(5000, 3)):
        y, st, _, _ = shape.scan(z, loud, cfg, RATE, final=True)
        assert y.abs().max() <= ceil and y.shape[0] == z.shape[0]
        rep = shape.report(st, 48, RATE)
        assert rep.peak_out <= float(ceil) and rep.limited_blocks > 0 and rep.limiter_min < 1.0
    for at in range(48, 96):                                                 # one full-scale spike at every position of a block
        z = np.zeros(4 * 48, dtype=np.float32)
        z[at] = 1.0
        y, st, pk, gn = shape.scan(z, loud, cfg, RATE, final=True)
        assert y.abs().max() <= ceil and shape.report(st).limited_blocks == 1
        assert y.abs().max() >= 0.9 * ceil                                   # and the spike is brought to the ceiling, not muted


def test_quality_on_a_loud_sine():
    """synthetic checks, not conformance: a +12 dB sine of amplitude 0.5 at 1 kHz (a sample falls on its crest; peak 1.99 against
    the ceiling 0.98) settles ON the ceiling.  Found on the host: limiter gain / (ceiling / peak) = 1 + 1.2e-8, a reduction of 6.155
    dB, the largest |y| the fp32 ceiling itself, nothing clamped.  The bounds are the roundings involved -- the crest sample, the
    gain, their product, the division: at most four of 2^-24 each, asserted as eight --, not what the code gave."""
    cfg = ShapeConfig()
    z = sine(24000, 0.5, 1000.0)
    y, st, pk, gn = shape.scan(z, [(0, 10 ** (12 / 20), 0)], cfg, RATE, final=True)
    rep = shape.report(st)
    want = cfg.ceiling / (0.5 * 10 ** (12 / 20))
    assert abs(rep.limiter_min / want - 1) <= 8 * EPS and abs(float(gn[-1]) / want - 1) <= 8 * EPS
    assert abs(20 * math.log10(rep.limiter_min) + 6.155) < 0.001
    assert float(y.abs().max()) <= float(np.float32(cfg.ceiling)) and rep.clamped == 0              # no overshoot, and no clamp needed
    assert float(y[12000:].abs().max()) >= cfg.ceiling * (1 - 8 * EPS)       # the steady state sits at the ceiling, not below it
    quiet = shape.scan(sine(4800, 0.4), [], cfg, RATE, final=True)
    assert np.array_equal(bits(quiet[0]), bits(sine(4800, 0.4))) and shape.report(quiet[1]).limiter_min == 1.0


def test_lengths_and_emitted():
    for N in (32, 120):
        cfg = ShapeConfig(block_samples=N)
        z = noise_with_burst(9 * N + 5, 1)
        for pieces in ([1], [N - 1], [N], [N + 1], [2 * N, 0, 3]):
            state, at, k, total = None, 0, 0, 0
            while at < len(z):
                n = min(pieces[k % len(pieces)], len(z) - at)
                k += 1
                hold = 0 if state is None else int(state[shape.I_HOLD])
                last = at + n >= len(z)
                y, state, pk, _ = shape.scan(z[at:at + n], [], cfg, RATE, state=state, final=last)
                assert y.shape[0] == shape.emitted(hold, n, N, last) and pk.shape[0] == shape.completed(hold, n, N, last)
                at, total = at + n, total + y.shape[0]
                held = at - total
                assert int(state[shape.I_HOLD]) == held and (last or held < 2 * N) and (last or at < N or held >= N)
                assert int(state[shape.I_IN]) == at and int(state[shape.I_OUT]) == total
            assert total == len(z) and int(state[shape.I_HOLD]) == 0
    assert shape.emitted(0, 100, 32, False, limit=False) == 100 and shape.completed(0, 100, 32, True, limit=False) == 0


def test_identity_without_the_limiter():
    cfg = ShapeConfig(limit=False)
    z = np.clip(noise_with_burst(3000, 5), -0.98, 0.98).astype(np.float32)
    z[7] = -0.0
    y, st, pk, gn = shape.scan(z, [], cfg, RATE)
    assert np.array_equal(bits(y), bits(z)) and pk.numel() == 0 and st.numel() == shape.HEADER
    assert shape.report(st).clamped == 0 and shape.report(st).samples_out == 3000
    loud = z.copy()
    loud[[3, 500, 2999]] = [1.5, -1.0, 0.99]
    y, st, _, _ = shape.scan(loud, [], cfg, RATE)
    assert shape.report(st).clamped == 3 and np.array_equal(y.numpy()[[3, 500, 2999]], np.float32([0.98, -0.98, 0.98]))
    assert np.array_equal(np.delete(bits(y), [3, 500, 2999]), np.delete(bits(z), [3, 500, 2999]))


def test_stop():
    cfg = ShapeConfig(block_samples=64)
    z = sine(5000, 0.7)
    ramp, now = 480, 1000
    reqs = [(now, 0.0, ramp)]
    y, st, _, _ = shape.scan(z, reqs, cfg, RATE, end=now + ramp)
    assert y.shape[0] == now + ramp and int(st[shape.I_HOLD]) == 0 and int(st[shape.I_IN]) == now + ramp
    # the last sample is at most |z| times the complement of the ramp's last step
    last = 1.0 - float(shape.ramp_table(ramp)[-1])
    assert abs(float(y[-1])) <= abs(float(z[now + ramp - 1])) * last * (1 + 4 * EPS) + 1e-12 and last < 1e-5
    assert np.array_equal(bits(y[:now - 2 * 64]), bits(shape.scan(z, [], cfg, RATE, final=True)[0][:now - 2 * 64]))
    # in pieces: the step that reaches E is the last, whatever it was handed
    state, outs = None, []
    for a in range(0, 5000, 333):
        o, state, _, _ = shape.scan(z[a:a + 333], reqs, cfg, RATE, end=now + ramp, state=state)
        outs.append(o)
        if int(state[shape.I_IN]) == now + ramp:
            break
    assert np.array_equal(bits(torch.cat(outs)), bits(y)) and torch.equal(state, st)
    # a stream that is shorter than the fade ends where it ends
    short, st2, _, _ = shape.scan(z[:1200], reqs, cfg, RATE, end=now + ramp, final=True)
    assert short.shape[0] == 1200 and int(st2[shape.I_HOLD]) == 0
    assert np.array_equal(bits(short[:1200 - 2 * 64]), bits(y[:1200 - 2 * 64])) and abs(float(short[-1])) < 0.7
    with pytest.raises(ValueError, match="end"):
        shape.scan(z[:10], reqs, cfg, RATE, end=5, state=st)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_config_refusals():
    for kw in (dict(block_samples=31), dict(block_samples=1025), dict(block_samples=64.0), dict(block_samples=True), dict(limit=1),
               dict(ceiling=0), dict(ceiling=-1.0), dict(ceiling=math.inf), dict(release=0), dict(release=1.5), dict(max_gain=0),
               dict(max_gain=math.nan), dict(initial_gain=-0.1), dict(initial_gain=4.5), dict(ceiling="1"), dict(ceiling=1e-42)):
        with pytest.raises(ValueError):
            ShapeConfig(**kw)
    assert ShapeConfig(initial_gain=0).initial_gain == 0.0 and ShapeConfig().block(RATE) == 120 and ShapeConfig().block(8000) == 40
    with pytest.raises(ValueError, match="block_samples"):
        ShapeConfig().block(4000)                                            # 5 ms are 20 samples
    with pytest.raises(ValueError, match="block_samples"):
        ShapeConfig().block(409600)
    assert ShapeConfig.from_dict(ShapeConfig(block_samples=64, limit=False).as_dict()) == ShapeConfig(block_samples=64, limit=False)
    assert shape.as_config(None) is None and shape.as_config(False) is None and shape.as_config(True) == ShapeConfig()
    with pytest.raises(ValueError, match="shape"):
        shape.as_config("yes")
    cfg = ShapeConfig()
    for bad in ((0, 4.5, 10), (0, -0.1, 10), (0, math.nan, 10), (0, 1.0, 16385), (0, 1.0, -1), (0, 1.0, 2.0), (-1, 1.0, 0), (1.5, 1.0, 0),
                (0, 1.0), (0, True, 0)):
        with pytest.raises(ValueError):
            shape.check_request(bad, cfg)
    with pytest.raises(ValueError, match="anchor"):
        shape.plan([(10, 1.0, 0), (9, 1.0, 0)], cfg)
    with pytest.raises(ValueError):
        shape.scan(np.zeros(4, np.float64), [], cfg, RATE)
    with pytest.raises(ValueError, match="state"):
        shape.scan(np.zeros(4, np.float32), [], cfg, RATE, state=torch.zeros(16, dtype=torch.int32))
    assert len(shape.ramp_table(16384)) == 16384 and np.array_equal(shape.ramp_table(100), tones.ramp_table(100))
    with pytest.raises(ValueError):
        shape.ramp_table(16385)


def test_entry_refuses_before_anything_is_read():
    """every pointer is a fake address: a call that passes the checks would fault, a refused one reads nothing"""
    L = _lib.lib()
    fake = 0x10000

    def call(n=100, hold=0, flags=2, N=64, cap=1000, fp=(0.98, 0.1, 1 / 64, 1.0, 4.0), count=0, segs=(), dst=fake, src=fake + 4, S=1,
             ramps=fake, ramp_floats=100, state=fake, pitch=16 + 127, opk=fake, ogn=fake, out_pitch=10, table=fake):
        words = list(segs) + [0] * (40 - len(segs))
        P = C.c_void_p * 1
        rc = L.dmel_shape_items(P(dst), (C.c_int64 * 1)(cap), P(src), (C.c_int64 * 1)(n), (C.c_int64 * 1)(hold), (C.c_int32 * 1)(flags),
                                (C.c_int32 * 1)(N), (C.c_float * 5)(*fp), (C.c_int32 * 1)(count), (C.c_int32 * 40)(*words), S, ramps,
                                ramp_floats, state, pitch, opk, ogn, out_pitch, table, None)
        return rc, L.dmel_last_error().decode()

    def f32(v):
        return int(np.array([v], dtype=np.float32).view(np.int32)[0])

    seg = [0, 10, 0, f32(1.0), f32(2.0)]
    refused = [dict(S=0), dict(S=65536), dict(state=None), dict(opk=None), dict(table=None), dict(table=fake + 4), dict(state=fake + 2),
               dict(ramps=None), dict(ramp_floats=-1), dict(pitch=15), dict(out_pitch=-1), dict(n=-1), dict(n=1 << 30), dict(flags=4),
               dict(flags=-1), dict(N=31), dict(N=1025), dict(hold=-1), dict(hold=128), dict(pitch=16 + 126), dict(out_pitch=0),
               dict(n=64 * 12, cap=64 * 12, out_pitch=11),                      # twelve blocks complete
               dict(n=200, cap=127), dict(n=128, cap=63), dict(flags=3, n=10, hold=100, cap=109), dict(flags=0, hold=1), dict(flags=0, cap=99),
               dict(dst=None, n=200), dict(src=None), dict(dst=fake + 1), dict(src=fake + 2),
               dict(fp=(0.0, 0.1, 1 / 64, 1.0, 4.0)), dict(fp=(0.98, 0.0, 1 / 64, 1.0, 4.0)), dict(fp=(0.98, 1.5, 1 / 64, 1.0, 4.0)),
               dict(fp=(0.98, 0.1, 2.0, 1.0, 4.0)), dict(fp=(0.98, 0.1, 1 / 64, -1.0, 4.0)), dict(fp=(0.98, 0.1, 1 / 64, 5.0, 4.0)),
               dict(fp=(math.nan, 0.1, 1 / 64, 1.0, 4.0)), dict(fp=(0.98, 0.1, 1 / 64, 1.0, math.inf)),
               dict(count=9), dict(count=-1), dict(count=1, segs=[0, 16385, 0, f32(1.0), f32(2.0)]),
               dict(count=1, segs=[0, -1, 0, f32(1.0), f32(2.0)]), dict(count=1, segs=[0, 10, 91, f32(1.0), f32(2.0)]),
               dict(count=1, segs=[0, 10, -1, f32(1.0), f32(2.0)]), dict(count=1, segs=[0, 10, 0, f32(1.0), f32(4.5)]),
               dict(count=1, segs=[0, 10, 0, f32(-1.0), f32(2.0)]), dict(count=1, segs=[0, 10, 0, f32(math.nan), f32(2.0)]),
               dict(count=1, segs=[(1 << 30) + 1, 10, 0, f32(1.0), f32(2.0)]), dict(count=2, segs=seg + [-1] + seg[1:])]
    for kw in refused:
        rc, msg = call(**kw)
        assert rc == -1 and "shape_items" in msg, (kw, rc, msg)
    assert "item 0" in call(N=31)[1] and "destination takes" in call(n=200, cap=0)[1] and "segment 0" in call(count=1, segs=[0, -1, 0, 0, 0])[1]
    # an idle item: nothing of it is looked at, and a call of idle items only launches nothing
    assert call(n=0, flags=2, N=-5, hold=-9, cap=-1, dst=None, src=None, count=99, fp=(0, 0, 0, 0, 0))[0] == 0
    assert call(n=0, flags=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1,
                       vocoder=dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                    resblock="1", resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
                                    activation="snakebeta", snake_logscale=True))


def test_pool_options_and_refusals(codec):
    plain = codec.decode_sessions(2, max_push_tokens=16, output_sample_rates=(8000,))
    pool = codec.decode_sessions(2, max_push_tokens=16, output_sample_rates=(8000,), shape=True)
    assert not plain.shape_on and pool.shape_on and pool.cap == plain.cap
    assert pool.rs.max_push == plain.rs.max_push + 2 * shape.MAX_BLOCK - 1    # what a limiter held back leaves with a later step
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="shape"):
            codec.decode_sessions(2, shape=bad)
    with pytest.raises(ValueError, match="return_audios"):
        codec.decode_sessions(2, shape=True, return_audios=False)
    with pytest.raises(ValueError, match="shape=True"):
        plain.open(shape=True)
    with pytest.raises(ValueError, match="ShapeConfig"):
        pool.open(shape="on")
    assert plain.open_slots == [] and pool.open_slots == []
    s = plain.open()
    for call in (lambda: plain.set_gain(s, -6.0), lambda: plain.stop(s), lambda: plain.shaped(), lambda: plain.shape_blocks(s),
                 lambda: plain.samples_fed(s)):
        with pytest.raises(ValueError, match="shape=True"):
            call()
    assert "shape" not in plain.snapshot([s])[s].meta
    a, b = pool.open(shape=True), pool.open()
    for call in (lambda: pool.set_gain(b, -6.0), lambda: pool.stop(b), lambda: pool.shape_blocks(b)):
        with pytest.raises(ValueError, match="without shape="):
            call()
    assert pool.open_slots == [a, b] and set(pool.shaped()) == {a}
    assert pool.shaped()[a].gain == 1.0 and pool.shaped()[a].samples_in == 0 and pool.buf is None


def test_pool_bookkeeping_of_gain_requests(codec):
    pool = codec.decode_sessions(3, max_push_tokens=16, early_emit=True, shape=True)
    a = pool.open(shape=ShapeConfig(block_samples=64, max_gain=2.0))
    assert pool.samples_fed(a) == 0 and pool.set_gain(a, -6.0) == 0 and pool.buf is None
    g = float(np.float32(10 ** (-6 / 20)))
    assert pool.sreq[a] == [(0, 1.0, g, 480)] and set(pool._sramp_off) == {480}
    assert pool.set_gain(a, float("-inf"), ramp_ms=0, at_sample=100) == 100
    assert pool.sreq[a][1] == (100, float(shape.gain_at(pool.sreq[a][:1], 1.0, 100)), 0.0, 0)
    before = copy.deepcopy(pool.sreq[a])
    for call, match in ((lambda: pool.set_gain(a, 6.1, at_sample=150), "max_gain"), (lambda: pool.set_gain(a, 0.0, ramp_ms=700, at_sample=150), "ramp"),
                        (lambda: pool.set_gain(a, 0.0, at_sample=99), "anchor"), (lambda: pool.set_gain(a, 0.0), "anchor"),
                        (lambda: pool.set_gain(a, math.nan), "gain_db"), (lambda: pool.set_gain(a, 0.0, ramp_ms=-1), "ramp_ms"),
                        (lambda: pool.set_gain(a, 0.0, at_sample=1.5), "anchor")):
        with pytest.raises(ValueError, match=match):
            call()
    assert pool.sreq[a] == before
    for k in range(6):
        pool.set_gain(a, -1.0 * k, at_sample=200 + k)
    with pytest.raises(ValueError, match="ninth"):
        pool.set_gain(a, 0.0, at_sample=300)
    assert len(pool.sreq[a]) == 8
    # the snapshot: plain values in, the same segments out; no row for a session that has fed nothing
    snap = pool.snapshot([a])[a]
    assert snap.meta["shape"] == pool.scfg[a].as_dict() and snap.meta["shape_segments"] == [list(sg) for sg in pool.sreq[a]]
    assert (snap.meta["shape_fed"], snap.meta["shape_hold"], snap.meta["shape_end"], snap.meta["shape_base"]) == (0, 0, None, 1.0)
    assert snap.nbytes == 0 and snap.meta["version"] == 1
    other = codec.decode_sessions(4, max_push_tokens=8, early_emit=True, shape=True)
    assert other.open() == 0 and other.restore([snap]) == [1]
    assert other.sreq[1] == pool.sreq[a] and other.scfg[1] == pool.scfg[a] and set(other._sramp_off) == {480} and other.sreq[0] == []
    plain = codec.decode_sessions(2, max_push_tokens=16, early_emit=True)
    with pytest.raises(ValueError, match="shape=True"):
        plain.restore([snap])
    assert plain.open_slots == []
    old = {k: v for k, v in snap.meta.items() if not k.startswith("shape")}
    assert plain.restore([SessionSnapshot(old, snap.blob)]) == [0] and other.restore([SessionSnapshot(old, snap.blob)]) == [2]
    assert other.scfg[2] is None
    for key, bad, match in (("shape_hold", 5, "counts"), ("shape_fed", -1, "counts"), ("shape_base", 9.0, "base"),
                            ("shape_segments", [[0, 1.0, 9.0, 0]], "gain"), ("shape_segments", [[5, 1.0, 1.0, 0], [4, 1.0, 1.0, 0]], "anchor"),
                            ("shape", dict(snap.meta["shape"], loudness=1), "ShapeConfig"), ("shape", dict(snap.meta["shape"], release=2), "release")):
        with pytest.raises(ValueError, match=match):
            other.restore([SessionSnapshot(dict(snap.meta, **{key: bad}), snap.blob)])
    assert other.open_slots == [0, 1, 2]
    pool.drop(a)
    assert pool.sreq[a] == [] and pool.scfg[a] is None
