"""The cross-fade of early decode sessions without a GPU: the weights, the host stitcher (utils/crossfade.py), the schedule with
fade_frames=1 and with a look-ahead that changes between pushes (models/stream_schedule.py: EarlyDecodeSchedule), the refusals of
the pool's open() / set_lookahead() and of the C entry dmel_crossfade_items."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_schedule import (DecodeGeometry, DecodeSchedule, EarlyDecodeSchedule, decode_capacity, decode_rebase)
from dmel_codec_amd.utils import crossfade

H = 4
# the geometries and push patterns of test_early_decode_cpu, restated
GEOS = [DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=19),
        DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=0),
        DecodeGeometry(factor=2, dilations=(1, 2, 4, 8, 16, 1, 2), voc_halo=7),
        DecodeGeometry(factor=4, dilations=(1, 1, 1), voc_halo=3)]


def lookaheads(geo):
    hold = geo.hold_frames
    return sorted({0, 1, geo.factor - 1, geo.factor, 8, hold - 1, hold, 10 ** 6})


def patterns(rng, max_push):
    yield [max_push] * 6, True
    yield [max_push] * 6, False
    yield [1] * 40, False
    yield [0, 1, 0, 0, 2, 0], True
    yield [3], False
    yield [0], False
    yield [H + 1, 0, 0, max_push, 1], True
    for _ in range(12):
        k = rng.randint(1, 25)
        yield [rng.choice([0, 1, rng.randint(0, max_push), max_push]) for _ in range(k)], rng.random() < 0.5


def plan(sizes, final_with_tokens):
    steps = [(n, False) for n in sizes]
    if final_with_tokens:
        steps[-1] = (steps[-1][0], True)
    else:
        steps.append((0, True))
    return steps


# ------------------------------------------------------------------------------------------------------------ weights and blend
@pytest.mark.parametrize("F", [1, 2, 3, 256, 512])
def test_weights_are_the_float64_formula_rounded_once(F):
    w = crossfade.weights(F)
    assert w.dtype == torch.float32 and w.shape == (F,)
    want = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / F)).astype(np.float32)
    assert np.array_equal(w.numpy(), want)
    assert bool((w > 0).all()) and bool((w < 1).all())
    assert bool((w[1:] > w[:-1]).all())
    # symmetric: the two halves of the raised cosine add up to one, to the rounding of fp32
    assert float((w + w.flip(0) - 1).abs().max()) <= 2.0 ** -23


def test_weights_refuse_what_is_not_a_fade():
    for bad in (0, -1, 4097, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="crossfade_samples"):
            crossfade.weights(bad)


def test_blend_is_three_rounded_fp32_operations_and_keeps_equal_versions():
    g = torch.Generator().manual_seed(3)
    old, new, w = torch.randn(4096, generator=g), torch.randn(4096, generator=g), crossfade.weights(4096)
    got = crossfade.blend(old, new, w)
    d = (new.numpy() - old.numpy()).astype(np.float32)
    p = (w.numpy() * d).astype(np.float32)
    assert np.array_equal(got.numpy(), (old.numpy() + p).astype(np.float32))
    assert torch.equal(crossfade.blend(old, old.clone(), w), old)


# ------------------------------------------------------------------------------------------------------------ the stitcher
def random_ranges(rng, up, F):
    """raw sample ranges of a session: empty pieces, one-frame pieces, longer ones; the last push final, with or without new frames"""
    frames = [rng.choice([0, 0, 1, 1, rng.randint(2, 9)]) for _ in range(rng.randint(1, 14))]
    if rng.random() < 0.5:
        frames.append(0)                               # a final push with no new frames
    at, out = 0, []
    for n in frames:
        out.append((at, at + n * up))
        at += n * up
    return out, at


@pytest.mark.parametrize("up,F", [(8, 1), (8, 3), (8, 8), (256, 64), (256, 256)])
def test_stitched_pieces_tile_the_total_and_equal_versions_come_back_delayed(up, F):
    rng = random.Random(100 * up + F)
    g = torch.Generator().manual_seed(up + F)
    seen_tail_only = seen_one_frame = 0
    for _ in range(40):
        ranges, total = random_ranges(rng, up, F)
        x = torch.randn(1, total, generator=g)
        # identical versions: every prefix decode is the same signal
        pieces = crossfade.stitch([x] * len(ranges), ranges, F)
        assert sum(p.shape[-1] for p in pieces) == total and all(p.shape[0] == 1 for p in pieces)
        assert torch.equal(torch.cat(pieces, dim=-1), x)
        # the input delayed by F: after push j the session has handed out [0, B_j - F), everything on the final push
        done, started = 0, False
        for j, ((a, b), p) in enumerate(zip(ranges, pieces)):
            started = started or b > a
            done += p.shape[-1]
            last = j == len(ranges) - 1
            assert done == (b if last or not started else b - F)
            if b == a and not last:
                assert p.shape[-1] == 0
            seen_tail_only += last and b == a and p.shape[-1] == F
            seen_one_frame += b - a == up
        # different versions: the samples outside the fade regions are the crops, the regions are the blend
        vers = [torch.randn(1, total, generator=g) for _ in ranges]
        pieces = crossfade.stitch(vers, ranges, F)
        assert sum(p.shape[-1] for p in pieces) == total
        w = crossfade.weights(F)
        tail = None
        for j, ((a, b), p, v) in enumerate(zip(ranges, pieces, vers)):
            last = j == len(ranges) - 1
            if b == a:
                assert p.shape[-1] == (F if last and tail is not None else 0)
                if last and tail is not None:
                    assert torch.equal(p, tail)
                continue
            head = 0
            if tail is not None:
                assert torch.equal(p[:, :F], tail + w * (v[:, a - F:a] - tail))
                head = F
            assert torch.equal(p[:, head:], v[:, a:b if last else b - F])
            tail = None if last else v[:, b - F:b]
    assert seen_tail_only and seen_one_frame
    # F = 0: the raw crops
    ranges, total = random_ranges(rng, up, F)
    x = torch.randn(1, total, generator=g)
    assert all(torch.equal(p, x[:, a:b]) for p, (a, b) in zip(crossfade.stitch([x] * len(ranges), ranges, 0), ranges))


def test_stitcher_refuses_ranges_that_do_not_continue():
    st = crossfade.Stitcher(4)
    x = torch.zeros(1, 64)
    st.push(x, 0, 8)
    with pytest.raises(ValueError):
        st.push(x, 9, 16)
    with pytest.raises(ValueError):
        st.push(x, 8, 10)                              # shorter than the fade
    st.push(x, 8, 64, final=True)
    with pytest.raises(RuntimeError):
        st.push(x, 64, 64)


# ------------------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("gi", range(len(GEOS)))
@pytest.mark.parametrize("max_push", [1, 16, 64])
def test_fade_frames_widens_the_windows_by_one_frame_and_nothing_else(gi, max_push):
    geo = GEOS[gi]
    halo = geo.voc_halo
    cap = decode_capacity(geo, max_push, extra_hold=1)
    assert decode_capacity(geo, max_push) <= cap <= decode_capacity(geo, max_push) + 32
    with pytest.raises(ValueError):
        EarlyDecodeSchedule(geo, 0, fade_frames=2)
    for k in lookaheads(geo):
        rng = random.Random(1000 * gi + max_push)
        shadows = rebases = widened = 0
        for sizes, final_with_tokens in patterns(rng, max_push):
            sch, ref, origin = EarlyDecodeSchedule(geo, k, fade_frames=1), EarlyDecodeSchedule(geo, k), 0
            assert sch.fade_frames == 1 and ref.fade_frames == 0
            for n, fin in plan(sizes, final_with_tokens):
                es, rs = sch.step(n, fin), ref.step(n, fin)
                # the committed schedule, the emit rule, the shadow row and the quantiser window are untouched
                assert es.step == rs.step and es.emit == rs.emit and es.shadow == rs.shadow
                assert (es.prev, es.next, es.tok_window, es.z) == (rs.prev, rs.next, rs.tok_window, rs.z)
                assert (es.fade, rs.fade) == (1, 0)
                # need_from: one frame more, never negative; no re-base drops a column and the enlarged capacity always fits
                assert es.need_from == max(0, rs.need_from - 1) >= origin
                new = decode_rebase(origin, es, cap)
                rebases += new != origin
                origin = new
                assert es.upto - origin <= cap
                # the vocoder window starts one frame earlier, or at 0, and ends where it ended
                lo, hi = es.voc_window
                if rs.voc_window == (0, 0):
                    assert (lo, hi) == (0, 0)
                else:
                    assert hi == rs.voc_window[1] and lo == max(0, es.emit[0] - halo - 1) == max(0, rs.voc_window[0] - 1)
                    assert lo >= es.need_from >= origin
                    assert es.emit[0] == 0 or lo <= es.emit[0] - 1      # the frame in front of the frontier is rendered again
                    widened += lo < rs.voc_window[0]
                if es.shadow:
                    shadows += 1
                    a, b = es.fork
                    assert b == rs.fork[1] and rs.fork[0] - 1 <= a <= rs.fork[0]
                    assert a >= es.need_from >= origin and b - origin < cap
                    assert a <= max(0, es.emit[0] - halo - 1)
                    for l, d in enumerate(geo.dilations):
                        assert a <= max(0, es.prev[l + 1] - d)
                    if halo:                           # a window that starts behind the committed last level reads forked mel
                        assert a <= lo or lo >= es.prev[-1]
                else:
                    assert es.fork == (0, 0)
            assert sch.emitted == sch.tokens * geo.factor and sch.finished
        if k < geo.factor:
            assert shadows
        if halo and max_push > 1:
            assert widened, "no window was widened: the test shows nothing"


SWITCH = [0, 40, 0, 10 ** 6]                           # the look-ahead of the four quarters of a session


@pytest.mark.parametrize("fade", [0, 1])
@pytest.mark.parametrize("gi", range(len(GEOS)))
def test_a_lookahead_that_changes_keeps_the_rule_push_by_push(gi, fade):
    geo = GEOS[gi]
    max_push = 16
    cap = decode_capacity(geo, max_push, extra_hold=fade)
    rng = random.Random(77 + gi)
    paused = forked_after_raise = 0
    for sizes, final_with_tokens in list(patterns(rng, max_push)) + [([3] * 40, False), ([1] * 80, True)]:
        steps = plan(sizes, final_with_tokens)
        sch, exact, origin, emitted = EarlyDecodeSchedule(geo, SWITCH[0], fade_frames=fade), DecodeSchedule(geo), 0, 0
        for j, (n, fin) in enumerate(steps):
            k = SWITCH[min(3, 4 * j // len(steps))]
            sch.set_lookahead(k)
            es, st = sch.step(n, fin), exact.step(n, fin)
            assert es.step == st
            T = st.upto
            want = T if fin else max(emitted, st.emit[1], T - k)
            assert es.emit == (emitted, want) and want >= emitted          # monotone: what has left never comes back
            paused += (not fin) and want == emitted and T - k < emitted and emitted > st.emit[1]
            emitted = want
            if k >= geo.hold_frames:
                assert not es.shadow and es.fork == (0, 0) and es.next == es.prev
                if geo.voc_halo and es.emit[1] > es.emit[0]:
                    assert es.voc_window[1] <= st.next[-1]                  # the committed row holds the window
            assert es.shadow == ((not fin) and want > max(es.emit[0], st.emit[1]))
            if es.voc_window != (0, 0):
                assert es.voc_window[0] == max(0, es.emit[0] - geo.voc_halo - fade) >= es.need_from
            origin = decode_rebase(origin, es, cap)
            assert es.need_from >= origin and T - origin <= cap
        assert emitted == sch.tokens * geo.factor
    assert paused, "raising the look-ahead never paused a session: the test shows nothing"
    for bad in (-1,):
        with pytest.raises(ValueError):
            EarlyDecodeSchedule(geo, 0).set_lookahead(bad)


# ------------------------------------------------------------------------------------------------------------ the pool's refusals
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1,
                       vocoder=dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                    resblock="1", resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
                                    activation="snakebeta", snake_logscale=True))


def test_pool_refusals_and_sizes(codec):
    UP = 8
    plain = codec.decode_sessions(2, max_push_tokens=16, early_emit=True)
    assert plain.up == UP and plain.fade_max == 0 and plain.cap == decode_capacity(plain.geo, 16)
    with pytest.raises(ValueError, match="crossfade_samples"):
        plain.open(lookahead_frames=0, crossfade_samples=4)                # a pool built without the option refuses it at open
    assert plain.open_slots == []
    for opt in (dict(early_emit=False), dict(early_emit=True, return_audios=False)):
        with pytest.raises(ValueError, match="crossfade_samples"):
            codec.decode_sessions(2, crossfade_samples=4, **opt)
    for bad in (UP + 1, -1, True, 2.0, "4"):
        with pytest.raises(ValueError, match="crossfade_samples"):
            codec.decode_sessions(2, early_emit=True, crossfade_samples=bad)
    pool = codec.decode_sessions(2, max_push_tokens=16, early_emit=True, crossfade_samples=4)
    assert pool.fade_max == 4 and pool.cap == decode_capacity(pool.geo, 16, extra_hold=1)
    for bad in (5, UP + 1, True, 2.0, "4", -1, None):
        with pytest.raises(ValueError, match="crossfade_samples"):
            pool.open(lookahead_frames=0, crossfade_samples=bad)
    with pytest.raises(ValueError, match="lookahead_frames"):
        pool.open(crossfade_samples=4)                                      # a cross-fade without a look-ahead
    assert pool.open_slots == []                                            # a refused open takes no slot
    a = pool.open(lookahead_frames=0, crossfade_samples=4)
    b = pool.open()                                                         # an exact session shares the pool
    assert (a, b) == (0, 1) and pool.fade == [4, 0]
    assert pool.sched[a].fade_frames == 1 and isinstance(pool.sched[b], DecodeSchedule)
    # set_lookahead: an early session only, an int >= 0 only, from the next push on
    pool.set_lookahead(a, 40)
    assert pool.sched[a].lookahead == 40
    for bad in (-1, True, 2.5, "3", None):
        with pytest.raises(ValueError, match="lookahead_frames"):
            pool.set_lookahead(a, bad)
    assert pool.sched[a].lookahead == 40
    with pytest.raises(ValueError, match="without lookahead_frames"):
        pool.set_lookahead(b, 0)
    with pytest.raises(ValueError):
        pool.set_lookahead(2, 0)
    pool.sched[a] = None
    with pytest.raises(RuntimeError):
        pool.set_lookahead(a, 0)
    # an early session without a fade in a cross-fading pool keeps the plain schedule
    c = pool.open(lookahead_frames=3)
    assert c == a and pool.fade[c] == 0 and pool.sched[c].fade_frames == 0


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_crossfade_entry_refuses_before_it_launches():
    """dmel_crossfade_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_crossfade_items"][1]) == 8
    fake = 1 << 20

    def call(rows, table=fake, R=None):
        n = len(rows)
        P, I64 = C.c_void_p * n, C.c_int64 * n
        cols = [P(*[r[i] for r in rows]) for i in range(4)]
        rc = lib.dmel_crossfade_items(*cols, I64(*[r[4] for r in rows]), n if R is None else R, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    good = (fake, fake + 4096, fake + 8192, fake + 12288, 64)
    for rows, words in (([good, (fake, fake, fake, fake, 0)], ("row 1", "4096")),
                        ([good, (fake, fake, fake, fake, 4097)], ("row 1", "4096")),
                        ([good, (fake, fake, fake, fake, -3)], ("row 1", "4096")),
                        ([(fake, None, fake, fake, 8), good], ("row 0", "NULL")),
                        ([good, (fake, fake, fake, None, 8)], ("row 1", "NULL")),
                        ([good, good, (None, fake, None, fake, 8)], ("row 2", "neither")),
                        ([good, (fake + 2, fake, fake, fake, 8)], ("row 1", "aligned"))):
        rc, msg = call(rows)
        assert rc == -1 and all(w in msg for w in words), (rows, rc, msg)
    for R in (0, -1, 65536):
        rc, msg = call([good], R=R)
        assert rc == -1 and "65535" in msg, (R, rc, msg)
    assert call([good], table=None)[0] == -1
    assert call([good], table=fake + 4)[0] == -1                           # the table is int64
