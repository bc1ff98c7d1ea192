"""The frontier arithmetic of decode sessions that emit with bounded look-ahead (models/stream_schedule.py: EarlyDecodeSchedule),
without a GPU: random push patterns at every look-ahead against the emit rule, the row rules the C entry checks, the fork window and
the capacity function, and against DecodeSchedule itself where the look-ahead covers the geometry's hold."""
import random

import pytest

from dmel_codec_amd.models.stream_schedule import (DecodeGeometry, DecodeSchedule, EarlyDecodeSchedule, decode_capacity, decode_rebase,
                                                   session_rows)

H = 4
# the four geometries of test_decode_sessions_cpu, restated
GEOS = [DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=19),      # the shipped decoder + BigVGAN-base
        DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=0),       # mel only
        DecodeGeometry(factor=2, dilations=(1, 2, 4, 8, 16, 1, 2), voc_halo=7),
        DecodeGeometry(factor=4, dilations=(1, 1, 1), voc_halo=3)]


def lookaheads(geo):
    hold = geo.hold_frames
    return sorted({0, 1, geo.factor - 1, geo.factor, 8, hold - 1, hold, 10 ** 6})


def row_check(prev, nxt, dils, cap, origin):
    """stream_row_check (csrc/modules.hip), restated: the rules dmel_wavenet_stream_step_items_layered holds every row to"""
    L = len(dils)
    final = nxt[L] == nxt[0]
    for l in range(L + 1):
        assert 0 <= prev[l] <= nxt[l] <= cap, f"level {l}: need 0 <= prev <= next <= cap"
        if l > 0:
            d = dils[l - 1]
            assert nxt[l] == nxt[0] if final else (nxt[l] == prev[l] or nxt[l] + d <= nxt[l - 1]), f"level {l} runs ahead of its input"
            assert prev[l] <= prev[l - 1], f"level {l} is ahead of level {l - 1}"
    if origin > 0:
        for l in range(1, L + 1):
            assert nxt[l] == prev[l] or prev[l] >= dils[l - 1], f"level {l} needs history in front of the buffer"


def patterns(rng, max_push):
    """(sizes, final with tokens?) -- 0, 1, ragged, at the maximum, shorter than the quantiser's hold"""
    yield [max_push] * 6, True
    yield [max_push] * 6, False
    yield [1] * 40, False
    yield [0, 1, 0, 0, 2, 0], True                     # shorter than H
    yield [3], False                                   # one push, closed without tokens
    yield [0], False                                   # nothing at all
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


@pytest.mark.parametrize("gi", range(len(GEOS)))
@pytest.mark.parametrize("max_push", [1, 16, 64])
def test_early_schedule_ranges_rows_fork_and_capacity(gi, max_push):
    geo = GEOS[gi]
    dils, f, L = geo.dilations, geo.factor, len(geo.dilations)
    cap = decode_capacity(geo, max_push)
    for k in lookaheads(geo):
        rng = random.Random(1000 * gi + max_push)
        shadows = rebases = 0
        for sizes, final_with_tokens in patterns(rng, max_push):
            sch, ref, origin, emitted = EarlyDecodeSchedule(geo, k), DecodeSchedule(geo), 0, 0
            for n, fin in plan(sizes, final_with_tokens):
                es = sch.step(n, fin)
                st = ref.step(n, fin)
                assert es.step == st                                   # the committed counters are the exact schedule's
                T = st.upto
                # the emit rule; the ranges tile [0, T_total)
                assert es.emit[0] == emitted
                want = T if fin else max(emitted, st.emit[1], T - k)
                assert es.emit[1] == want
                emitted = want
                if not fin:
                    assert emitted >= T - k
                assert sch.emitted == emitted <= T
                if k >= geo.hold_frames:
                    assert es.emit == st.emit and es.voc_window == st.voc_window and not es.shadow and es.fork == (0, 0)
                # room: the exact schedule's rule, unchanged
                assert es.need_from == st.need_from >= origin
                assert T - st.need_from <= decode_capacity(geo, max_push)
                new = decode_rebase(origin, st, cap)
                rebases += new != origin
                origin = new
                assert T - origin <= cap
                lo, hi = es.voc_window
                if es.shadow:
                    shadows += 1
                    assert not fin and es.emit[1] == T - k > max(es.emit[0], st.emit[1])
                    assert es.prev == st.prev and es.next == (T,) * (L + 1)
                    # the row the pool hands the kernel, beside the committed one
                    prev, nxt, org = session_rows(2, {1: es}, [0, origin])
                    assert org == [0, origin]
                    row_check(prev[L + 1:], nxt[L + 1:], dils, cap, origin)
                    # the fork window: inside the buffer, in front of every column the shadow step and its vocoder window read, and
                    # up to the committed condition frontier, behind which the pool writes the shadow's own columns
                    a, b = es.fork
                    assert 0 <= a - origin <= b - origin < cap
                    assert a >= st.need_from
                    for l, d in enumerate(dils):
                        assert a <= max(0, es.prev[l + 1] - d)
                        assert b >= es.prev[l + 1]
                    assert a <= max(0, es.emit[0] - geo.voc_halo)
                    assert b == sch.exact.z_valid == es.z[0] and es.z[1] == T
                    assert es.tok_window[1] == st.tokens and es.tok_window[0] * f <= min(es.z[0], st.z[0])
                    assert es.tok_window[0] >= sch.exact.tok_origin or st.z[1] > st.z[0]
                    if st.z[1] > st.z[0]:
                        assert es.tok_window == st.tok_window
                    assert (lo, hi) == ((max(0, es.emit[0] - geo.voc_halo), T) if geo.voc_halo else (0, 0))
                else:
                    assert es.next == es.prev and es.fork == (0, 0) and es.z[0] == es.z[1]
                    assert es.tok_window == st.tok_window
                    if geo.voc_halo and es.emit[1] > es.emit[0]:
                        assert lo == max(0, es.emit[0] - geo.voc_halo) >= origin
                        assert es.emit[1] <= hi <= st.next[-1]          # the committed row holds every frame of the window
                        assert hi == min(st.next[-1], es.emit[1] + geo.voc_halo)
                    else:
                        assert (lo, hi) == (0, 0)
                assert es.emit[0] >= origin
            assert emitted == sch.tokens * f and sch.finished
            with pytest.raises(RuntimeError):
                sch.step(1)
        if k < f:
            assert shadows, "no push took the shadow path: the test shows nothing"
        if k >= geo.hold_frames:
            assert shadows == 0


def test_lookahead_zero_emits_every_received_frame():
    for geo in GEOS:
        sch = EarlyDecodeSchedule(geo, 0)
        for n in (1, 0, 3, 64, 1):
            es = sch.step(n)
            assert es.emit[1] == es.upto == sch.tokens * geo.factor
        es = sch.step(0, True)
        assert es.emit == (es.upto, es.upto) and not es.shadow


def test_refusals():
    with pytest.raises(ValueError):
        EarlyDecodeSchedule(GEOS[0], -1)
    sch = EarlyDecodeSchedule(GEOS[0], 5)
    with pytest.raises(ValueError):
        sch.step(-1)


def test_fork_entry_refuses_before_it_launches():
    """dmel_stream_fork_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    import ctypes as C
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_stream_fork_items"][1]) == 17
    fake = 1 << 20

    def call(rows, cond=fake, ccond=3, table=fake, n_items=6):
        I64 = C.c_int64 * len(rows)
        cols = [I64(*[r[i] for r in rows]) for i in range(4)]
        rc = lib.dmel_stream_fork_items(fake, fake, cond, fake, 2, n_items, 5, ccond, 2, 96, len(rows), *cols, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    for rows, words in (([(0, 3, 0, 8), (2, 2, 0, 8)], ("row 1", "itself")),
                        ([(0, 3, 0, 8), (3, 4, 0, 8)], ("row 0", "source")),
                        ([(0, 3, 0, 8), (1, 3, 0, 8)], ("row 1", "destination")),
                        ([(0, 3, 0, 8), (1, 4, 0, 97)], ("row 1", "window")),
                        ([(0, 3, 0, 8), (1, 4, -4, 8)], ("row 1", "window")),
                        ([(0, 3, 0, 8), (1, 4, 8, 4)], ("row 1", "window")),
                        ([(0, 3, 0, 8), (1, 6, 0, 8)], ("row 1", "outside")),
                        ([(-1, 3, 0, 8)], ("row 0", "outside"))):
        rc, msg = call(rows)
        assert rc == -1 and all(w in msg for w in words), (rows, rc, msg)
    assert call([(0, 3, 0, 8)], cond=None)[0] == -1                      # the condition tensor goes with Ccond
    assert call([(0, 3, 0, 8)], table=None)[0] == -1
    assert call([(0, 3, 0, 8)], table=fake + 2)[0] == -1                 # the table is int32
    assert call([(0, 3, 5, 5), (1, 4, 0, 0)])[0] == 0                    # every row idle: nothing is launched
