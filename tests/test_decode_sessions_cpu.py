"""The frontier arithmetic of independent decode sessions (models/stream_schedule.py: DecodeSchedule), without a GPU: random push
patterns against the row rules the C entry checks, against the capacity function, and against the counters StreamingDecoder keeps."""
import random

import pytest

from dmel_codec_amd.models.stream_schedule import (DecodeGeometry, DecodeSchedule, decode_capacity, decode_rebase, decode_session_rows)

H = 4
GEOS = [DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=19),      # the shipped decoder + BigVGAN-base
        DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=0),       # mel only
        DecodeGeometry(factor=2, dilations=(1, 2, 4, 8, 16, 1, 2), voc_halo=7),
        DecodeGeometry(factor=4, dilations=(1, 1, 1), voc_halo=3)]


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
    """(sizes, final with tokens?) -- 0, 1, ragged, at the maximum, shorter than the lookahead"""
    yield [max_push] * 6, True
    yield [max_push] * 6, False
    yield [1] * 40, False
    yield [0, 1, 0, 0, 2, 0], True                     # shorter than the quantiser's lookahead
    yield [3], False                                   # one push, closed without tokens
    yield [0], False                                   # nothing at all
    yield [H + 1, 0, 0, max_push, 1], True
    for _ in range(30):
        k = rng.randint(1, 25)
        yield [rng.choice([0, 1, rng.randint(0, max_push), max_push]) for _ in range(k)], rng.random() < 0.5


class DecoderCounters:
    """StreamingDecoder._push_eager's arithmetic (models/codec_lit_modules.py), replayed without tensors"""

    def __init__(self, f, dils, voc_halo, return_audios):
        self.f, self.dils, self.voc_halo, self.ra = f, dils, voc_halo, return_audios
        self.L = len(dils)
        self.n_tok = self.tok_origin = self.z_valid = self.emitted = 0
        self.prev = [0] * (self.L + 1)

    def push(self, n, final):
        f = self.f
        need_from = max(0, min(self.prev[self.L] - max(self.dils), self.emitted - self.voc_halo))
        self.n_tok += n
        total = self.n_tok * f
        z_new = total if final else max(self.z_valid, (self.n_tok - H) * f)
        win = None
        if z_new > self.z_valid:
            win = (max(0, self.z_valid // f - H), self.n_tok)
            self.z_valid = z_new
            self.tok_origin += max(0, self.z_valid // f - H - self.tok_origin)
        nxt = [self.z_valid]
        for d in self.dils:
            nxt.append(self.z_valid if final else max(self.prev[len(nxt)], nxt[-1] - d))
        stepped = final or nxt[self.L] > self.prev[self.L]
        if stepped:
            self.prev = nxt
        ready = self.prev[self.L]
        e_new = ready if (final or not self.ra) else max(self.emitted, ready - self.voc_halo)
        voc = None
        if self.ra and e_new > self.emitted:
            voc = (max(0, self.emitted - self.voc_halo), min(ready, e_new + self.voc_halo))
        emit = (self.emitted, e_new)
        self.emitted = e_new
        return need_from, win, stepped, emit, voc


@pytest.mark.parametrize("gi", range(len(GEOS)))
@pytest.mark.parametrize("max_push", [1, 16, 64])
def test_schedule_rows_ranges_and_capacity(gi, max_push):
    geo = GEOS[gi]
    rng = random.Random(1000 * gi + max_push)
    cap = decode_capacity(geo, max_push)
    assert cap % 32 == 0 and cap >= geo.hold_frames + 4 * max_push * geo.factor
    for sizes, final_with_tokens in patterns(rng, max_push):
        sch, origin = DecodeSchedule(geo), 0
        steps = [(n, False) for n in sizes]
        if final_with_tokens:
            steps[-1] = (steps[-1][0], True)
        else:
            steps.append((0, True))
        emitted, rebases = 0, 0
        for n, fin in steps:
            n_before = sch.tokens
            st = sch.step(n, fin)
            assert st.tokens == n_before + n and st.upto == st.tokens * geo.factor
            # the oldest column still needed never lies in front of the origin, and what is held fits
            assert st.need_from >= origin
            new = decode_rebase(origin, st, cap)
            rebases += new != origin
            origin = new
            assert origin in (st.need_from, origin) and st.upto - origin <= cap
            assert st.upto - st.need_from <= geo.hold_frames + max_push * geo.factor <= cap
            # the row the pool hands the kernel
            if st.next != st.prev:
                prev, nxt, org = decode_session_rows(2, {1: st}, [0, origin])
                L1 = len(geo.dilations) + 1
                assert prev[:L1] == nxt[:L1] == [0] * L1 and org == [0, origin]          # slot 0 is idle
                row_check(prev[L1:], nxt[L1:], geo.dilations, cap, origin)
                assert st.next[0] == st.z[1] or st.z[1] == st.z[0]
            else:
                assert not fin or st.upto == st.prev[0] == st.prev[-1]      # a final step only stays put when everything is out already
            if fin:
                assert all(v == st.upto for v in st.next)
            # quantiser window: covers the new condition frames with H tokens of context, inside the carried tail
            if st.z[1] > st.z[0]:
                lo, hi = st.tok_window
                assert hi == st.tokens and lo * geo.factor <= st.z[0] and st.z[1] <= hi * geo.factor
                assert lo == max(0, st.z[0] // geo.factor - H) and st.tok_keep_from <= st.z[1] // geo.factor
            else:
                assert st.tok_window == (0, 0)
            # emitted frame ranges are contiguous
            assert st.emit[0] == emitted and st.emit[1] >= emitted
            emitted = st.emit[1]
            if st.voc_window[1] > st.voc_window[0]:
                assert st.voc_window[0] <= st.emit[0] and st.emit[1] <= st.voc_window[1] <= st.next[-1] and st.voc_window[0] >= origin
                assert st.voc_window[0] == max(0, st.emit[0] - geo.voc_halo)
            else:
                assert geo.voc_halo == 0 or st.emit[1] == st.emit[0]
            assert st.emit[0] >= origin
        assert emitted == sch.tokens * geo.factor and sch.finished
        with pytest.raises(RuntimeError):
            sch.step(1)
        # a slot that pushes the maximum every time is re-based once in several pushes, not in every one
        if sizes == [max_push] * 6:
            assert rebases <= 2


@pytest.mark.parametrize("gi", range(len(GEOS)))
def test_schedule_agrees_with_streaming_decoder_counters(gi):
    geo = GEOS[gi]
    rng = random.Random(77 + gi)
    for sizes, final_with_tokens in patterns(rng, 64):
        sch = DecodeSchedule(geo)
        ref = DecoderCounters(geo.factor, list(geo.dilations), geo.voc_halo, geo.voc_halo > 0)
        steps = [(n, False) for n in sizes]
        if final_with_tokens:
            steps[-1] = (steps[-1][0], True)
        else:
            steps.append((0, True))
        for n, fin in steps:
            st = sch.step(n, fin)
            need_from, win, stepped, emit, voc = ref.push(n, fin)
            assert st.need_from == need_from
            assert st.tok_window == (win or (0, 0))
            assert (st.next != st.prev) == (stepped and tuple(ref.prev) != st.prev)
            assert list(st.next) == ref.prev and st.emit == emit and st.voc_window == (voc or (0, 0))
            assert (sch.tokens, sch.z_valid, sch.emitted, sch.tok_origin) == (ref.n_tok, ref.z_valid, ref.emitted, ref.tok_origin)
            assert st.tok_keep_from == ref.tok_origin


def test_refusals_and_prototype():
    geo = GEOS[0]
    with pytest.raises(ValueError):
        decode_capacity(geo, 0)
    sch = DecodeSchedule(geo)
    with pytest.raises(ValueError):
        sch.step(-1)
    st = sch.step(500)                                 # far beyond any max_push the capacity was made for
    with pytest.raises(RuntimeError):
        decode_rebase(0, st, decode_capacity(geo, 16))
    with pytest.raises(ValueError):
        decode_session_rows(2, {0: DecodeSchedule(geo).step(0)}, [0, 0])      # nothing to step
    from dmel_codec_amd import _lib
    assert _lib.PROTOTYPES["dmel_wavenet_stream_step_items_layered"] == _lib.PROTOTYPES["dmel_wavenet_stream_step_items"]
