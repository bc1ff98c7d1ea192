"""Parking, moving and branching live sessions, the part that needs no GPU: the schedules' state() / from_state(), the live windows,
the refusals of the C entry dmel_stream_pack_items (fake pointers, never read) and the pool-level refusals of snapshot / drop / park
/ restore (models/stream_park.py, models/stream_sessions.py)."""
import copy
import ctypes as C
import io
import random

import pytest
import torch

from dmel_codec_amd.models.stream_park import VERSION, SessionSnapshot, dense_layout
from dmel_codec_amd.models.stream_schedule import (DecodeGeometry, DecodeSchedule, EarlyDecodeSchedule, EncodeGeometry, EncodeSchedule,
                                                   ResampleSchedule, decode_capacity, decode_live_window, decode_rebase,
                                                   encode_live_window)

DEC_GEOS = [DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=19),
            DecodeGeometry(factor=4, dilations=tuple(2 ** (i % 4) for i in range(20)), voc_halo=0),
            DecodeGeometry(factor=2, dilations=(1, 2, 4, 8, 16, 1, 2), voc_halo=7),
            DecodeGeometry(factor=4, dilations=(1, 1, 1), voc_halo=3)]
ENC_GEOS = [EncodeGeometry(hop=256, n_fft=1024, dilations=(1, 2)), EncodeGeometry(hop=256, n_fft=1024, dilations=(1, 2, 4, 8, 1, 2)),
            EncodeGeometry(hop=160, n_fft=400, dilations=(1, 1, 1), downsample_factor=(2,))]


def scripts(rng, top, n=10):
    """random push scripts [(count, final)], the last step final, with or without a payload"""
    yield [(top, False)] * 6 + [(0, True)]
    yield [(0, False), (1, False), (0, False), (top, True)]
    for _ in range(n):
        k = rng.randint(1, 25)
        sizes = [rng.choice([0, 1, rng.randint(0, top), top]) for _ in range(k)]
        yield [(s, False) for s in sizes] + [(rng.choice([0, top // 2]), True)]


def replay_from_every_point(make, rebuild, script):
    """from_state(state()) taken in front of every step returns, for every later step, the step the original returns"""
    ref = make()
    expected = [ref.step(n, fin) for n, fin in script]
    for cut in range(len(script) + 1):
        sc = make()
        for n, fin in script[:cut]:
            sc.step(n, fin)
        state = copy.deepcopy(sc.state())
        buf = io.BytesIO()
        torch.save(state, buf)                                              # plain values: they pass the weights-only loader
        buf.seek(0)
        assert torch.load(buf, weights_only=True) == state
        twin = rebuild(state)
        assert twin.state() == state
        assert [twin.step(n, fin) for n, fin in script[cut:]] == expected[cut:], cut
        assert sc.state() == state                                          # rebuilding shares nothing with the original


# ------------------------------------------------------------------------------------------------------------ the four schedules
@pytest.mark.parametrize("gi", range(len(ENC_GEOS)))
def test_encode_schedule_leaves_and_comes_back(gi):
    geo, rng = ENC_GEOS[gi], random.Random(gi)
    for script in scripts(rng, 5000):
        replay_from_every_point(lambda: EncodeSchedule(geo), lambda st: EncodeSchedule.from_state(geo, st), script)


@pytest.mark.parametrize("gi", range(len(DEC_GEOS)))
def test_decode_schedule_leaves_and_comes_back(gi):
    geo, rng = DEC_GEOS[gi], random.Random(10 + gi)
    for script in scripts(rng, 16):
        replay_from_every_point(lambda: DecodeSchedule(geo), lambda st: DecodeSchedule.from_state(geo, st), script)


@pytest.mark.parametrize("gi", range(len(DEC_GEOS)))
@pytest.mark.parametrize("fade", [0, 1])
def test_early_decode_schedule_leaves_and_comes_back(gi, fade):
    geo, rng = DEC_GEOS[gi], random.Random(20 + gi)
    for k in (0, 3, geo.hold_frames, 10 ** 6):
        for script in scripts(rng, 16, n=4):
            replay_from_every_point(lambda: EarlyDecodeSchedule(geo, k, fade_frames=fade), lambda st: EarlyDecodeSchedule.from_state(geo, st),
                                    script)
    # a look-ahead that moved travels with the state
    sc = EarlyDecodeSchedule(geo, 0, fade_frames=fade)
    sc.step(9)
    sc.set_lookahead(7)
    twin = EarlyDecodeSchedule.from_state(geo, sc.state())
    assert twin.lookahead == 7 and twin.fade_frames == fade
    assert [twin.step(n) for n in (3, 0, 16)] == [sc.step(n) for n in (3, 0, 16)]


@pytest.mark.parametrize("rates", [(48000, 24000), (16000, 24000), (8000, 24000), (44100, 24000), (24000, 24000)])
def test_resample_schedule_leaves_and_comes_back(rates):
    rng = random.Random(rates[0])
    for script in scripts(rng, 3000):
        replay_from_every_point(lambda: ResampleSchedule(*rates), lambda st: ResampleSchedule.from_state(rates, st), script)
    with pytest.raises(ValueError):
        ResampleSchedule.from_state(rates, dict(samples=10 ** 6, emitted=1, finished=False))


def test_a_state_of_the_wrong_depth_is_refused():
    shallow, deep = DEC_GEOS[3], DEC_GEOS[2]
    with pytest.raises(ValueError, match="depth"):
        DecodeSchedule.from_state(deep, DecodeSchedule(shallow).state())
    with pytest.raises(ValueError, match="depth"):
        EarlyDecodeSchedule.from_state(deep, EarlyDecodeSchedule(shallow, 0).state())
    with pytest.raises(ValueError, match="depth"):
        EncodeSchedule.from_state(ENC_GEOS[1], EncodeSchedule(ENC_GEOS[0]).state())
    for sc in (DecodeSchedule(deep), EarlyDecodeSchedule(deep, 3, 1), EncodeSchedule(ENC_GEOS[0]), ResampleSchedule(48000, 24000)):
        sc.step(5)

        def flat(v):
            return all(flat(x) for x in (v.values() if isinstance(v, dict) else v)) if isinstance(v, (dict, list)) else isinstance(v, (int, bool))
        assert flat(sc.state()), sc.state()                                 # ints, bools, lists, dicts of them: nothing of the geometry


# ------------------------------------------------------------------------------------------------------------ the live windows
@pytest.mark.parametrize("gi", range(len(DEC_GEOS)))
@pytest.mark.parametrize("max_push", [1, 16])
def test_decode_window_is_what_a_rebase_keeps_and_stays_in_the_slot(gi, max_push):
    geo, rng = DEC_GEOS[gi], random.Random(30 + gi)
    for fade in (None, 0, 1):
        cap = decode_capacity(geo, max_push, extra_hold=1 if fade else 0)
        for script in scripts(rng, max_push, n=6):
            sc = DecodeSchedule(geo) if fade is None else EarlyDecodeSchedule(geo, rng.choice([0, 5, 10 ** 6]), fade_frames=fade)
            origin = 0
            for n, fin in script:
                lo, hi = decode_live_window(sc)
                assert origin <= lo <= hi <= origin + cap                  # inside the slot's columns
                assert hi - lo <= geo.hold_frames + 1                       # the bound decode_capacity documents (+ 1: a fading session)
                if fade != 1:
                    assert hi - lo <= geo.hold_frames
                st = sc.step(n, fin)
                assert st.need_from == lo                                   # the step's own need_from: what decode_rebase would keep
                origin = decode_rebase(origin, st, cap)
                assert origin <= lo


@pytest.mark.parametrize("gi", range(len(ENC_GEOS)))
def test_encode_window_is_what_a_rebase_keeps(gi):
    geo, rng = ENC_GEOS[gi], random.Random(40 + gi)
    maxdil = max(geo.dilations)
    for script in scripts(rng, 5000):
        sc = EncodeSchedule(geo)
        for n, fin in script:
            lo, hi = encode_live_window(sc)
            frames = sc.frames
            st = sc.step(n, fin)
            assert lo == max(0, min(st.prev[-1] - maxdil, st.quant_window[0]))      # the expression _rebase had inline
            assert hi == max(lo, frames) and hi == max(lo, st.frames[0])


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_pack_entry_refuses_before_it_launches():
    """dmel_stream_pack_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_stream_pack_items"][1]) == 9
    fake = 1 << 20

    def call(items, table=fake, R=None):
        n = len(items)
        P, I64 = C.c_void_p * n, C.c_int64 * n
        cols = list(zip(*items))
        rc = lib.dmel_stream_pack_items(P(*cols[0]), P(*cols[1]), I64(*cols[2]), I64(*cols[3]), I64(*cols[4]), I64(*cols[5]),
                                        n if R is None else R, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    good = (fake, fake + (1 << 16), 5, 33, 96, 33)                         # (src, dst, rows, cols, src pitch, dst pitch)
    for items, words in (([good, (fake, fake, -1, 4, 8, 8)], ("row 1", "negative")),
                         ([good, (fake, fake, 2, -4, 8, 8)], ("row 1", "negative")),
                         ([(None, fake, 1, 4, 4, 4), good], ("row 0", "NULL")),
                         ([good, good, (fake, None, 1, 4, 4, 4)], ("row 2", "NULL")),
                         ([good, (fake + 2, fake, 1, 4, 4, 4)], ("row 1", "aligned")),
                         ([good, (fake, fake + 1, 1, 4, 4, 4)], ("row 1", "aligned")),
                         ([good, (fake, fake, 2, 9, 8, 9)], ("row 1", "pitch")),
                         ([good, (fake, fake, 2, 9, 9, 8)], ("row 1", "pitch")),
                         ([good, (fake, fake, 1 << 20, 4, 1 << 20, 4)], ("row 1", "2^40")),
                         ([good, (fake, fake, 1 << 20, 4, 4, 1 << 20)], ("row 1", "2^40")),
                         # products that do not fit an int64: 2^63 wraps to a negative number, 2^64 to 0
                         ([good, (fake, fake, 1 << 33, 1, 1 << 30, 1)], ("row 1", "2^40")),
                         ([good, (fake, fake, 1 << 33, 1, 1, 1 << 30)], ("row 1", "2^40")),
                         ([good, (fake, fake, 1 << 32, 1, 1 << 32, 1 << 32)], ("row 1", "2^40")),
                         ([good, (fake, fake, (1 << 40) - 1, 1, (1 << 40) - 1, 1)], ("row 1", "2^40")),
                         ([good, (fake, fake, 3, 1, 1 << 62, 1)], ("row 1", "2^40"))):
        rc, msg = call(items)
        assert rc == -1 and all(w in msg for w in words), (items, rc, msg)
    for R in (0, -1, 65536):
        rc, msg = call([good], R=R)
        assert rc == -1 and "65535" in msg, (R, rc, msg)
    assert call([good], table=None)[0] == -1
    assert call([good], table=fake + 4)[0] == -1                           # the table is int64
    # idle descriptors: their pointers and pitches are not looked at, and a call of idle descriptors only launches nothing
    assert call([(None, None, 0, 7, -1, -1), (3, 5, 9, 0, 0, 0)])[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pools
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70,
                       vocoder=dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                    resblock="1", resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
                                    activation="snakebeta", snake_logscale=True))


def through_a_file(snap):
    buf = io.BytesIO()
    torch.save(snap.cpu().as_dict(), buf)
    buf.seek(0)
    return SessionSnapshot.from_dict(torch.load(buf, weights_only=True))


def edited(snap, **changes):
    meta = copy.deepcopy(snap.meta)
    meta.update(changes)
    return SessionSnapshot(meta, snap.blob)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin) == before                         # a refused restore takes no slot


def test_decode_pool_snapshot_drop_restore_bookkeeping(codec):
    voc = codec.decode_sessions(2, max_push_tokens=16).voc_rate
    pool = codec.decode_sessions(3, max_push_tokens=16, early_emit=True, crossfade_samples=4, output_sample_rates=[48000])
    a = pool.open()
    b = pool.open(lookahead_frames=0, crossfade_samples=4, output_sample_rate=48000, sample_format="s16", channels=2)
    snaps = pool.snapshot([a, b])                                           # nothing was pushed: no buffers, nothing to gather
    assert set(snaps) == {a, b} and pool.open_slots == [a, b] and pool.buf is None
    for s, sn in snaps.items():
        assert sn.nbytes == 0 and sn.meta["version"] == VERSION and sn.meta["kind"] == "decode" and sn.meta["layout"] == []
        assert sn.meta["window"] == [0, 0] and sn.meta["G"] == pool.G and sn.meta["C"] == pool.C and sn.meta["L"] == pool.L
        assert sn.meta["geometry"]["dilations"] == list(pool.geo.dilations) and sn.meta["n_mels"] == 80
    mb = snaps[b].meta
    assert (mb["lookahead"], mb["fade"], mb["has_tail"], mb["rate"], mb["sample_format"], mb["channels"]) == (0, 4, False, 48000, "s16", 2)
    assert mb["resampler"]["pair"] == [voc, 48000] and snaps[a].meta["resampler"] is None and mb["tok_origin"] == 0 and mb["n_noise"] == 0
    back = through_a_file(snaps[b])
    assert back.meta == snaps[b].meta and back.blob.dtype == torch.int32 and back.nbytes == 0
    # closed and out-of-range slots: the errors push gives
    for method in (pool.snapshot, pool.park, lambda s: pool.drop(s[0])):
        with pytest.raises(RuntimeError, match="not open"):
            method([2])
        with pytest.raises(ValueError, match="out of range"):
            method([3])
    with pytest.raises(RuntimeError, match="not open"):
        pool.park([a, 2])
    assert pool.open_slots == [a, b]                                        # a refused park drops nothing
    with pytest.raises(ValueError, match="twice"):
        pool.snapshot([a, a])
    # drop frees without a device call; the resampler entry is closed with it
    assert pool.rs.is_open(b)
    pool.drop(b)
    assert pool.open_slots == [a] and not pool.rs.is_open(b) and pool.buf is None
    # restore takes free slots, in order, and continues the counters
    parked = pool.park([a])
    assert pool.open_slots == []
    slots = pool.restore([snaps[b], parked[a]])
    assert slots == [0, 1] and pool.open_slots == [0, 1]
    assert isinstance(pool.sched[0], EarlyDecodeSchedule) and pool.sched[0].fade_frames == 1 and pool.fade[0] == 4
    assert (pool.rate[0], pool.fmt[0], pool.ch[0]) == (48000, "s16", 2) and pool.rs.is_open(0) and pool.rs.pair[0] == (voc, 48000)
    assert isinstance(pool.sched[1], DecodeSchedule) and pool.rate[1] == voc
    # fewer free slots than snapshots: RuntimeError, no slot taken
    with pytest.raises(RuntimeError, match="free"):
        pool.restore({0: snaps[a], 1: snaps[b]})
    assert pool.open_slots == [0, 1]


def test_decode_pool_refuses_what_it_cannot_continue(codec):
    src = codec.decode_sessions(2, max_push_tokens=16, early_emit=True, crossfade_samples=4, output_sample_rates=[48000])
    exact = src.snapshot([src.open()])[0]
    early = src.snapshot([src.open(lookahead_frames=3)])[1]
    src.drop(1)
    fading = src.snapshot([src.open(lookahead_frames=0, crossfade_samples=4)])[1]
    src.drop(1)
    fast = src.snapshot([src.open(output_sample_rate=48000)])[1]
    src.drop(1)
    wired = src.snapshot([src.open(sample_format="s16", channels=2)])[1]

    plain_pool = codec.decode_sessions(2, max_push_tokens=16)
    refused(plain_pool, early, "early_emit")
    refused(plain_pool, fast, "48000")                                      # a rate the pool did not declare
    early_pool = codec.decode_sessions(2, max_push_tokens=16, early_emit=True, crossfade_samples=2)
    refused(early_pool, fading, "crossfade_samples")
    assert early_pool.restore([early]) == [0]
    mel_only = codec.decode_sessions(2, max_push_tokens=16, return_audios=False)
    refused(mel_only, exact)                                                # audio into a pool without: its geometry has no vocoder halo
    refused(mel_only, edited(wired, geometry=mel_only.snapshot([mel_only.open()])[0].meta["geometry"], voc_rate=None, up=1), "return_audios")
    mel_only.drop(0)
    # the other kind, an unknown version, another geometry, width or depth
    enc = codec.encode_sessions(2, max_push_samples=4096)
    enc_snap = enc.snapshot([enc.open()])[0]
    refused(plain_pool, enc_snap, "kind")
    refused(enc, exact, "kind")
    refused(plain_pool, edited(exact, version=VERSION + 1), "version")
    geo = copy.deepcopy(exact.meta["geometry"])
    geo["dilations"] = geo["dilations"] + [1]
    refused(plain_pool, edited(exact, geometry=geo), "geometry")
    for key in ("G", "C", "L", "n_mels", "cond_channels"):
        refused(plain_pool, edited(exact, **{key: exact.meta[key] + 1}), key)
    # a window and one maximal push that do not fit the target's capacity: a session from a pool of a deeper look-back
    sc = DecodeSchedule(plain_pool.geo)
    sc.step(16)
    sc.step(16)
    big = codec.decode_sessions(1, max_push_tokens=4096)
    assert big.cap > 4096 * big.geo.factor
    lo, hi = decode_live_window(sc)
    meta = dict(exact.meta, schedule=sc.state(), window=[lo, hi], tok_origin=sc.tok_origin, n_noise=sc.tokens * sc.geo.factor - sc.z_valid)
    shapes = plain_pool._park_shapes(meta)
    meta["layout"], words = dense_layout(shapes)
    fits = SessionSnapshot(meta, torch.zeros(words, dtype=torch.int32))
    tiny_cap = codec.decode_sessions(1, max_push_tokens=16)
    tiny_cap.cap = hi - lo + 16 * tiny_cap.geo.factor                       # below what decode_capacity gives: the refusal's own arithmetic
    refused(tiny_cap, fits, "capacity")
    refused(plain_pool, fits, "GPU")                                        # it fits; the words of a blob to restore live on the GPU
    # a layout that is not the layout of the state, a window that is not the schedule's
    refused(plain_pool, SessionSnapshot(meta, torch.zeros(words + 1, dtype=torch.int32)), "layout")
    refused(plain_pool, SessionSnapshot(dict(meta, window=[lo, hi + 4]), torch.zeros(words, dtype=torch.int32)), "window")
    with pytest.raises(ValueError, match="SessionSnapshot"):
        plain_pool.restore([meta])
    assert plain_pool.open_slots == []


def test_encode_pool_refuses_what_it_cannot_continue(codec):
    src = codec.encode_sessions(3, max_push_samples=4096, sample_rates=[48000, 8000])
    a = src.open()
    b = src.open(sample_rate=48000, sample_format="s16", channels=2, channel=1)
    c = src.open(sample_rate=8000, sample_format="ulaw")
    snaps = src.park([a, b, c])
    assert src.open_slots == [] and not src.rs.is_open(b)
    mb = snaps[b].meta
    assert (mb["kind"], mb["rate"], mb["sample_format"], mb["channels"], mb["channel"]) == ("encode", 48000, "s16", 2, 1)
    assert mb["resampler"]["pair"] == [48000, src.codec_rate] and mb["s0"] == 0 and mb["tail"] == 0 and mb["window"] == [0, 0]
    assert through_a_file(snaps[c]).meta == snaps[c].meta
    # another order of the declared pairs is fine: the pair travels by value
    other = codec.encode_sessions(2, max_push_samples=1000, sample_rates=[8000, 16000, 48000])
    assert other.cap != src.cap
    assert other.restore([snaps[b], snaps[c]]) == [0, 1]
    assert other.rs.pair[0] == (48000, src.codec_rate) and other.rs.rate[0] == other.rs.pairs.index((48000, src.codec_rate))
    assert (other.fmt[1], other.rate[1], other.pick[0], other.ch[0]) == ("ulaw", 8000, 1, 2)
    with pytest.raises(RuntimeError, match="free"):
        other.restore([snaps[a]])
    assert other.open_slots == [0, 1]
    # a rate the target did not declare; the codec's own rate needs no declaration
    codec_rate_only = codec.encode_sessions(2, max_push_samples=4096)
    refused(codec_rate_only, snaps[b], "48000")
    assert codec_rate_only.restore([snaps[a]]) == [0]
    refused(codec_rate_only, edited(snaps[a], version=0), "version")
    geo = copy.deepcopy(snaps[a].meta["geometry"])
    geo["hop"] += 1
    refused(codec_rate_only, edited(snaps[a], geometry=geo), "geometry")
    for key in ("G", "C", "L", "n_mels"):
        refused(codec_rate_only, edited(snaps[a], **{key: snaps[a].meta[key] + 1}), key)
    refused(codec_rate_only, edited(snaps[a], tail=codec_rate_only.geo.n_fft + 1), "tail")
    for method in (src.snapshot, src.park, lambda s: src.drop(s[0])):
        with pytest.raises(RuntimeError, match="not open"):
            method([0])
        with pytest.raises(ValueError, match="out of range"):
            method([7])


@pytest.mark.parametrize("opts", [dict(max_push_samples=4096), dict(max_push_samples=2048, sample_rates=[48000, 8000]),
                                  dict(max_push_samples=300)])
def test_encode_window_stays_in_the_slot_of_a_pool(codec, opts):
    """EncodeSessions._rebase walked on the host with the pool's own cap: in front of every push the live window lies inside the
    slot's columns [origin, origin + cap), is what the re-base keeps, and is at most the pool's widest window (want_max) wide"""
    from dmel_codec_amd.models.stream_schedule import encode_need_from
    pool = codec.encode_sessions(2, **opts)
    geo, cap, L, top = pool.geo, pool.cap, pool.L, pool.codec_push
    rng = random.Random(top)
    rebased = 0
    for sizes in ([top] * (3 * cap * geo.hop // top + 4), [rng.choice([0, 1, rng.randint(0, top), top]) for _ in range(6 * cap * geo.hop // top)]):
        sc, origin = EncodeSchedule(geo), 0
        for n, fin in [(n, False) for n in sizes] + [(top // 2, True)]:
            lo, hi = encode_live_window(sc)
            assert origin <= lo <= hi <= origin + cap
            assert hi - lo <= pool.want_max
            st = sc.step(n, fin)
            if st.frames[1] - origin > cap:                                 # _rebase: keep [need_from, frames[0]), shift to column 0
                need_from = encode_need_from(geo, st.prev[L], st.tokens[0])
                assert need_from == lo and st.frames[1] - need_from <= cap
                origin, rebased = need_from, rebased + 1
            assert origin <= lo and st.frames[1] - origin <= cap
    assert rebased >= 2
