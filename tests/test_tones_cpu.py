"""The tone rule of decode sessions on the host (utils/tones.py), without a GPU: the tables against float64, programs and their
bounds, the rendering and the splice, the read-back of rendered keys by the project's own detector (utils/dtmf.py: scan with the
default config), the refusals of the C entry dmel_tone_items (fake pointers, never read) and the pool's bookkeeping: send_dtmf /
send_tones, anchors, tones_pending, the keys of a snapshot, drop."""
import copy
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot
from dmel_codec_amd.utils import dtmf, tones

GOOD = (697, 1209, 0.25, 0.5, 100, 20, 10)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("rate", [8000, 24000, 44100])
def test_sine_table_is_float64_rounded_once(rate):
    t = tones.sine_table(rate)
    assert t.dtype == np.float32 and t.shape == (rate,) and not t.flags.writeable
    want = np.array([math.sin(2 * math.pi * j / rate) for j in range(rate)], dtype=np.float64).astype(np.float32)
    assert np.array_equal(bits(t), bits(want)) and t[0] == 0.0


@pytest.mark.parametrize("n", [0, 1, 2, 24, 4096])
def test_ramp_table_is_float64_rounded_once(n):
    t = tones.ramp_table(n)
    want = np.array([0.5 - 0.5 * math.cos(math.pi * (i + 0.5) / n) for i in range(n)], dtype=np.float64).astype(np.float32)
    assert t.dtype == np.float32 and np.array_equal(bits(t), bits(want))
    assert np.all(np.diff(t) >= 0) and np.all((t > 0) & (t < 1))


def test_tables_refuse():
    for rate in (3999, 192001, 24000.0, True, None):
        with pytest.raises(ValueError, match="rate"):
            tones.sine_table(rate)
    for n in (-1, 4097, 2.0, True):
        with pytest.raises(ValueError, match="ramp"):
            tones.ramp_table(n)


# ------------------------------------------------------------------------------------------------------------ programs
def test_dtmf_program_lengths_levels_and_keys():
    p = tones.dtmf_program("1a#", 24000)
    assert len(p) == 3 and tones.length(p) == 3 * (1920 + 1920)
    assert [s[:2] for s in p] == [(697, 1209), (697, 1633), (941, 1477)]
    for s in p:
        assert s[2] == float(np.float32(10 ** (-10 / 20))) and s[3] == float(np.float32(10 ** (-8 / 20))) and s[4:] == (1920, 1920, 24)
    # samples are floor(ms * rate / 1000 + 0.5)
    q = tones.dtmf_program("5", 44100, tone_ms=50, gap_ms=45.5, ramp_ms=0.3)
    assert q[0][4:] == (2205, 2007, 13) and q[0][:2] == (770, 1336)
    assert tones.length(tones.dtmf_program("0123456789*#ABCD1122", 8000, 40, 40)) == 20 * 640
    assert tones.dtmf_program("abcd", 8000) == tones.dtmf_program("ABCD", 8000)
    for bad in ("", "12x", "1 2", None, 12):
        with pytest.raises(ValueError, match="key"):
            tones.dtmf_program(bad, 24000)
    with pytest.raises(ValueError, match="64"):
        tones.dtmf_program("1" * 65, 24000)
    with pytest.raises(ValueError, match="exceed 1"):
        tones.dtmf_program("1", 24000, level_dbfs=-5.0)                      # 0.562 + 0.708
    with pytest.raises(ValueError, match="ramp"):
        tones.dtmf_program("1", 24000, tone_ms=1, ramp_ms=1)                # a ramp above half the tone
    with pytest.raises(ValueError, match="f1"):
        tones.tone_program(2000, 10, 4000)                                  # not below half the rate
    for kw in (dict(tone_ms=-1), dict(gap_ms=math.nan), dict(ramp_ms="1"), dict(level_dbfs=math.inf), dict(twist_db=None), dict(tone_ms=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            tones.dtmf_program("1", 24000, **kw)


def test_tone_program():
    a = float(np.float32(10 ** (-10 / 20)))
    assert tones.tone_program(1000, 200, 24000) == ((1000, 0, a, 0.0, 4800, 0, 24),)
    assert tones.tone_program([350, 440], 1000, 8000, level_dbfs=-13, gap_ms=250, ramp_ms=0) == \
        ((350, 440, float(np.float32(10 ** (-13 / 20))), float(np.float32(10 ** (-13 / 20))), 8000, 2000, 0),)
    for bad in ((), (1, 2, 3), (0,), (-5,), (440.0,), "44"):
        with pytest.raises(ValueError, match="frequenc"):
            tones.tone_program(bad, 100, 24000)
    with pytest.raises(ValueError, match="f1"):
        tones.tone_program(12000, 100, 24000)
    with pytest.raises(ValueError, match="on"):
        tones.tone_program(440, 0, 24000)


def with_(k, v):
    return [GOOD, GOOD[:k] + (v,) + GOOD[k + 1:]]


@pytest.mark.parametrize("program, words", [
    ((), "1 .. 64"), ([GOOD] * 65, "1 .. 64"), (5, "sequence"), ([GOOD[:6]], "segment 0"), ([GOOD + (1,)], "segment 0"),
    (with_(0, -1), "segment 1: f1"), (with_(0, 12000), "segment 1: f1"), (with_(1, 697.0), "segment 1: f2"), (with_(1, True), "segment 1: f2"),
    (with_(2, -0.1), "segment 1: the amplitude of f1"), (with_(2, math.nan), "amplitude of f1"), (with_(3, math.inf), "amplitude of f2"),
    (with_(3, "1"), "amplitude of f2"), (with_(3, 0.76), "exceed 1"), (with_(0, 0), "f1 = 0"), (with_(1, 0), "f2 = 0"),
    (with_(4, 0), "segment 1: on"), (with_(4, 1 << 24), "segment 1: on"), (with_(4, 100.0), "segment 1: on"),
    (with_(5, -1), "segment 1: off"), (with_(5, 1 << 24), "segment 1: off"), (with_(6, -1), "segment 1: ramp"),
    (with_(6, 51), "segment 1: ramp"), ([GOOD[:4] + (10000, 0, 4097)], "segment 0: ramp"), (with_(6, 2.0), "segment 1: ramp")])
def test_check_program_refuses(program, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        tones.check_program(program, 24000)
    with pytest.raises(ValueError):
        tones.render(program, 24000)


def test_check_program_accepts_the_bounds():
    p = tones.check_program([[0, 0, 0, 0.0, 1, 0, 0], (11999, 1, 0.5, 0.5, (1 << 24) - 1, (1 << 24) - 1, 4096), (5, 0, 1.0, 0, 8192, 0, 4096),
                             (np.int64(440), 0, np.float32(0.3), 0.0, 2, 7, 1)], 24000)
    assert p[0] == (0, 0, 0.0, 0.0, 1, 0, 0) and all(type(v) in (int, float) for s in p for v in s)
    assert p[3][2] == float(np.float32(0.3)) and tones.length(p) == 1 + 2 * ((1 << 24) - 1) + 8192 + 9
    with pytest.raises(ValueError, match="f1"):
        tones.check_program(p, 8000)                                        # the same program at a rate that does not carry it


# ------------------------------------------------------------------------------------------------------------ rendering
def reference(seg, rate):
    """the rule, sample by sample in Python: every operation one numpy float32 operation"""
    f1, f2, a1, a2, on, off, ramp = seg
    S, R = tones.sine_table(rate), tones.ramp_table(ramp)
    y = []
    for i in range(on):
        t1 = np.float32(a1) * S[(f1 * i) % rate]
        t2 = np.float32(a2) * S[(f2 * i) % rate]
        x = np.float32(t1 + t2)
        g = R[i] if i < ramp else R[on - 1 - i] if i >= on - ramp else np.float32(1.0)
        y.append(np.float32(x * g))
    return np.array(y + [0.0] * off, dtype=np.float32)


@pytest.mark.parametrize("rate", [8000, 24000, 44100])
def test_render_is_the_rule_and_the_concatenation_of_its_segments(rate):
    p = tones.check_program([(697, 1209, 0.3, 0.4, 300, 7, 24), (941, 0, 0.5, 0.0, 5, 0, 2), (1, 3999, 0.5, 0.5, 64, 3, 0),
                             (350, 440, 0.1, 0.1, 1, 2, 0), (852, 1477, 0.316, 0.398, 2 * 100, 0, 100)], rate)
    y = tones.render(p, rate)
    assert y.dtype == np.float32 and y.shape == (tones.length(p),)
    assert np.array_equal(bits(y), bits(np.concatenate([reference(s, rate) for s in p])))
    assert np.array_equal(bits(y), bits(np.concatenate([tones.render([s], rate) for s in p])))
    at = 0
    for f1, f2, a1, a2, on, off, ramp in p:
        assert np.all(np.abs(y[at:at + on]) <= np.float32(a1) + np.float32(a2))
        assert np.array_equal(bits(y[at + on:at + on + off]), np.zeros(off, np.int32))          # the gap is +0.0
        at += on + off
    # the ramp shapes both ends, the phase starts at 0
    assert y[0] == 0.0 and abs(y[1]) < 0.01


def test_phase_is_exact_where_f_times_i_passes_2_to_the_32():
    seg = (11999, 0, 0.5, 0.0, 400000, 0, 0)                                # 11999 * 399999 = 4.8e9
    y = tones.render([seg], 24000)
    S = tones.sine_table(24000)
    for i in (0, 1, 178957, 357914, 399999):
        assert y[i] == np.float32(np.float32(0.5) * S[(11999 * i) % 24000] + np.float32(0.0))


def test_splice_against_a_hand_built_array():
    rate = 8000
    x = np.arange(1, 11, dtype=np.float32)
    a, b, c = tones.tone_program(440, 1, rate, ramp_ms=0), tones.dtmf_program("5", rate, 1, 0.5, ramp_ms=0), tones.tone_program([350, 440], 0.5, rate, ramp_ms=0)
    ra, rb, rc = (tones.render(p, rate) for p in (a, b, c))
    assert (len(ra), len(rb), len(rc)) == (8, 12, 4)
    got = tones.splice(x, [(0, a), (4, b), (4, c), (10, a)], rate)
    want = np.concatenate([ra, x[:4], rb, rc, x[4:], ra])
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(tones.splice(torch.from_numpy(x), [(4, c), (4, b)], rate), np.concatenate([x[:4], rc, rb, x[4:]]))
    assert np.array_equal(tones.splice(x, [], rate), x) and tones.splice(x, [], rate) is not x
    assert np.array_equal(tones.splice(np.zeros(0, np.float32), [(0, c)], rate), rc)
    with pytest.raises(TypeError):
        tones.splice(x, [(3, a)])                                           # the rate has no default: a wrong one is a wrong pitch
    for bad in ([(-1, a)], [(11, a)], [(5, a), (4, b)], [(2.0, a)], [(True, a)]):
        with pytest.raises(ValueError, match="position"):
            tones.splice(x, bad, rate)
    with pytest.raises(ValueError, match="fp32"):
        tones.splice(x.astype(np.float64), [(0, a)], rate)
    with pytest.raises(ValueError, match="1-D"):
        tones.splice(x[None], [(0, a)], rate)
    with pytest.raises(ValueError, match="segment"):
        tones.splice(x, [(0, [GOOD[:5]])], rate)


# ------------------------------------------------------------------------------------------------------------ read-back
ALL_KEYS = "0123456789*#ABCD1122"


@pytest.mark.parametrize("tone_ms, gap_ms, level_dbfs, twist_db, ramp_ms",
                         [(80, 80, -10, 2, 1), (50, 50, -10, 2, 1), (40, 40, -10, 2, 1), (80, 80, -30, 0, 2), (50, 50, -6.1, 0, 1)])
def test_the_detector_reads_rendered_keys_back(tone_ms, gap_ms, level_dbfs, twist_db, ramp_ms):
    cfg = dtmf.DtmfConfig()
    p = tones.dtmf_program(ALL_KEYS, 24000, tone_ms, gap_ms, level_dbfs, twist_db, ramp_ms)
    x = tones.splice(np.zeros(1000, np.float32), [(1000, p)], 24000)
    assert x.shape[0] == 1000 + tones.length(p) and np.abs(x).max() <= 1.0
    state, _, _ = dtmf.scan(x, cfg, None, 24000)
    assert dtmf.report(state, cfg.block(24000), 24000).digits == ALL_KEYS


def test_keys_between_bursts_of_noise():
    cfg, g = dtmf.DtmfConfig(), np.random.default_rng(7)
    noise = (0.05 * g.standard_normal(10000)).astype(np.float32)
    x = tones.splice(noise, [(5000, tones.dtmf_program("42#", 24000))], 24000)
    assert np.array_equal(x[:5000], noise[:5000]) and np.array_equal(x[-5000:], noise[5000:])
    state, _, _ = dtmf.scan(x, cfg, None, 24000)
    assert dtmf.report(state, cfg.block(24000), 24000).digits == "42#"


# ------------------------------------------------------------------------------------------------------------ the C entry
def header_args(name):
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dmel_hip.h")).read()
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text).group(1)
    return len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(","))


def test_tone_entry_refuses_before_it_launches():
    """dmel_tone_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_tone_items"][1]) == header_args("dmel_tone_items") == 14
    fake = 1 << 20
    seg = (697, 1209, 0.25, 0.5, 100, 20, 10, 0)

    def call(parts, segs=(seg,), R=None, n_segs=None, sine=fake + (1 << 18), rate=8000, ramps=fake + (1 << 19), ramp_floats=64,
             table=fake + (1 << 17), null_segs=False):
        """parts: (dst, src, n, seg_first, seg_count)"""
        n = len(parts)
        cols = list(zip(*parts))
        words = []
        for s in segs:
            a = np.array(s[2:4], dtype=np.float32).view(np.int32)
            words += [s[0], s[1], int(a[0]), int(a[1])] + list(s[4:])
        P = C.c_void_p * n
        rc = lib.dmel_tone_items(P(*cols[0]), P(*cols[1]), (C.c_int64 * n)(*cols[2]), (C.c_int32 * n)(*cols[3]), (C.c_int32 * n)(*cols[4]),
                                 n if R is None else R, None if null_segs else (C.c_int32 * max(len(words), 1))(*words),
                                 len(segs) if n_segs is None else n_segs, sine, rate, ramps, ramp_floats, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    copy_part, tone_part = (fake, fake + 4096, 5, 0, 0), (fake + 64, None, 120, 0, 1)

    def seg_with(k, v):
        return (seg[:k] + (v,) + seg[k + 1:],)

    cases = [(dict(parts=[copy_part, (fake, fake, -1, 0, 0)]), ("part 1", "samples")),
             (dict(parts=[copy_part, (None, fake, 5, 0, 0)]), ("part 1", "NULL destination")),
             (dict(parts=[(fake + 2, fake, 5, 0, 0), copy_part]), ("part 0", "4-byte")),
             (dict(parts=[copy_part, (fake, fake + 1, 5, 0, 0)]), ("part 1", "4-byte")),
             (dict(parts=[copy_part, (fake, None, 120, 1, 1)]), ("part 1", "segments")),
             (dict(parts=[copy_part, (fake, None, 120, -1, 1)]), ("part 1", "segments")),
             (dict(parts=[copy_part, (fake, None, 120, 0, 0)]), ("part 1", "segments")),
             (dict(parts=[copy_part, (fake, None, 120, 0, 2)]), ("part 1", "segments")),
             (dict(parts=[(fake, None, 65 * 120, 0, 65)], segs=(seg,) * 65), ("part 0", "segments")),
             (dict(parts=[copy_part, (fake, None, 119, 0, 1)]), ("part 1", "length mismatch")),
             (dict(parts=[copy_part, (fake, None, 121, 0, 1)]), ("part 1", "length mismatch")),
             (dict(parts=[copy_part, (fake, None, 240, 0, 2)], segs=(seg, seg), n_segs=1), ("part 1", "segments")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(0, -1)), ("part 1", "segment 0", "f1")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(0, 4000)), ("part 1", "segment 0", "f1")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(1, 4000)), ("part 1", "f2")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(0, 0)), ("part 1", "a1")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(2, -0.5)), ("part 1", "a1")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(2, math.nan)), ("part 1", "a1")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(3, math.inf)), ("part 1", "a2")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(3, 0.76)), ("part 1", "exceed 1")),
             (dict(parts=[copy_part, (fake, None, 20, 0, 1)], segs=seg_with(4, 0)), ("part 1", "on =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(4, 1 << 24)), ("part 1", "on =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(5, -1)), ("part 1", "off =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(5, 1 << 24)), ("part 1", "off =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(6, -1)), ("part 1", "ramp =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(6, 51)), ("part 1", "ramp =")),
             (dict(parts=[(fake, None, 10000, 0, 1)], segs=((697, 1209, 0.25, 0.5, 10000, 0, 4097, 0),), ramp_floats=8192), ("part 0", "ramp =")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(7, 55)), ("part 1", "arena")),
             (dict(parts=[copy_part, tone_part], segs=seg_with(7, -1)), ("part 1", "arena")),
             (dict(parts=[copy_part, tone_part], ramp_floats=9), ("part 1", "arena")),
             # one prefix sum per segment of the table: a segment two parts would begin at different samples is refused
             (dict(parts=[(fake, None, 240, 0, 2), (fake + 4096, None, 120, 1, 1)], segs=(seg, seg)), ("part 1", "segment 1", "share")),
             (dict(parts=[(fake, None, 120, 1, 1), copy_part, (fake + 4096, None, 240, 0, 2)], segs=(seg, seg)), ("part 2", "segment 1", "share")),
             (dict(parts=[(fake, None, 240, 0, 2), (fake + 4096, None, 240, 1, 2)], segs=(seg, seg, seg)), ("part 1", "segment 1", "share"))]
    for kw, words in cases:
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for R in (0, -1, 65536):
        rc, msg = call([copy_part], R=R)
        assert rc == -1 and "65535" in msg, (R, rc, msg)
    for rate in (3999, 192001):
        rc, msg = call([copy_part], rate=rate)
        assert rc == -1 and "rate" in msg, (rate, rc, msg)
    for kw in (dict(sine=None), dict(table=None), dict(sine=fake + 2), dict(ramps=fake + 1), dict(table=fake + 4), dict(ramps=None),
               dict(ramp_floats=-1), dict(null_segs=True), dict(n_segs=-1), dict(n_segs=64 * 65535 + 1)):
        assert call([copy_part, tone_part], **kw)[0] == -1, kw
    # idle parts: nothing of them is looked at, and a call of idle parts only launches nothing
    assert call([(None, None, 0, -3, 99), (fake + 1, fake + 3, 0, 0, 0)], segs=(), null_segs=True, ramps=None, ramp_floats=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
UP, FACTOR = 8, 4


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1,
                       vocoder=dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                    resblock="1", resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
                                    activation="snakebeta", snake_logscale=True))


def test_pool_options(codec):
    plain = codec.decode_sessions(2, max_push_tokens=16)
    pool = codec.decode_sessions(2, max_push_tokens=16, tones=True)
    assert not plain.tones_on and pool.tones_on and pool.up == UP and pool.cap == plain.cap
    assert pool.max_tone == 2 * pool.voc_rate == 48000 and plain.max_tone == 0
    assert codec.decode_sessions(2, tones=True, max_tone_samples=100).max_tone == 100
    for bad in (0, -1, 2.0, True, "9"):
        with pytest.raises(ValueError, match="max_tone_samples"):
            codec.decode_sessions(2, tones=True, max_tone_samples=bad)
    with pytest.raises(ValueError, match="tones=True"):
        codec.decode_sessions(2, max_tone_samples=100)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="tones"):
            codec.decode_sessions(2, tones=bad)
    with pytest.raises(ValueError, match="return_audios"):
        codec.decode_sessions(2, tones=True, return_audios=False)
    # the resampler's rows take a step's speech and the tones that waited
    a = codec.decode_sessions(2, max_push_tokens=16, output_sample_rates=(8000,))
    b = codec.decode_sessions(2, max_push_tokens=16, output_sample_rates=(8000,), tones=True, max_tone_samples=1000)
    assert a.rs.max_push == a.cap * UP and b.rs.max_push == b.cap * UP + 1000
    s = plain.open()
    for send in (lambda: plain.send_dtmf(s, "1"), lambda: plain.send_tones(s, tones.tone_program(440, 10, 24000))):
        with pytest.raises(ValueError, match="tones=True"):
            send()
    assert "tones" not in plain.snapshot([s])[s].meta and "handed" not in plain.snapshot([s])[s].meta


def test_pool_bookkeeping_of_tone_requests(codec):
    pool = codec.decode_sessions(3, max_push_tokens=16, output_sample_rates=(8000,), early_emit=True, tones=True, max_tone_samples=20000)
    a, b = pool.open(), pool.open(output_sample_rate=8000, sample_format="ulaw")
    assert pool.tones_pending(a) == [] and pool.buf is None
    n = pool.send_dtmf(a, "12")
    assert n == 2 * 3840 and pool.tones_pending(a) == [(0, 7680)] and pool.tone_samples[a] == 7680
    assert pool.tq[a] == [(0, tones.dtmf_program("12", 24000))]
    beep = tones.tone_program(1000, 100, 24000, ramp_ms=5)
    assert pool.send_tones(a, beep) == 2400 and pool.send_tones(a, [list(s) for s in beep], at_frame=0) == 2400
    assert pool.tones_pending(a) == [(0, 7680), (0, 2400), (0, 2400)] and pool.tone_samples[a] == 12480
    assert pool.buf is None and set(pool._ramp_off) == {24, 120}            # no device call: the tables wait for the arena
    # anchors: nothing was received, so 0 is the only frame
    for bad in (1, -1, 0.0, True):
        with pytest.raises(ValueError, match="at_frame"):
            pool.send_tones(a, beep, at_frame=bad)
    # the schedule's counters say what was received and what left
    pool.sched[a].tokens, pool.sched[a].emitted = 10, 12
    assert pool.send_tones(a, beep, at_frame=12) == 2400 and pool.send_tones(a, beep) == 2400
    assert pool.tones_pending(a)[-2:] == [(12, 2400), (FACTOR * 10, 2400)] and pool.tq[a][-1][0] == FACTOR * 10 * UP
    for bad in (11, 41, 39):                                                # before what left, behind what came, before a pending anchor
        with pytest.raises(ValueError, match="at_frame"):
            pool.send_tones(a, beep, at_frame=bad)
    pool.sched[a].tokens = pool.sched[a].emitted = 0
    # refusals: nothing is queued
    before = copy.deepcopy(pool.tq)
    with pytest.raises(ValueError, match="max_tone_samples"):
        pool.send_tones(a, tones.tone_program(440, 120, 24000))             # 17280 pending + 2880 > 20000
    with pytest.raises(ValueError, match="half of the session's output rate"):
        pool.send_tones(b, tones.tone_program(4000, 10, 24000))             # the session leaves at 8 kHz
    with pytest.raises(ValueError, match="f1"):
        pool.send_tones(a, tones.tone_program(3000, 10, 8000) + ((12000, 0, 0.1, 0.0, 10, 0, 0),))
    with pytest.raises(ValueError, match="key"):
        pool.send_dtmf(a, "1x")
    with pytest.raises(ValueError, match="segments"):
        for _ in range(70):
            pool.send_tones(b, [(440, 0, 0.1, 0.0, 1, 0, 0)])
    assert len(pool.tq[b]) == 64 and pool.tq[a] == before[a]
    with pytest.raises(RuntimeError):
        pool.send_dtmf(2, "1")                                              # not open
    # the snapshot: plain values in, the same requests out
    snap = pool.snapshot([a])[a]
    assert snap.meta["tones"] == [[P, [list(s) for s in p]] for P, p in pool.tq[a]] and snap.meta["handed"] == 0
    assert snap.meta["tone_samples"] == 17280 and snap.nbytes == 0
    other = codec.decode_sessions(4, max_push_tokens=8, early_emit=True, tones=True)
    assert other.open() == 0 and other.open() == 1                         # the session leaves slot 0 and lands in slot 2 of a pool of 4
    assert other.restore([snap]) == [2] and other.tq[2] == pool.tq[a] and other.tone_samples[2] == 17280 and other.handed[2] == 0
    assert other.tq[:2] == [[], []] and other.tq[3] == [] and other.tone_samples == [0, 0, 17280, 0]
    assert set(other._ramp_off) == {24, 120} and other.tones_pending(2) == pool.tones_pending(a)
    other.drop(0)
    # a pool without the option refuses pending requests, takes a snapshot without them (and one written before the keys existed)
    plain = codec.decode_sessions(2, max_push_tokens=16, early_emit=True)
    with pytest.raises(ValueError, match="tones=True"):
        plain.restore([snap])
    assert plain.open_slots == []
    empty = dict(snap.meta, tones=[], tone_samples=0)
    assert plain.restore([SessionSnapshot(empty, snap.blob)]) == [0]
    old = {k: v for k, v in snap.meta.items() if k not in ("tones", "handed", "tone_samples")}
    assert plain.restore([SessionSnapshot(old, snap.blob)]) == [1] and other.restore([SessionSnapshot(old, snap.blob)]) == [0]
    assert other.tq[0] == [] and other.handed[0] == 0 and other.tone_samples[0] == 0
    # a tone pool refuses more pending samples than it holds, and requests that are none
    small = codec.decode_sessions(2, max_push_tokens=16, early_emit=True, tones=True, max_tone_samples=17279)
    with pytest.raises(ValueError, match="max_tone_samples"):
        small.restore([snap])
    bad = copy.deepcopy(snap.meta)
    bad["tones"][0][1][0][4] = 0
    with pytest.raises(ValueError, match="on"):
        other.restore([SessionSnapshot(bad, snap.blob)])
    bad = copy.deepcopy(snap.meta)
    bad["tones"][1][0] = -8
    with pytest.raises(ValueError, match="anchors"):
        other.restore([SessionSnapshot(bad, snap.blob)])
    assert small.open_slots == [] and other.open_slots == [0, 1, 2]
    # drop discards the queue; a reopened slot starts without one
    pool.drop(a)
    assert pool.tq[a] == [] and pool.tone_samples[a] == 0
    assert pool.open() == a and pool.tones_pending(a) == []
