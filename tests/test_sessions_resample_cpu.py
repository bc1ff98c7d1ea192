"""Sessions at each sound card's rate, the parts that need no GPU: the bound on what one resampler step can release
(models/stream_schedule.py: resample_max_outputs), the row planner of the items launch (resample_session_rows), the binding of
dmel_resample_window_items_f32, and what the two pools refuse and keep when rates are or are not declared."""
import ctypes as C
import os
import re

import pytest
import torch

from dmel_codec_amd.models.stream_schedule import ResampleSchedule, resample_max_outputs, resample_session_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 24000), (16000, 24000), (44100, 24000), (24000, 48000), (24000, 16000), (24000, 44100)]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_no_step_releases_more_than_the_bound(orig, new):
    """Brute force: a fresh schedule brought to every phase k mod down (and to every k below and around the first group) by one push,
    then one push of n samples, final or not, never releases more than resample_max_outputs(orig, new, n)."""
    ref = ResampleSchedule(orig, new)
    down, width = ref.down, ref.width
    starts = range(0, 2 * down + 2 * width + 1)                    # every residue of k mod down, on both sides of width + down
    worst = {}
    for n in (0, 1, width, down, 255, 300, 777):
        bound = resample_max_outputs(orig, new, n)
        smaller = resample_max_outputs(orig, new, max(n - 1, 0))
        assert smaller <= bound                                    # a bound for "at most n samples"
        for final in (False, True):
            for k in starts:
                sc = ResampleSchedule(orig, new)
                sc.step(k)
                a, b = sc.step(n, final).outputs
                assert b - a <= bound, (orig, new, n, final, k, b - a, bound)
                worst[n] = max(worst.get(n, 0), b - a)
            # and from the very first push
            sc = ResampleSchedule(orig, new)
            a, b = sc.step(n, final).outputs
            assert b - a <= bound
    # the bound is the worst case, not a guess above it: some start reaches it
    for n in (1, 300):
        assert worst[n] == resample_max_outputs(orig, new, n)


def test_rows_follow_the_per_slot_schedules_and_hold_every_tap():
    """Four slots, three live at three rates with their own starts, push sizes and ends; the tables of a step are each slot's own
    ResampleSchedule walk, and every tap of a planned item that lies inside the signal lies inside [s0, s0 + n_valid)."""
    S = 4
    rates = {0: (48000, 24000), 2: (16000, 24000), 3: (44100, 48000)}
    walks = {0: [960, 0, 5, 960, 1, 2000, 960, 13],
             2: [None, 320, 3, 0, 320, None, 777, 1],
             3: [None, None, 441, 100, 0, 2000, None, None]}
    ends = {0: 7, 2: 7, 3: 5}
    pool = {s: ResampleSchedule(*rates[s]) for s in walks}
    alone = {s: ResampleSchedule(*rates[s]) for s in walks}
    s0, fill = [0] * S, [0] * S
    planned = 0
    for i in range(8):
        steps = {}
        for s, w in walks.items():
            if w[i] is not None:
                steps[s] = pool[s].step(w[i], final=(i == ends[s]))
                fill[s] += w[i]
        rs0, nv, o0, n_out, total = resample_session_rows(S, steps, s0, fill)
        assert [len(t) for t in (rs0, nv, o0, n_out, total)] == [S] * 5
        for s in range(S):
            if s not in steps:
                assert (rs0[s], nv[s], o0[s], n_out[s], total[s]) == (0, 0, 0, 0, -1)
                continue
            want = alone[s].step(walks[s][i], final=(i == ends[s]))
            assert want == steps[s]
            a, b = want.outputs
            assert n_out[s] == b - a
            if b > a:
                planned += 1
                sc = alone[s]
                assert (rs0[s], nv[s], o0[s], total[s]) == (s0[s], fill[s], a, want.total_length)
                L = want.total_length if want.final else 1 << 62
                for o in (a, b - 1):                                   # the first and the last output bound every tap in between
                    lo, hi = max(0, sc.first_read(o)), min(L, sc.first_read(o) + sc.kw)
                    assert lo >= hi or (rs0[s] <= lo and hi <= rs0[s] + nv[s]), (s, i, o)
            # carry the tail the way the pool does
            st = steps[s]
            if st.final:
                fill[s] = 0
            elif st.keep_from > s0[s]:
                fill[s] -= st.keep_from - s0[s]
                s0[s] = st.keep_from
            assert 0 <= fill[s] < alone[s].kw or st.final
    assert planned >= 12
    with pytest.raises(ValueError, match="out of range"):
        resample_session_rows(S, {4: ResampleSchedule(48000, 24000).step(100)}, [0] * 5, [100] * 5)
    with pytest.raises(ValueError, match="slot 1"):                    # a row that does not hold what the step reads
        resample_session_rows(S, {1: ResampleSchedule(48000, 24000).step(100)}, [0] * S, [50] * S)


def test_the_items_entry_is_declared_exported_and_bound():
    from dmel_codec_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dmel_hip.h")).read()
    name = "dmel_resample_window_items_f32"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/dmel_hip.h"
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    res, args = _lib.PROTOTYPES[name]
    assert res is C.c_int and len(args) == len(params) == 19
    # the host tables are int64 pointers, as the header has them
    tables = [i for i, p in enumerate(params) if re.search(r"const\s+int64_t\s*\*", p)]
    assert len(tables) == 8 and [args[i] for i in tables] == [_lib.i64p] * 8
    assert callable(getattr(_lib.lib(), name))                        # exported by the built library
    assert _lib.lib().dmel_abi_version() == 2


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1,
                       vocoder=dict(num_mels=80, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
                                    resblock="1", resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
                                    activation="snakebeta", snake_logscale=True))


def test_open_refuses_an_undeclared_rate(codec):
    sr = int(codec.encode_mel_transform.sample_rate)
    enc = codec.encode_sessions(slots=3, max_push_samples=4000, sample_rates=(48000, 16000))
    with pytest.raises(ValueError, match="44100"):
        enc.open(sample_rate=44100)
    assert enc.open_slots == []                                       # the refusal took no slot
    a, b, c = enc.open(sample_rate=48000), enc.open(), enc.open(sample_rate=sr)
    assert (a, b, c) == (0, 1, 2) and enc.rate == [48000, sr, sr]
    with pytest.raises(ValueError, match="exceeds max_push_samples"):  # the bound is in the slot's own samples
        enc.push({a: torch.zeros(4001)})
    with pytest.raises(ValueError, match="reflect pad"):              # 700 samples at 48 kHz are 350 at the codec's rate
        enc.push({a: torch.zeros(700)}, final=(a,))
    with pytest.raises(ValueError):
        codec.encode_sessions(slots=2).open(sample_rate=48000)
    dec = codec.decode_sessions(slots=2, output_sample_rates=(48000,))
    with pytest.raises(ValueError, match="16000"):
        dec.open(output_sample_rate=16000)
    assert dec.open(output_sample_rate=48000) == 0 and dec.open() == 1 and dec.rate[0] == 48000
    with pytest.raises(ValueError):
        codec.decode_sessions(slots=2).open(output_sample_rate=48000)


def test_rates_without_audio_and_pool_wide_rates_are_refused(codec):
    with pytest.raises(ValueError, match="return_audios"):
        codec.decode_sessions(2, return_audios=False, output_sample_rates=(48000,))
    with pytest.raises(NotImplementedError):
        codec.decode_sessions(2, output_sample_rate=48000, output_sample_rates=(48000,))
    with pytest.raises(NotImplementedError, match="codec's own rate"):
        codec.encode_sessions(2, sample_rate=48000, sample_rates=(48000,))


def test_a_pool_without_declared_rates_is_sized_as_before(codec):
    """cap and the sample row width of the parent commit's formulas, and no resampler; declared rates only ever enlarge them, by the
    bound of the schedule."""
    sr = int(codec.encode_mel_transform.sample_rate)
    for push in (2560, 7680):
        plain = codec.encode_sessions(2, max_push_samples=push)
        g = plain.geo
        left, right = g.quant_context
        F = g.factor
        hold = g.encoder_context + right + 1 + F * ((left + F - 1) // F) + F
        want = hold + push // g.hop + 1 + (g.n_fft - g.pad + g.hop - 1) // g.hop
        assert plain.want_max == want and plain.cap == (2 * want + 31) // 32 * 32 and plain.width == g.n_fft + push
        assert plain.rs is None and plain.sample_rates == ()
        same = codec.encode_sessions(2, max_push_samples=push, sample_rates=(sr,))      # the codec's own rate converts nothing
        assert (same.cap, same.width, same.rs) == (plain.cap, plain.width, None)
        down = codec.encode_sessions(2, max_push_samples=push, sample_rates=(48000,))   # 48 -> 24 kHz halves a push
        assert (down.cap, down.width) == (plain.cap, plain.width)
        up = codec.encode_sessions(2, max_push_samples=push, sample_rates=(16000, 48000))
        most = resample_max_outputs(16000, sr, push)
        assert most > push and up.width == g.n_fft + most and up.cap >= plain.cap
        assert up.rs.width == max(ResampleSchedule(16000, sr).kw, ResampleSchedule(48000, sr).kw) - 1 + push
    dec = codec.decode_sessions(2, max_push_tokens=16)
    assert dec.rs is None and dec.output_sample_rates == ()
    from dmel_codec_amd.models.stream_schedule import decode_capacity
    assert dec.cap == decode_capacity(dec.geo, 16)
    assert codec.decode_sessions(2, max_push_tokens=16, output_sample_rates=(48000,)).cap == dec.cap
