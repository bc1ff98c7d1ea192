"""The integer arithmetic of the streamed resampler (models/stream_schedule.py: ResampleSchedule), without a GPU: which outputs are final
after k input samples, what the last step adds, what is carried and how much, held to a brute-force walk over the tap indices."""
import math

import pytest

from dmel_codec_amd.models.stream_schedule import ResampleSchedule, resample_width

PAIRS = [(48000, 24000, 2, 1, 28), (16000, 24000, 2, 3, 16), (44100, 24000, 147, 80, 171), (24000, 48000, 1, 2, 15)]
RAGGED = [0, 7, 1, 300, 0, 4097]


def taps_of(o, down, up, width):
    """input samples output o reads: the whole-clip kernel's own indexing"""
    n = o // up
    return n * down - width, n * down + width + down          # [first, end)


def brute_final(k, down, up, width, limit):
    """outputs o < limit whose every tap is among the first k samples of an unfinished stream; they form a prefix"""
    count = 0
    for o in range(limit):
        if taps_of(o, down, up, width)[1] - 1 < k:
            assert count == o, "final outputs must be a prefix"
            count += 1
    return count


def chunks_of(total, pattern):
    out, left = [], total
    for n in pattern:
        n = min(n, left)
        out.append(n)
        left -= n
    while left:
        n = min(left, pattern[-1])
        out.append(n)
        left -= n
    return out


@pytest.mark.parametrize("orig,new,down,up,kw", PAIRS)
def test_geometry_of_the_rate_pairs(orig, new, down, up, kw):
    s = ResampleSchedule(orig, new)
    assert (s.down, s.up, s.kw) == (down, up, kw)
    assert s.width == resample_width(down, up) and s.kw == 2 * s.width + s.down
    from dmel_codec_amd.utils.resample import sinc_resample_bank            # the bank the kernel reads has this geometry
    kern, width, o, n = sinc_resample_bank(orig, new)
    assert (width, o, n) == (s.width, down, up) and kern.shape == (up, kw)


@pytest.mark.parametrize("orig,new,down,up,kw", PAIRS)
def test_mid_stream_outputs_are_exactly_the_brute_force_final_ones(orig, new, down, up, kw):
    s = ResampleSchedule(orig, new)
    w = s.width
    kmax = 3 * (w + down) + 2 * down
    limit = (kmax // down + 2) * up
    for k in range(kmax + 1):
        want = brute_final(k, down, up, w, limit)
        assert s.outputs_ready(k) == want, k
        assert want % up == 0                                              # whole phase groups
        # the inverse: the smallest k' that makes that many outputs final, and one more output needs more
        assert s.samples_needed(want) <= k
        assert want == 0 or s.outputs_ready(s.samples_needed(want) - 1) < want
        assert s.outputs_ready(s.samples_needed(want + 1)) >= want + 1 and s.samples_needed(want + 1) > k
        # one push of k samples emits exactly those
        one = ResampleSchedule(orig, new)
        assert one.step(k).outputs == (0, want)
    # latency: output m is final at most width + down source samples behind its own position m down / up
    for m in range(limit):
        assert s.samples_needed(m + 1) - m * down / up <= w + down


@pytest.mark.parametrize("orig,new,down,up,kw", PAIRS)
def test_final_step_emits_the_rest_of_the_whole_clip(orig, new, down, up, kw):
    w = ResampleSchedule(orig, new).width
    for L in sorted({1, max(1, down - 1), down, w + down, 1000, 1001}):
        Lout = math.ceil(new * L / orig)
        assert Lout == -(-up * L // down)
        for pattern in ([1], RAGGED, [L]):
            s = ResampleSchedule(orig, new)
            assert s.total_outputs(L) == Lout
            emitted, k, tail_from = 0, 0, 0
            sizes = chunks_of(L, pattern)
            for i, n in enumerate(sizes + [0]):
                final = i == len(sizes)
                st = s.step(n, final)
                k += n
                a, b = st.outputs
                assert a == emitted and st.samples == k
                if final:
                    assert b == Lout and st.total_length == L
                else:
                    assert b == brute_final(k, down, up, w, Lout + up) and st.total_length == -1
                # nothing in front of the carried tail, nothing behind what has arrived
                for o in (a, b - 1) if b > a else ():
                    first, end = taps_of(o, down, up, w)
                    assert max(first, 0) >= tail_from, (L, pattern, i, o)
                    assert final or end <= k
                if b > a:
                    assert st.reads == (max(0, taps_of(a, down, up, w)[0]), min(k, taps_of(b - 1, down, up, w)[1]))
                    assert tail_from <= st.reads[0] <= st.reads[1] <= k
                emitted = b
                assert st.keep_from >= tail_from and st.keep_from <= k
                tail_from = st.keep_from
                assert k - tail_from < s.max_tail or final
            assert emitted == Lout and s.finished
            with pytest.raises(RuntimeError, match="finished"):
                s.step(1)


@pytest.mark.parametrize("orig,new,down,up,kw", PAIRS)
def test_tail_stays_under_its_bound(orig, new, down, up, kw):
    """200 pushes of 0.32 s: the carried tail is shorter than kw = 2 width + down samples (width of left context for the next group, and
    less than width + down of that group's own span still arriving), whatever the stream's length"""
    s = ResampleSchedule(orig, new)
    assert s.max_tail == kw
    n = int(0.32 * orig)
    k = 0
    longest = 0
    for _ in range(200):
        st = s.step(n)
        k += n
        assert st.keep_from == s.tail_start == max(0, (st.outputs[1] // up) * down - s.width)
        longest = max(longest, k - st.keep_from)
        assert 0 <= k - st.keep_from < s.max_tail
    assert longest >= s.width                                 # and it is not trivially empty: the left context is always there


def test_equal_rates_and_bad_arguments():
    s = ResampleSchedule(24000, 24000)
    assert (s.down, s.up) == (1, 1) and s.total_outputs(777) == 777
    with pytest.raises(ValueError):
        ResampleSchedule(0, 24000)
    with pytest.raises(ValueError):
        ResampleSchedule(48000, 24000).step(-1)
