"""Streaming encode, the parts that need no GPU: the pure frontier / window schedule (models/stream_schedule.py), the new C-ABI symbols'
bindings, and the refusal of CPU tensors."""
import random

import pytest
import torch

from dmel_codec_amd.models.stream_schedule import EncodeGeometry, EncodeSchedule, quantizer_context

HOP, NFFT = 256, 1024
DILS = tuple(2 ** (i % 4) for i in range(20))
GEO = EncodeGeometry(hop=HOP, n_fft=NFFT, dilations=DILS)


def ragged(total, seed):
    rng = random.Random(seed)
    out, left = [100, 7, 5000, 1, 256, 0, 255, 257, 30000], total
    res = []
    for n in out:
        n = min(n, left)
        res.append(n)
        left -= n
    while left:
        n = min(left, rng.choice([1, 3, 255, 256, 1000, 7680, 12345]))
        res.append(n)
        left -= n
    return res


PATTERNS = {
    "one_sample_at_a_time": [1] * 3000,
    "ragged": ragged(24000 * 4 + 77, 0),
    "everything_at_once": [24000 * 3 + 5],
    "short_clip": [400] * 24,
}


def test_quantizer_context_is_derived_from_the_layers():
    # token j <- rate-4 positions j-3 .. j+3 (ConvNeXt k7) <- rate-2 positions 2j-6 .. 2j+7 (k2 s2) <- 2j-9 .. 2j+10 (ConvNeXt k7)
    # <- frames 4j-18 .. 4j+21 (k2 s2)
    assert quantizer_context((2, 2), 7) == (18, 21)
    assert quantizer_context((2,), 7) == (6, 7)
    assert GEO.encoder_context == 75
    assert GEO.pad == 384
    # token 0: frames up to 21 + 75 = 96, whose window ends at sample 96 * 256 - 384 + 1024
    assert GEO.lookahead_samples == 96 * HOP + NFFT - GEO.pad == 25216


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_schedule_emits_every_token_once_and_on_time(name):
    chunks = PATTERNS[name]
    total = sum(chunks)
    sched = EncodeSchedule(GEO)
    steps = [sched.step(n) for n in chunks]
    steps.append(sched.step(0, final=True))
    with pytest.raises(RuntimeError):
        sched.step(0)
    # the union of the emitted ranges is exactly 0 .. L // hop // 4, no gap, no overlap
    pos = 0
    for st in steps:
        assert st.tokens[0] == pos and st.tokens[1] >= pos
        pos = st.tokens[1]
    assert pos == total // HOP // 4
    # frames and level frontiers: contiguous, never ahead of their input, at most `dilation` behind it mid-stream
    f = 0
    lv = (0,) * 21
    for st in steps:
        assert st.frames[0] == f and st.prev == lv
        f, lv = st.frames[1], st.next
        assert st.next[0] == f
        for l, d in enumerate(DILS):
            assert st.prev[l + 1] <= st.next[l + 1] <= st.next[l]
            if not st.final:
                assert st.next[l + 1] == st.prev[l + 1] or st.next[l + 1] + d <= st.next[l]
        if not st.final:
            # a frame computed mid-stream has all its samples (no right reflection)
            assert f == 0 or (f - 1) * HOP - GEO.pad + NFFT <= st.samples
    assert f == total // HOP and set(lv) == {f}
    # no token is final before the sample that completes its right context has arrived (or the stream has ended) ...
    for i, st in enumerate(steps):
        for j in range(*st.tokens):
            assert st.final or st.samples >= GEO.token_ready_samples(j), (i, j)
            # ... and never later than the push that brings that sample (so: no later than one push after it)
            first = next((k for k, s in enumerate(steps) if s.samples >= GEO.token_ready_samples(j)), len(steps) - 1)
            assert i <= first, (i, j, first)
        # the quantiser window starts on a token boundary, covers the left context and ends where the features end
        lo, hi = st.quant_window
        if st.tokens[1] > st.tokens[0]:
            assert lo % 4 == 0 and lo <= max(0, 4 * st.tokens[0] - 18) and hi == st.next[-1]
            assert st.final or 4 * (st.tokens[1] - 1) + 21 < hi


def test_emission_bound_matches_the_documented_lookahead():
    sched = EncodeSchedule(GEO)
    for n in [7680] * 20:
        st = sched.step(n)
        k = st.samples
        promised = max(0, (k - GEO.lookahead_samples) // (4 * HOP) + 1) if k >= GEO.lookahead_samples else 0
        assert st.tokens[1] == promised


def test_new_symbols_are_bound():
    from dmel_codec_amd import _lib
    assert "dmel_stft_window_f32" in _lib.PROTOTYPES
    assert "dmel_wavenet_stream_step_ex" in _lib.PROTOTYPES


def test_streaming_encoder_refuses_cpu_tensors():
    from dmel_codec_amd.configs import build_codec
    codec = build_codec(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, vocoder=None)
    enc = codec.streaming_encoder(batch=1)
    with pytest.raises(RuntimeError, match="GPU"):
        enc.push(torch.zeros(1, 4000))
    with pytest.raises(RuntimeError, match="GPU"):
        next(codec.encode_stream(torch.zeros(1, 4000)))
