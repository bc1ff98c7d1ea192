"""DecodeSessions makes ONE vocoder call per step whatever the sessions pushed: mel windows of different lengths go through
BigVGAN.forward(x, lengths) as one right-padded batch.  Every session's audio and mel stay the bits of decode() on its own clip; a step
whose windows all have one length still makes the plain call.  Codec, clips and feeders are those of test_gpu_decode_sessions."""
import pytest
import torch

from test_gpu_decode_sessions import Feeder, clip, step
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


class CountedVocoder:
    """codec.vocoder.forward wrapped: every call's (batch, frames, lengths) on record"""

    def __init__(self, codec):
        self.voc, self.calls = codec.vocoder, []
        self.inner = codec.vocoder.forward

    def __enter__(self):
        def forward(x, lengths=None):
            self.calls.append((x.shape[0], x.shape[2], None if lengths is None else list(lengths)))
            return self.inner(x) if lengths is None else self.inner(x, lengths=lengths)
        self.voc.forward = forward
        return self

    def __exit__(self, *exc):
        del self.voc.forward                           # the instance attribute: the class's forward is back

    def since(self, mark):
        return self.calls[mark:]


def counted_step(cv, pool, feeders, plan, final=()):
    mark = len(cv.calls)
    step(pool, feeders, plan, final)
    new = cv.since(mark)
    assert len(new) <= 1, f"a push called the vocoder {len(new)} times: {new}"
    return new


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_ragged_sessions_one_vocoder_call_per_push(dev, codec, precision):
    """3 slots, 4 sessions (one slot reused), another push size for every session in every step, 0- and 1-token pushes, a session
    shorter than the lookahead, closes with and without tokens"""
    codec.set_decode_precision(precision)
    try:
        with CountedVocoder(codec) as cv:
            pool = codec.decode_sessions(3, max_push_tokens=64)
            lengths = [170, 3, 101, 77]
            clips = [clip(codec, 80 + i, T, dev) for i, T in enumerate(lengths)]
            f = [Feeder(pool, *clips[0])]
            seen = []
            seen += counted_step(cv, pool, f, {0: 41})
            f.append(Feeder(pool, *clips[1]))
            seen += counted_step(cv, pool, f, {0: 1, 1: 2})
            f.append(Feeder(pool, *clips[2]))
            seen += counted_step(cv, pool, f, {0: 64, 1: 1, 2: 33}, final=(1,))      # session 1: 3 tokens, shorter than the lookahead
            f.append(Feeder(pool, *clips[3]))                                         # takes over session 1's slot
            assert f[3].slot == f[1].slot
            seen += counted_step(cv, pool, f, {0: 0, 2: 50, 3: 61})
            seen += counted_step(cv, pool, f, {0: 23, 2: 18, 3: 1}, final=(2,))       # closes with tokens in its final push
            seen += counted_step(cv, pool, f, {0: 41, 3: 15})
            mark = len(cv.calls)
            f[0].got(pool.close(f[0].slot))                                           # closes without
            f[3].got(pool.close(f[3].slot))
            assert len(cv.since(mark)) <= 2
            seen += cv.since(mark)
            assert pool.open_slots == []
        ragged = [c for c in seen if c[2] is not None]
        assert ragged, "no step had windows of different lengths: the test shows nothing"
        for n, frames, lens in ragged:
            assert n == len(lens) >= 2 and max(lens) == frames and min(lens) < frames and min(lens) > 0
        assert all(c[2] is None for c in seen if c[0] == 1)                           # a lone window is the plain call
        for s in f:
            s.check(codec)                                                           # torch.equal against decode() of the clip
    finally:
        codec.set_decode_precision("fp32")


def test_equal_windows_make_the_plain_call(dev, codec):
    """two sessions in step with each other: every window pair has one length, so the vocoder is called as it always was"""
    with CountedVocoder(codec) as cv:
        pool = codec.decode_sessions(2, max_push_tokens=64)
        f = [Feeder(pool, *clip(codec, 90, 120, dev)), Feeder(pool, *clip(codec, 91, 120, dev))]
        for n in (64, 40):
            counted_step(cv, pool, f, {0: n, 1: n})
        counted_step(cv, pool, f, {0: 16, 1: 16}, final=(0, 1))
    assert cv.calls and all(lens is None for _, _, lens in cv.calls) and {n for n, _, _ in cv.calls} == {2}
    for s in f:
        s.check(codec)
