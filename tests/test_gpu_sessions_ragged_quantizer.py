"""Both session pools make ONE quantiser call per step whatever the sessions pushed: feature windows (encode) and token windows
(decode) of different lengths, final or not, go through quantizer.encode(z, lengths=) / quantizer.decode(ids, lengths=) as one
right-padded batch.  Every session's ids stay the bits of encode() of its clip, its audio and mel the bits of decode() of its ids; a
step whose windows all have one length still makes the plain call.  Codec, clips and feeders are those of the other session tests."""
import pytest
import torch

from test_gpu_decode_sessions import Feeder, clip, step
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

HOP = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def wide_gammas(codec):
    """the constructor's layer scale of 1e-6 hides what the depthwise convolutions read across a window's end: N(0, 0.5)"""
    gen = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for m in codec.quantizer.modules():
            if hasattr(m, "gamma"):
                m.gamma.copy_(torch.randn(m.gamma.shape, generator=gen).to(m.gamma.device) * 0.5)
    codec.quantizer._free_native()
    return codec


@pytest.fixture(scope="module")
def enc_codec(dev):
    return wide_gammas(make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev))


@pytest.fixture(scope="module")
def dec_codec(dev):
    return wide_gammas(make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev))


class CountedQuantizer:
    """codec.quantizer.encode / .decode wrapped: every call's (batch items, columns, lengths) on record"""

    def __init__(self, codec):
        self.q, self.calls = codec.quantizer, []
        self.encode, self.decode = codec.quantizer.encode, codec.quantizer.decode

    def __enter__(self):
        def encode(z, *a, lengths=None, **kw):
            self.calls.append(("encode", z.shape[0] // self.q.groups, z.shape[2], None if lengths is None else list(lengths)))
            return self.encode(z, *a, **kw) if lengths is None else self.encode(z, *a, lengths=lengths, **kw)

        def decode(ids, lengths=None):
            self.calls.append(("decode", ids.shape[0], ids.shape[2], None if lengths is None else [int(n) for n in lengths]))
            return self.decode(ids) if lengths is None else self.decode(ids, lengths=lengths)
        self.q.encode, self.q.decode = encode, decode
        return self

    def __exit__(self, *exc):
        del self.q.encode, self.q.decode                # the instance attributes: the class's methods are back


def check_ragged(calls):
    ragged = [c for c in calls if c[3] is not None]
    assert ragged, "no step had windows of different lengths: the test shows nothing"
    for _, n, cols, lens in ragged:
        assert n == len(lens) >= 2 and max(lens) == cols and min(lens) < cols and min(lens) > 0
    assert all(c[3] is None for c in calls if c[1] == 1)                               # a lone window is the plain call


def test_encode_pool_one_quantizer_call_per_step(dev, enc_codec):
    """five slots; every step gives each named slot another number of samples (0 among them), slots idle, one closes while the others
    push, its slot is reopened"""
    codec = enc_codec
    lengths = [60000, 41000, 30011, 52345, 26000, 33333]
    clips = [(torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.2).to(dev) for n in lengths]
    ref = [codec.encode(c[None], torch.tensor([c.shape[0]], device=dev)) for c in clips]
    #        step: 0     1     2     3     4     5     6     7     8     9     10    11
    plan = {0: [7680, 5000, 7001, 0, 7680, 3000, 6400, 7680, 7680, 7000, 879],
            1: [6000, 7680, 1, 6999, None, 7680, 5120, 7520],
            2: [7680, 7680, 7680, 6971],                                              # closes in step 3, while the others push
            3: [2000, 7680, 7680, 7680, 4000, 7680, 7680, 7680, 265],
            4: [7680, 0, 7680, 7680, 2960],
            5: [None, None, None, None, 7680, 7680, 6000, 7680, 4293]}                 # opened in step 4: takes over clip 2's slot
    for i, sizes in plan.items():
        assert sum(n or 0 for n in sizes) == lengths[i], (i, sum(n or 0 for n in sizes))
    pool = codec.encode_sessions(slots=5, max_push_samples=7680)
    slot, pos, got = {}, [0] * 6, [[] for _ in clips]
    with CountedQuantizer(codec) as cq:
        for t in range(max(len(v) for v in plan.values())):
            for i in plan:
                if i not in slot and (i < 5 and t == 0 or i == 5 and t == 4):
                    slot[i] = pool.open()
            audio, final = {}, []
            for i, sizes in plan.items():
                if t < len(sizes) and sizes[t] is not None:
                    audio[slot[i]] = clips[i][pos[i]:pos[i] + sizes[t]]
                    pos[i] += sizes[t]
                    if pos[i] == lengths[i]:
                        final.append(slot[i])
            if not audio:
                continue
            mark = len(cq.calls)
            out = pool.push(audio, final=final)
            new = cq.calls[mark:]
            assert len(new) <= 1 and all(c[0] == "encode" for c in new), f"step {t} called the quantiser {len(new)} times: {new}"
            for i in plan:
                if i in slot and slot[i] in audio and t < len(plan[i]) and plan[i][t] is not None:
                    got[i].append(out[slot[i]])
        assert slot[5] == slot[2] and pool.open_slots == []
    check_ragged(cq.calls)
    # a step in which a session ended while others went on made one call all the same
    for i, (ids, lens) in enumerate(ref):
        mine = torch.cat(got[i], dim=1)
        assert mine.shape[1] == int(lens[0]) == lengths[i] // HOP // 4, i
        assert torch.equal(mine, ids[0, :, :int(lens[0])]), i


def counted_step(cq, pool, feeders, plan, final=()):
    mark = len(cq.calls)
    step(pool, feeders, plan, final)
    new = cq.calls[mark:]
    assert len(new) <= 1 and all(c[0] == "decode" for c in new), f"a push called the quantiser {len(new)} times: {new}"
    return new


def test_decode_pool_one_quantizer_call_per_step(dev, dec_codec):
    """five slots, six sessions (one slot reused), another push size for every session in every step, 0- and 1-token pushes, a session
    shorter than the lookahead, one that closes while the others push"""
    codec = dec_codec
    with CountedQuantizer(codec) as cq:
        pool = codec.decode_sessions(5, max_push_tokens=64)
        lengths = [170, 3, 101, 77, 90, 45]
        clips = [clip(codec, 180 + i, T, dev) for i, T in enumerate(lengths)]
        f = [Feeder(pool, *clips[i]) for i in range(5)]
        counted_step(cq, pool, f, {0: 41, 1: 2, 2: 33, 3: 7, 4: 64})
        counted_step(cq, pool, f, {0: 1, 1: 1, 2: 50, 3: 0, 4: 13}, final=(1,))        # session 1: 3 tokens, shorter than the lookahead
        f.append(Feeder(pool, *clips[5]))                                              # takes over session 1's slot
        assert f[5].slot == f[1].slot
        counted_step(cq, pool, f, {0: 64, 2: 18, 3: 61, 4: 13, 5: 20}, final=(2, 4))   # two close with tokens while the others push
        counted_step(cq, pool, f, {0: 0, 3: 9, 5: 24})
        counted_step(cq, pool, f, {0: 64, 5: 1}, final=(5,))
        mark = len(cq.calls)
        f[0].got(pool.close(f[0].slot))                                                # closes without tokens
        f[3].got(pool.close(f[3].slot))
        assert len(cq.calls) - mark <= 2 and pool.open_slots == []
    check_ragged(cq.calls)
    for s in f:
        s.check(codec)                                                                 # torch.equal against decode() of the clip


def test_equal_pushes_make_the_plain_calls(dev, enc_codec, dec_codec):
    """sessions in step with each other: every window has one length, so the quantiser is called as it always was -- one plain call,
    even in the step in which they end (finality no longer splits a step)"""
    with CountedQuantizer(enc_codec) as cq:
        pool = enc_codec.encode_sessions(slots=3, max_push_samples=7680)
        clips = [(torch.randn(7680 * 5, generator=torch.Generator().manual_seed(60 + i)) * 0.2).to(dev) for i in range(3)]
        slots = [pool.open() for _ in clips]
        got = [[] for _ in clips]
        for t in range(5):
            mark = len(cq.calls)
            out = pool.push({s: c[t * 7680:(t + 1) * 7680] for s, c in zip(slots, clips)}, final=slots if t == 4 else ())
            assert len(cq.calls) - mark <= 1
            for i, s in enumerate(slots):
                got[i].append(out[s])
    assert cq.calls and all(c == ("encode", 3, c[2], None) for c in cq.calls)
    for i, c in enumerate(clips):
        ids, lens = enc_codec.encode(c[None], torch.tensor([c.shape[0]], device=dev))
        assert torch.equal(torch.cat(got[i], dim=1), ids[0, :, :int(lens[0])])
    with CountedQuantizer(dec_codec) as cq:
        pool = dec_codec.decode_sessions(2, max_push_tokens=64)
        f = [Feeder(pool, *clip(dec_codec, 190, 120, dev)), Feeder(pool, *clip(dec_codec, 191, 120, dev))]
        for n in (64, 40):
            counted_step(cq, pool, f, {0: n, 1: n})
        counted_step(cq, pool, f, {0: 16, 1: 16}, final=(0, 1))
    assert cq.calls and all(c[0] == "decode" and c[1] == 2 and c[3] is None for c in cq.calls)
    for s in f:
        s.check(dec_codec)
