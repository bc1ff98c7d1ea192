"""Decode sessions that emit with bounded look-ahead (decode_sessions(early_emit=True), open(lookahead_frames=k)) on the GPU.  Every
comparison is torch.equal.  The reference of an early piece is decode() of the tokens received SO FAR, cropped to the piece; the
reference of an exact session is the same session in a pool built without early_emit."""
import pytest
import torch

from test_gpu_decode_sessions import clip
from test_gpu_parity import make_codec
from test_gpu_sessions_ragged_vocoder import CountedVocoder

pytestmark = pytest.mark.gpu

F, UP = 4, 256                                         # mel frames per token, samples per frame


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


class CountedQuantiser:
    """codec.get_quantized_features_from_indices wrapped: every call's (batch, tokens, item_features) on record"""

    def __init__(self, codec):
        self.codec, self.calls = codec, []
        self.inner = codec.get_quantized_features_from_indices

    def __enter__(self):
        def call(indices, lengths, **kw):
            self.calls.append((indices.shape[0], indices.shape[-1], bool(kw.get("item_features"))))
            return self.inner(indices, lengths, **kw)
        self.codec.get_quantized_features_from_indices = call
        return self

    def __exit__(self, *exc):
        del self.codec.get_quantized_features_from_indices


def prefix_decode(codec, ids, noise, n, audios=True):
    """P_n: decode() of the first n tokens with the noise the session has used for them -> (audio (1, n F UP) | None, mel (80, n F))"""
    out = codec.decode(ids[:, :n][None].contiguous(), torch.tensor([n], device=ids.device), return_audios=audios,
                       noise=noise[None, :, :n * F].contiguous())
    return (out[0][0], out[1][0]) if audios else (None, out[0])


class Feeder:
    """one session: its clip, its look-ahead (None: exact), the pieces that came back; every piece of an early session is checked
    against the prefix decode as it arrives"""

    def __init__(self, pool, ids, noise, k, audios=True, **open_kw):
        from dmel_codec_amd.models.stream_schedule import DecodeSchedule
        self.slot = pool.open(lookahead_frames=k, **open_kw) if k is not None or open_kw else pool.open()
        self.ids, self.noise, self.k, self.audios = ids, noise, k, audios
        self.pos = self.emitted = 0
        self.audio, self.mel = [], []
        self.exact = DecodeSchedule(pool.geo)          # what today's schedule would have emitted: e_exact of the emit rule
        self.float_audio = not open_kw

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, F * a:F * self.pos]

    def got(self, out, codec, n, final):
        audio, mel = out
        m, T = mel.shape[1], F * self.pos
        e_exact = self.exact.step(n, final).emit[1]
        want = T if final else max(self.emitted, e_exact, T - (10 ** 9 if self.k is None else self.k))
        assert self.emitted + m == want, f"emitted to {self.emitted + m}, the rule says {want}"
        assert mel.shape[0] == 80
        if self.audios and self.float_audio:
            assert audio.shape == (1, m * UP)
        if self.k is not None and m and self.float_audio:
            p_audio, p_mel = prefix_decode(codec, self.ids, self.noise, self.pos, self.audios)
            assert torch.equal(mel, p_mel[:, self.emitted:want]), f"mel [{self.emitted}, {want}) of the decode of {self.pos} tokens"
            if self.audios:
                assert torch.equal(audio, p_audio[:, self.emitted * UP:want * UP]), f"audio of frames [{self.emitted}, {want})"
        self.emitted = want
        self.audio.append(audio.clone() if audio is not None else None)
        self.mel.append(mel)


def step(pool, feeders, plan, codec, final=(), counters=()):
    """plan: {feeder index: tokens}; final: feeder indices that end with this push -> calls each counter saw during the push"""
    ids, noise = {}, {}
    for i, n in plan.items():
        f = feeders[i]
        ids[f.slot], noise[f.slot] = f.take(n)
    marks = [len(c.calls) for c in counters]
    out = pool.push(ids, noise=noise, final=[feeders[i].slot for i in final])
    seen = [c.calls[m:] for c, m in zip(counters, marks)]
    assert set(out) == set(ids)
    for i, n in plan.items():
        feeders[i].got(out[feeders[i].slot], codec, n, i in final)
    return seen


# 3 slots, 4 sessions: 0 emits at once and is long enough to be re-based, 1 is shorter than the quantiser's hold H, 2 is exact, 3 takes
# over session 1's slot.  0- and 1-token pushes, pushes of max_push_tokens, closes with tokens (2) and without (0, 3).
LENGTHS, LOOKAHEADS, MAX_PUSH = [150, 3, 36, 42], [0, 5, None, 40], 16
SCRIPT = [({0: 16}, ()), "open 1", ({0: 1, 1: 2}, ()), "open 2", ({0: 16, 1: 1, 2: 13}, (1,)), "open 3", ({0: 0, 2: 16, 3: 16}, ()),
          ({0: 16, 2: 7, 3: 1}, (2,)), ({0: 16, 3: 9}, ()), ({0: 16, 3: 0}, ()), ({0: 16}, ()), ({0: 16, 3: 16}, ()), ({0: 16}, ()),
          ({0: 16}, ()), ({0: 5}, ()), ({0: 0}, (0,)), ({3: 0}, (3,))]


def run_script(pool, codec, clips, lookaheads, counters=(), only=None):
    f, log, origins = [], [], []
    new = lambda i: Feeder(pool, *clips[i], lookaheads[i])
    f.append(new(0) if only is None or 0 in only else None)
    for item in SCRIPT:
        if isinstance(item, str):
            i = int(item.split()[1])
            f.append(new(i) if only is None or i in only else None)
            continue
        plan, final = item
        if only is not None:
            plan, final = {i: n for i, n in plan.items() if i in only}, tuple(i for i in final if i in only)
            if not plan:
                continue
        log.append((plan, step(pool, f, plan, codec, final, counters)))
        origins.append(list(pool.origin))
    return f, log, origins


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_early_pieces_are_crops_of_the_prefix_decode(dev, codec, precision):
    codec.set_decode_precision(precision)
    try:
        clips = [clip(codec, 140 + i, T, dev) for i, T in enumerate(LENGTHS)]
        with CountedVocoder(codec) as cv, CountedQuantiser(codec) as cq:
            pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True)
            assert pool.geo.quant_halo_tokens > LENGTHS[1]
            f, log, origins = run_script(pool, codec, clips, LOOKAHEADS, counters=(cv, cq))
            assert f[3].slot == f[1].slot and pool.open_slots == []
        # ONE vocoder call and ONE quantiser call per push, early and exact slots mixed
        mixed = 0
        for plan, (voc, quant) in log:
            assert len(voc) <= 1 and len(quant) <= 1, (plan, voc, quant)
            if 2 in plan and len(plan) > 1 and plan[2]:
                assert len(voc) == 1 and len(quant) == 1, (plan, voc, quant)
                mixed += 1
        assert mixed >= 2
        assert max(o[f[0].slot] for o in origins) > 0, "session 0 was never re-based: the test shows nothing about re-bases"
        # pieces tile the clip; the last piece is cut from decode() of the whole sequence (checked in got()); k = 0 emits at once
        for s, T in zip(f, LENGTHS):
            assert sum(m.shape[1] for m in s.mel) == T * F and sum(a.shape[1] for a in s.audio) == T * F * UP
        assert [m.shape[1] for m in f[0].mel] == [F * plan[0] for plan, _ in log if 0 in plan]
        # the exact session: the pieces of the same session in a pool built without early_emit, boundaries and bits
        plain = codec.decode_sessions(3, max_push_tokens=MAX_PUSH)
        g, _, _ = run_script(plain, codec, clips, [None] * 4, only={2})
        ex = [s for s in g if s is not None][0]
        assert len(ex.mel) == len(f[2].mel)
        for a, b in zip(ex.mel + ex.audio, f[2].mel + f[2].audio):
            assert a.shape == b.shape and torch.equal(a, b)
        w_audio, w_mel = prefix_decode(codec, *clips[2], LENGTHS[2])
        assert torch.equal(torch.cat(f[2].mel, dim=1), w_mel) and torch.equal(torch.cat(f[2].audio, dim=1), w_audio)
    finally:
        codec.set_decode_precision("fp32")


def test_a_lookahead_that_covers_the_hold_is_the_exact_session(dev, codec):
    """k = 10 ** 6: the piece boundaries and the bits of an exact session, and not one fork launch"""
    from test_gpu_sessions_pcm import prof_launches
    clips = [clip(codec, 140 + i, T, dev) for i, T in enumerate(LENGTHS)]
    pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True)
    forks, (f, _, _) = prof_launches(lambda: run_script(pool, codec, clips, [10 ** 6] * 4), family="stream_fork")
    assert forks == 0
    plain = codec.decode_sessions(3, max_push_tokens=MAX_PUSH)
    g, _, _ = run_script(plain, codec, clips, [None] * 4)
    for a, b in zip(f, g):
        assert len(a.mel) == len(b.mel)
        for x, y in zip(a.mel + a.audio, b.mel + b.audio):
            assert x.shape == y.shape and torch.equal(x, y)
    # and a look-ahead below it does fork: at most one launch per push
    pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True)
    forks, (_, log, _) = prof_launches(lambda: run_script(pool, codec, clips, LOOKAHEADS), family="stream_fork")
    assert 0 < forks <= len(log)


def test_mel_only_emits_at_once(dev, codec):
    ids, noise = clip(codec, 150, 40, dev)
    pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, return_audios=False, early_emit=True)
    assert pool.geo.voc_halo == 0
    f = [Feeder(pool, ids, noise, 0, audios=False)]
    sizes = [3, 0, 1, 16, 16, 4]
    for j, n in enumerate(sizes):
        step(pool, f, {0: n}, codec, final=(0,) if j == len(sizes) - 1 else ())
    assert all(a is None for a in f[0].audio) and [m.shape[1] for m in f[0].mel] == [F * n for n in sizes]
    # every piece was a crop of the decode of its own prefix (got()); the last one, 4 tokens, is cut from decode() of all 40
    assert torch.equal(f[0].mel[-1], prefix_decode(codec, ids, noise, 40, audios=False)[1][:, -4 * F:])


def test_rate_and_format_consume_the_float_pieces(dev, codec):
    """an early session at 48 kHz / s16: its pieces are the conversion of the concatenated f32 pieces of the same early session at the
    vocoder's rate -- to_pcm16(resample(cat(pieces))), the identity exact sessions are held to"""
    from dmel_codec_amd.utils.pcm import to_pcm16
    from dmel_codec_amd.utils.resample import resample
    ids, noise = clip(codec, 151, 50, dev)
    sizes = [7, 1, 0, 16, 16, 10]
    pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, output_sample_rates=(48000,), early_emit=True)
    a = Feeder(pool, ids, noise, 8)
    b = Feeder(pool, ids, noise, 8, output_sample_rate=48000, sample_format="s16")
    for j, n in enumerate(sizes):
        step(pool, [a, b], {0: n, 1: n}, codec, final=(0, 1) if j == len(sizes) - 1 else ())
    floats = torch.cat(a.audio, dim=1)
    assert floats.shape == (1, 50 * F * UP) and all(p.dtype == torch.int16 for p in b.audio)
    assert all(torch.equal(x, y) for x, y in zip(a.mel, b.mel))
    assert torch.equal(torch.cat(b.audio, dim=1), to_pcm16(resample(floats, 24000, 48000)))


def test_allocation_and_refusals(dev, codec):
    ids, noise = clip(codec, 152, 8, dev)
    plain = codec.decode_sessions(2, max_push_tokens=MAX_PUSH)
    early = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, early_emit=True)
    with pytest.raises(ValueError, match="early_emit"):
        plain.open(lookahead_frames=0)
    assert plain.open_slots == []                                           # a refused open takes no slot
    for bad in (-1, 2.5, "3"):
        with pytest.raises(ValueError, match="lookahead_frames"):
            early.open(lookahead_frames=bad)
    assert early.open_slots == []
    s, t = plain.open(), early.open(lookahead_frames=0)
    plain.push({s: ids}, noise={s: noise})
    early.push({t: ids}, noise={t: noise})
    S, L, C, cap = 2, plain.L, plain.C, plain.cap
    assert plain.buf["hist"].shape == (L + 1, S, C, cap) and "fork_tab" not in plain.buf
    assert early.buf["hist"].shape == (L + 1, 2 * S, C, cap) and early.buf["skip"].shape[0] == early.buf["mel"].shape[0] == 2 * S
    dec = codec.decoder
    words = ((L + 1) * S * C * cap + S * C * cap + S * dec.condition_channels * cap + S * dec.output_channels * cap
             + S * 8 * plain.tok_width + S * C * plain.noise_width + 2 * S * C * cap + 2 * S + S * (2 * (L + 1) + 1))
    assert plain.allocated_bytes() == 4 * words + 8 * 4 * S                 # what a pool allocated before early_emit existed
    assert early.allocated_bytes() > plain.allocated_bytes()
