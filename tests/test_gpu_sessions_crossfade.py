"""Early decode sessions that cross-fade their pieces (decode_sessions(early_emit=True, crossfade_samples=Fmax),
open(lookahead_frames=k, crossfade_samples=F)) and whose look-ahead moves (pool.set_lookahead) on the GPU.  Every comparison is
torch.equal.  The reference of a piece is the host stitcher (utils/crossfade.py) applied, on CPU tensors, to decode() of the tokens
received SO FAR; the reference of a session without a fade is the same session in a pool built with crossfade_samples=0."""
import pytest
import torch

from dmel_codec_amd.utils import crossfade
from test_gpu_parity import make_codec
from test_gpu_sessions_ragged_vocoder import CountedVocoder

pytestmark = pytest.mark.gpu

F, UP = 4, 256                                         # mel frames per token, samples per frame (the tiny codec of the early tests)
MAX_PUSH = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


# ---- helpers of test_gpu_sessions_early / test_gpu_decode_sessions, copied -----------------------------------------------------------
def clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * 4, generator=g).to(dev)
    return ids, noise


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


class CountedFades:
    """the cross-fade launches of the library, through its profiler's "crossfade" records; `calls` grows by one per launch"""

    def __enter__(self):
        from dmel_codec_amd import _lib
        self.lib = _lib
        _lib.prof_reset(); _lib.prof_enable(True)
        return self

    @property
    def calls(self):
        torch.cuda.synchronize()
        return [None] * self.lib.prof_read("crossfade")["launches"]

    def __exit__(self, *exc):
        self.lib.prof_enable(False); self.lib.prof_reset()


_prefix = {}                                           # (precision, seed, n) -> (audio (1, n F UP), mel (80, n F)) on the CPU, computed once


def prefix_decode(codec, seed, ids, noise, n):
    """P_n: decode() of the first n tokens with the noise the session has used for them, on the CPU"""
    key = (getattr(codec, "_test_precision", "fp32"), seed, n)
    if key not in _prefix:
        if n == 0:
            _prefix[key] = (torch.zeros(1, 0), torch.zeros(80, 0))
        else:
            out = codec.decode(ids[:, :n][None].contiguous(), torch.tensor([n], device=ids.device), return_audios=True,
                               noise=noise[None, :, :n * F].contiguous())
            _prefix[key] = (out[0][0].cpu(), out[1][0].cpu())
    return _prefix[key]


class Feeder:
    """one session: its clip, its look-ahead k (None: exact), its fade; with check=True every piece is held, as it arrives, to the
    emit rule, to the mel of the prefix decode and to the stitcher over the prefix decodes"""

    def __init__(self, pool, codec, seed, T, k, fade=0, check=True, **open_kw):
        from dmel_codec_amd.models.stream_schedule import DecodeSchedule
        dev = next(codec.parameters()).device
        self.codec, self.pool, self.seed, self.T = codec, pool, seed, T
        self.ids, self.noise = clip(codec, seed, T, dev)
        kw = dict(open_kw)
        if k is not None:
            kw["lookahead_frames"] = k
        if fade:
            kw["crossfade_samples"] = fade
        self.slot = pool.open(**kw)
        self.k, self.fade, self.check = k, fade, check and not open_kw
        self.pos = self.emitted = self.samples = 0
        self.audio, self.mel = [], []
        self.exact = DecodeSchedule(pool.geo)
        self.stitcher = crossfade.Stitcher(fade)

    def set_lookahead(self, k):
        self.pool.set_lookahead(self.slot, k)
        self.k = k

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, F * a:F * self.pos]

    def got(self, out, n, final):
        audio, mel = out
        m, T = mel.shape[1], F * self.pos
        e_exact = self.exact.step(n, final).emit[1]
        want = T if final else max(self.emitted, e_exact, T - (10 ** 9 if self.k is None else self.k))
        assert self.emitted + m == want, f"emitted to {self.emitted + m}, the rule says {want}"
        if self.check:
            p_audio, p_mel = prefix_decode(self.codec, self.seed, self.ids, self.noise, self.pos)
            assert torch.equal(mel.cpu(), p_mel[:, self.emitted:want]), f"mel [{self.emitted}, {want}) of the decode of {self.pos} tokens"
            piece = self.stitcher.push(p_audio, self.emitted * UP, want * UP, final)
            assert audio.shape == piece.shape, f"audio piece {tuple(audio.shape)}, the stitcher says {tuple(piece.shape)}"
            assert torch.equal(audio.cpu(), piece), f"audio of frames [{self.emitted}, {want}) after {self.pos} tokens (final {final})"
            # the audio runs `fade` samples behind the mel while the session lives
            self.samples += audio.shape[1]
            assert self.samples == (want * UP if final or want == 0 else want * UP - self.fade)
        self.emitted = want
        self.audio.append(audio.clone())
        self.mel.append(mel)


def step(pool, feeders, plan, final=(), counters=()):
    """plan: {feeder index: tokens}; final: feeder indices that end with this push -> what each counter saw during the push"""
    ids, noise = {}, {}
    for i, n in plan.items():
        f = feeders[i]
        ids[f.slot], noise[f.slot] = f.take(n)
    marks = [len(c.calls) for c in counters]
    out = pool.push(ids, noise=noise, final=[feeders[i].slot for i in final])
    seen = [len(c.calls) - m for c, m in zip(counters, marks)]
    assert set(out) == set(ids)
    for i, n in plan.items():
        feeders[i].got(out[feeders[i].slot], n, i in final)
    return seen


def run_script(pool, script, sessions, counters=(), only=None):
    """script: push plans ({session: tokens}, final sessions) and "open i"; sessions[i]: the Feeder arguments of session i"""
    f, log = [None] * len(sessions), []
    for item in script:
        if isinstance(item, str):
            i = int(item.split()[1])
            if only is None or i in only:
                f[i] = sessions[i](pool)
            continue
        plan, final = item
        if only is not None:
            plan, final = {i: n for i, n in plan.items() if i in only}, tuple(i for i in final if i in only)
            if not plan:
                continue
        log.append((plan, step(pool, f, plan, final, counters)))
    return f, log


# 3 slots, 4 sessions.  0: k = 0, F = 1, ends without tokens after a push without tokens; 1: 3 tokens, shorter than the quantiser's
# hold, k = 5, F = 64, ends with a token; 2: k = 0, F = up, ends without tokens -- its last piece is the tail alone; 3: k = 5, F = 64,
# takes over session 1's slot, ends without tokens with frames still to come.  0- and 1-token pushes, pushes of max_push_tokens.
LENGTHS, SEEDS, FADES = [40, 3, 30, 22], [240, 241, 242, 243], [(0, 1), (5, 64), (0, UP), (5, 64)]
SCRIPT = ["open 0", ({0: 7}, ()), "open 1", ({0: 1, 1: 2}, ()), "open 2", ({0: 16, 1: 1, 2: 13}, (1,)), "open 3",
          ({0: 0, 2: 1, 3: 16}, ()), ({0: 16, 2: 16, 3: 0}, ()), ({0: 0, 2: 0, 3: 6}, (2,)), ({0: 0, 3: 0}, (0,)), ({3: 0}, (3,))]


def sessions_of(codec, fades=FADES, check=True):
    return [lambda pool, i=i, kf=kf: Feeder(pool, codec, SEEDS[i], LENGTHS[i], kf[0], kf[1], check=check) for i, kf in enumerate(fades)]


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_every_piece_is_the_stitcher_over_the_prefix_decodes(dev, codec, precision):
    codec.set_decode_precision(precision)
    codec._test_precision = precision
    try:
        with CountedVocoder(codec) as cv, CountedQuantiser(codec) as cq, CountedFades() as cf:
            pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=UP)
            assert pool.geo.quant_halo_tokens > LENGTHS[1]
            f, log = run_script(pool, SCRIPT, sessions_of(codec), counters=(cv, cq, cf))
            assert f[3].slot == f[1].slot and pool.open_slots == []
        # ONE vocoder call, ONE quantiser call and at most ONE cross-fade launch per push
        fades = 0
        for plan, (voc, quant, fade) in log:
            assert voc <= 1 and quant <= 1 and fade <= 1, (plan, voc, quant, fade)
            assert fade <= voc, "a cross-fade launch without a vocoder call"
            fades += fade
        assert fades >= 5
        # the pieces tile the clip; every piece was held to the stitcher in got(); session 2's last piece is its tail alone
        for s, T in zip(f, LENGTHS):
            assert sum(m.shape[1] for m in s.mel) == T * F and sum(a.shape[1] for a in s.audio) == T * F * UP
        assert f[2].audio[-1].shape == (1, UP) and f[2].mel[-1].shape[1] == 0
        assert f[0].audio[-1].shape == (1, 1) and f[3].audio[-1].shape == (1, 5 * UP + 64)
        # session 2's 1-token push: the blend of a whole frame in front, the last frame held back
        assert f[2].audio[1].shape == (1, F * UP) and f[2].audio[0].shape == (1, (13 * F - 1) * UP)
    finally:
        codec.set_decode_precision("fp32")
        del codec._test_precision


def test_a_lookahead_that_covers_the_hold_returns_decode_delayed_by_the_fade(dev, codec):
    """k = 10 ** 6, F = 64: the concatenation is decode()'s audio, every piece the exact session's stream shifted by F, no fork"""
    from test_gpu_sessions_pcm import prof_launches
    fade = 64
    pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=fade)
    forks, (f, log) = prof_launches(lambda: run_script(pool, SCRIPT, sessions_of(codec, [(10 ** 6, fade)] * 4, check=False)),
                                    family="stream_fork")
    assert forks == 0
    plain = codec.decode_sessions(3, max_push_tokens=MAX_PUSH)
    g, _ = run_script(plain, SCRIPT, sessions_of(codec, [(None, 0)] * 4, check=False))
    shifted = 0
    for i, (a, b) in enumerate(zip(f, g)):
        whole, w_mel = prefix_decode(codec, SEEDS[i], a.ids, a.noise, LENGTHS[i])
        assert torch.equal(torch.cat(a.audio, dim=1).cpu(), whole) and torch.equal(torch.cat(a.mel, dim=1).cpu(), w_mel)
        assert len(a.mel) == len(b.mel) and all(torch.equal(x, y) for x, y in zip(a.mel, b.mel))
        # the exact session's stream, cut F samples behind the exact session's own boundaries
        stream, done, at = torch.cat(b.audio, dim=1), 0, 0
        for j, (x, y) in enumerate(zip(a.audio, b.audio)):
            done += y.shape[1]
            upto = done if j == len(b.audio) - 1 or done == 0 else done - fade
            assert torch.equal(x, stream[:, at:upto]), f"session {i}, piece {j}"
            shifted += upto != done
            at = upto
    assert shifted >= 3


def test_a_session_that_is_rebased_still_matches(dev, codec):
    """max_push_tokens so small that the slot's columns are shifted while tails and frontiers are live"""
    pool = codec.decode_sessions(2, max_push_tokens=4, early_emit=True, crossfade_samples=64)
    T = pool.cap // F + 10
    f = [Feeder(pool, codec, 250, T, 0, 64), Feeder(pool, codec, 250, T, 5, 0)]     # one clip: the prefix decodes are shared
    sizes = [4] * (T // 4) + ([T % 4] if T % 4 else [])
    origins = []
    for j, n in enumerate(sizes):
        step(pool, f, {0: n, 1: n}, final=(0, 1) if j == len(sizes) - 1 else ())
        origins.append(list(pool.origin))
    assert max(o[f[0].slot] for o in origins) > 0, "the cross-fading session was never re-based: the test shows nothing"
    assert sum(a.shape[1] for a in f[0].audio) == T * F * UP


def test_neighbours_without_a_fade_return_what_a_pool_without_the_option_returns(dev, codec):
    """an exact session and an early session with F = 0 beside a cross-fading one: the pieces of a pool built with crossfade_samples=0"""
    kinds = [(0, UP), (None, 0), (5, 0), (40, 0)]
    both = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=UP)
    f, _ = run_script(both, SCRIPT, sessions_of(codec, kinds, check=False))
    none = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=0)
    assert none.fade_max == 0 and "fade_tail" not in (none.buf or {}) and none.cap <= both.cap
    g, _ = run_script(none, SCRIPT, sessions_of(codec, kinds, check=False), only={1, 2, 3})
    assert "fade_tail" in both.buf and "fade_tail" not in none.buf
    assert both.buf["fade_tail"].shape == both.buf["fade_w"].shape == (3, UP)
    for i in (1, 2, 3):
        assert len(f[i].mel) == len(g[i].mel) > 0
        for x, y in zip(f[i].mel + f[i].audio, g[i].mel + g[i].audio):
            assert x.shape == y.shape and torch.equal(x, y)
    with pytest.raises(ValueError, match="crossfade_samples"):
        none.open(lookahead_frames=0, crossfade_samples=64)
    assert none.open_slots == []


def test_rate_and_format_consume_the_cross_faded_pieces(dev, codec):
    """a cross-fading session at 48 kHz and one as s16: the conversions of the concatenated pieces of the same cross-fading session
    in f32 at the codec's rate -- the resampler sees the concatenation, the convert launch the float piece"""
    from dmel_codec_amd.utils.pcm import to_pcm16
    from dmel_codec_amd.utils.resample import resample
    T, sizes = 34, [7, 1, 0, 16, 10, 0]
    pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, output_sample_rates=(48000,), early_emit=True, crossfade_samples=64)
    a = Feeder(pool, codec, 251, T, 8, 64)
    b = Feeder(pool, codec, 251, T, 8, 64, output_sample_rate=48000)
    c = Feeder(pool, codec, 251, T, 8, 64, sample_format="s16")
    for j, n in enumerate(sizes):
        step(pool, [a, b, c], {0: n, 1: n, 2: n}, final=(0, 1, 2) if j == len(sizes) - 1 else ())
    floats = torch.cat(a.audio, dim=1)
    assert floats.shape == (1, T * F * UP) and all(p.dtype == torch.int16 for p in c.audio) and all(p.dtype == torch.float32 for p in b.audio)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a.mel, b.mel, c.mel))
    assert torch.equal(torch.cat(b.audio, dim=1), resample(floats, 24000, 48000))
    assert torch.equal(torch.cat(c.audio, dim=1), to_pcm16(floats))
    assert [p.shape for p in c.audio] == [p.shape for p in a.audio]       # the s16 pieces are cut where the float pieces are


def test_the_lookahead_moves_on_a_live_session(dev, codec):
    """set_lookahead 0 -> 40 -> 0, with a fade and without: every piece matches the rule (got()); raising k pauses the session"""
    T, sizes = 48, [6, 1, 5, 8, 8, 0, 8, 4, 8]
    pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, early_emit=True, crossfade_samples=64)
    f = [Feeder(pool, codec, 252, T, 0, 64), Feeder(pool, codec, 252, T, 0, 0)]
    frames = []
    for j, n in enumerate(sizes):
        if j == 3:
            for s in f:
                s.set_lookahead(40)
        if j == 6:
            for s in f:
                s.set_lookahead(0)
        step(pool, f, {0: n, 1: n}, final=(0, 1) if j == len(sizes) - 1 else ())
        frames.append(f[0].mel[-1].shape[1])
    assert frames[:3] == [24, 4, 20]                                        # k = 0: every received frame at once
    assert frames[3] == 0 and frames[4] == 28 * F - 40 - 12 * F             # k = 40: paused until the newest frame is 40 ahead
    assert frames[5] == 0
    assert frames[6] > F * sizes[6]                                         # k = 0 again: everything that waited
    assert [m.shape[1] for m in f[1].mel] == frames
    for s in f:
        assert sum(a.shape[1] for a in s.audio) == T * F * UP
    with pytest.raises(RuntimeError):
        pool.set_lookahead(f[0].slot, 0)                                    # the session is over
