"""Sessions that speak 16-bit PCM on the GPU.  Every comparison is torch.equal, and every reference is a path that existed before the
format became a property of a session: encode() / decode() / resample() on one finished clip, with the conversion done outside --
from_pcm16 in front (exact), the CPU rounding oracle of test_gpu_pcm_convert.py behind."""
import pytest
import torch

from test_gpu_pcm_convert import oracle_to_s16

pytestmark = pytest.mark.gpu

SR = 24000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def randomise(module, seed, scale=1.0):
    """O(1) weights so every term of the arithmetic matters (default inits are ~0.02 / 1e-6)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf in ("alpha", "beta"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif leaf == "gamma":
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif leaf == "weight_g":
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (scale / p[0].numel() ** 0.5))
            elif leaf == "weight":
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)


def make_codec(seed, **kw):
    from dmel_codec_amd.configs import build_codec
    torch.manual_seed(seed)
    codec = build_codec(**kw)
    randomise(codec.encoder, seed + 1)
    randomise(codec.quantizer, seed + 2, scale=1.5)
    randomise(codec.decoder, seed + 3)
    if codec.vocoder is not None:
        randomise(codec.vocoder, seed + 4, scale=0.7)
    with torch.no_grad():
        codec.quality_projection.weight.normal_(0, 0.3)
        codec.quality_projection.bias.normal_(0, 0.1)
    return codec


def prof_launches(fn, family="pcm_convert"):
    from dmel_codec_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        n = _lib.prof_read(family)["launches"]
    finally:
        _lib.prof_enable(False); _lib.prof_reset()
    return n, out


# ------------------------------------------------------------------------------------ encode sessions
# clip -> (format, rate, seconds, step of its open(), push sizes in its own samples, steps in which it is not named)
ENC = {"a": ("s16", SR, 1.2, 0, [7680, 0, 5000, 1, 7680], {2}),
       "b": ("f32", 48000, 1.0, 0, [15360, 9, 0, 11111], set()),
       "c": ("s16", 16000, 1.1, 1, [5120, 3, 0, 4097], {4, 5}),              # stalls for two steps
       "d": ("f32", 16000, 0.6, 9, [5120, 100], set()),                      # takes over a's slot: s16 at the codec's rate -> f32 at 16 kHz
       "e": ("s16", 48000, 0.6, 9, [15360, 7], set())}                       # takes over b's slot: f32 -> s16, same rate
_enc = {}


def _plan(total, start, sizes, idle):
    out, pos, step, i = {}, 0, start, 0
    while pos < total:
        if step not in idle:
            n = min(sizes[i % len(sizes)], total - pos)
            out[step] = (pos, n, pos + n == total)
            pos, i = pos + n, i + 1
        step += 1
    return out


def _pcm_clip(n, seed):
    x = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.2 * 32768).round().clamp(-32768, 32767).to(torch.int16)
    x[5], x[6] = -32768, 32767                                               # full scale both ways
    return x


def _serve(codec, clips, plans, as_f32):
    """one pool run over all clips; as_f32: every session opened as f32, the s16 clips fed as pcm.float() / 32768"""
    pool = codec.encode_sessions(slots=3, max_push_samples=15360, sample_rates=(48000, 16000))
    slot, got, closed_at, sizes = {}, {k: [] for k in clips}, {}, []
    for step in range(max(max(p) for p in plans.values()) + 1):
        for k in clips:
            if ENC[k][3] == step:
                slot[k] = pool.open(sample_rate=ENC[k][1], sample_format="f32" if as_f32 else ENC[k][0])
        named = {k: plans[k][step] for k in clips if step in plans[k]}
        if not named:
            continue
        audio = {}
        for k, (pos, n, _) in named.items():
            a = clips[k][pos:pos + n]
            audio[slot[k]] = a.float() / 32768 if as_f32 and a.dtype == torch.int16 else a
        ids = pool.push(audio, final=[slot[k] for k, (_, _, fin) in named.items() if fin])
        assert set(ids) == set(audio)
        for k, (_, _, fin) in named.items():
            got[k].append(ids[slot[k]])
            if fin:
                closed_at[k] = step
        sizes.append(pool.allocated_bytes())
    return dict(pool=pool, slot=slot, got=got, closed_at=closed_at, sizes=sizes)


def encode_run(dev):
    if not _enc:
        from dmel_codec_amd.utils.pcm import from_pcm16
        codec = make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)
        clips = {}
        for k, (fmt, rate, secs, *_rest) in ENC.items():
            n = int(secs * rate) + 7
            clips[k] = (_pcm_clip(n, ord(k)) if fmt == "s16" else torch.randn(n, generator=torch.Generator().manual_seed(ord(k))) * 0.2).to(dev)
        ref = {}
        for k, c in clips.items():
            x = from_pcm16(c) if c.dtype == torch.int16 else c
            ref[k] = codec.encode(x[None], torch.tensor([c.shape[0]], device=dev), sample_rate=ENC[k][1])
        plans = {k: _plan(clips[k].shape[0], *ENC[k][3:]) for k in clips}
        _enc.update(codec=codec, clips=clips, ref=ref, plans=plans, pcm=_serve(codec, clips, plans, False),
                    f32=_serve(codec, clips, plans, True))
    return _enc


def test_from_pcm16_is_exact(dev):
    from dmel_codec_amd.utils.pcm import from_pcm16, to_pcm16
    r = encode_run(dev)
    for k in ("a", "c"):
        c = r["clips"][k]
        x = from_pcm16(c)
        assert x.dtype == torch.float32 and torch.equal(x, c.float() / 32768) and torch.equal(to_pcm16(x), c)
    two = r["clips"]["a"][:2 * 3001].view(2, 3001)                            # rows of odd length: the second one is not 16-byte aligned
    assert torch.equal(from_pcm16(two), two.float() / 32768) and torch.equal(to_pcm16(from_pcm16(two)), two)
    y = (torch.rand(3, 1001, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2).to(dev)
    assert torch.equal(to_pcm16(y).cpu(), oracle_to_s16(y))


@pytest.mark.parametrize("clip", ["a", "b", "c", "d", "e"])
def test_encode_sessions_equal_encode_of_the_converted_clip(dev, clip):
    """three slots, s16 at the codec's rate / f32 at 48 kHz / s16 at 16 kHz; staggered opens, ragged pushes with 0 samples, stalled
    slots, both slots that close first reopened with the other format"""
    r = encode_run(dev)
    ids, lens = r["ref"][clip]
    mine = torch.cat(r["pcm"]["got"][clip], dim=1)
    assert int(lens[0]) > 8 and mine.dtype == torch.int32
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    as_f32 = torch.cat(r["f32"]["got"][clip], dim=1)                          # the same session opened as f32, fed pcm.float() / 32768
    assert torch.equal(mine, as_f32)
    for a, b in zip(r["pcm"]["got"][clip], r["f32"]["got"][clip]):            # step by step, not only in the end
        assert torch.equal(a, b)


def test_encode_plan_covers_what_it_claims(dev):
    r = encode_run(dev)
    p, run = r["plans"], r["pcm"]
    assert 0 in [n for _, n, _ in p["a"].values()] and 0 in [n for _, n, _ in p["c"].values()]       # 0-sample pushes, both kinds of slot
    assert 2 not in p["a"] and 4 not in p["c"] and 5 not in p["c"] and max(p["c"]) > 5               # stalled while others advance
    assert run["slot"]["d"] == run["slot"]["a"] and run["slot"]["e"] == run["slot"]["b"]             # reopened, the other format each
    assert ENC["d"][3] > run["closed_at"]["a"] and ENC["e"][3] > run["closed_at"]["b"]
    assert any(step in p["b"] and step in p["c"] for step in p["a"])                                  # f32 rides in steps with s16 slots
    assert run["pool"].open_slots == [] and len(set(run["sizes"])) == 1 and run["sizes"][0] > 0      # constant from the first push on
    assert run["sizes"] == r["f32"]["sizes"]                                                          # a format sizes nothing


@pytest.mark.parametrize("n_s16", [0, 1, 3])
def test_encode_push_makes_one_convert_launch(dev, n_s16):
    r = encode_run(dev)
    codec = r["codec"]
    pool = codec.encode_sessions(slots=3, max_push_samples=15360, sample_rates=(48000,))
    rates = [SR, 48000, SR]
    fmts = ["s16" if i < n_s16 else "f32" for i in range(3)]
    slots = [pool.open(sample_rate=rates[i], sample_format=fmts[i]) for i in range(3)]
    chunk = lambda i, n: (_pcm_clip(n, 40 + i) if fmts[i] == "s16" else torch.randn(n) * 0.2).to(dev)
    step = lambda: pool.push({s: chunk(i, 7680 * rates[i] // SR - 100 * i) for i, s in enumerate(slots)})      # ~0.32 s for every slot
    for _ in range(6):                                                        # past the lookahead (~100 frames): every step emits tokens
        step()
    n, ids = prof_launches(step)
    assert n == (1 if n_s16 else 0) and all(t.shape[1] > 0 for t in ids.values())


def test_encode_refusals_change_nothing(dev):
    r = encode_run(dev)
    codec, clip = r["codec"], r["clips"]["a"]
    ids, lens = r["ref"]["a"]
    pool = codec.encode_sessions(slots=2, max_push_samples=15360)
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="s24")
    a, b = pool.open(sample_format="s16"), pool.open()
    assert (a, b) == (0, 1)
    got = [pool.push({a: clip[:9000], b: clip[:9000].float() / 32768})[a]]
    state = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b], pool.buf["samples"].clone())
    for bad in ({a: clip[9000:12000].float() / 32768}, {b: clip[9000:12000]},
                {a: clip[9000:12000], b: clip[9000:12000]}, {a: clip[9000:12000].to(torch.int32)}):
        with pytest.raises(ValueError, match="does not match"):
            pool.push(bad)
    now = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b])
    assert now == state[:5] and torch.equal(pool.buf["samples"], state[5])
    got.append(pool.push({a: clip[9000:20000], b: clip[9000:20000].float() / 32768})[a])
    got.append(pool.push({a: clip[20000:]}, final=(a,))[a])
    mine = torch.cat(got, dim=1)
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    assert pool.close(b).shape[0] == 8                                        # close() of an f32 slot in a pool that has served s16
    s = pool.open(sample_format="s16")
    pool.push({s: clip[:9000]})
    assert pool.close(s).dtype == torch.int32                                 # and of an s16 slot: its empty last push is int16


def test_encode_memory_is_constant_over_many_sessions(dev):
    codec = encode_run(dev)["codec"]
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, sample_rates=(48000,))
    x = _pcm_clip(4096 * 5, 99).to(dev)
    sizes, ptrs = set(), set()
    for cycle in range(8):
        a, b = pool.open(sample_rate=48000, sample_format="s16"), pool.open(sample_format="s16" if cycle % 2 else "f32")
        for i in range(5):
            ca = x[4096 * i:4096 * (i + 1) - 13 * cycle]
            cb = x[4096 * i:4096 * i + 3000 + cycle]
            pool.push({a: ca, b: cb if pool.fmt[b] == "s16" else cb.float() / 32768}, final=(a, b) if i == 4 else ())
            sizes.add(pool.allocated_bytes())
            ptrs.add(tuple(t.data_ptr() for t in pool.buf.values()) + tuple(t.data_ptr() for t in pool.rs.buf.values()))
    assert len(sizes) == 1 and len(ptrs) == 1 and pool.open_slots == []


# ------------------------------------------------------------------------------------ decode sessions
@pytest.fixture(scope="module")
def dcodec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


def _clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * 4, generator=g).to(dev)
    return ids, noise


class Feeder:
    def __init__(self, pool, ids, noise, rate, fmt):
        self.slot = pool.open(output_sample_rate=rate, sample_format=fmt)
        self.ids, self.noise, self.rate, self.fmt, self.pos, self.audio, self.mel = ids, noise, rate, fmt, 0, [], []

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, 4 * a:4 * self.pos]

    def got(self, out):
        audio, mel = out
        assert audio.ndim == 2 and audio.shape[0] == 1 and mel.shape[0] == 80
        assert audio.dtype == (torch.int16 if self.fmt == "s16" else torch.float32)
        self.audio.append(audio.clone())                          # a piece must survive the steps that follow
        self.mel.append(mel)

    def check(self, codec):
        from dmel_codec_amd.utils.resample import resample
        assert self.pos == self.ids.shape[1]
        T = self.ids.shape[1]
        audio, mel = codec.decode(self.ids[None], torch.tensor([T], device=self.ids.device), return_audios=True, noise=self.noise[None])
        want = audio[0] if self.rate is None else resample(audio[0], SR, self.rate)
        assert torch.equal(torch.cat(self.mel, dim=1), mel[0])
        mine = torch.cat(self.audio, dim=1)
        if self.fmt == "s16":
            assert mine.shape == want.shape and torch.equal(mine.cpu(), oracle_to_s16(want))
        else:
            assert mine.shape == want.shape and torch.equal(mine, want)      # the bits an f32 session has without any s16 slot beside it


def _step(pool, feeders, plan, final=()):
    ids, noise = {}, {}
    for i, n in plan.items():
        f = feeders[i]
        ids[f.slot], noise[f.slot] = f.take(n)
    out = pool.push(ids, noise=noise, final=[feeders[i].slot for i in final])
    assert set(out) == set(ids)
    for i in plan:
        feeders[i].got(out[feeders[i].slot])


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_decode_sessions_return_the_rounded_decode_audio(dev, dcodec, precision):
    """3 slots, s16 at the vocoder's rate / f32 at 48 kHz / s16 at the vocoder's rate, 5 sessions: the f32 slot reused by an s16 session
    at 48 kHz, an s16 slot reused by an f32 session; ragged pushes with 0- and 1-token pushes, one session shorter than the lookahead"""
    codec = dcodec
    assert int(codec.vocoder.h.get("sampling_rate", SR)) == SR
    codec.set_decode_precision(precision)
    try:
        pool = codec.decode_sessions(3, max_push_tokens=32, output_sample_rates=(48000,))
        lengths = [70, 3, 45, 28, 20]
        rates = [None, 48000, None, 48000, None]
        fmts = ["s16", "f32", "s16", "s16", "f32"]
        clips = [_clip(codec, 80 + i, T, dev) for i, T in enumerate(lengths)]
        new = lambda i: Feeder(pool, *clips[i], rates[i], fmts[i])
        f = [new(0)]
        _step(pool, f, {0: 27})
        sizes = {pool.allocated_bytes()}
        f.append(new(1))
        _step(pool, f, {0: 1, 1: 2})
        f.append(new(2))
        _step(pool, f, {0: 32, 1: 1, 2: 30}, final=(1,))                   # session 1 ends after 3 tokens: shorter than the lookahead
        f.append(new(3))                                                   # takes over session 1's slot: f32 -> s16, both at 48 kHz
        assert f[3].slot == f[1].slot
        _step(pool, f, {0: 0, 2: 15, 3: 28})
        _step(pool, f, {0: 10, 2: 0}, final=(2,))
        f.append(new(4))                                                   # takes over session 2's slot: s16 -> f32
        assert f[4].slot == f[2].slot
        _step(pool, f, {4: 20})
        sizes.add(pool.allocated_bytes())
        f[0].got(pool.close(f[0].slot))                                    # closes without tokens: the flush alone
        f[3].got(pool.close(f[3].slot))
        f[4].got(pool.close(f[4].slot))
        sizes.add(pool.allocated_bytes())
        assert pool.open_slots == [] and len(sizes) == 1 and max(pool.rs.fill) == 0
        assert all(sum(a.shape[1] for a in s.audio) > 0 for s in f)
        for s in f:
            s.check(codec)
    finally:
        codec.set_decode_precision("fp32")


@pytest.mark.parametrize("n_s16", [0, 1, 3])
def test_decode_push_makes_one_convert_launch(dev, dcodec, n_s16):
    pool = dcodec.decode_sessions(3, max_push_tokens=32, output_sample_rates=(48000,))
    rates = [None, 48000, None]
    fmts = ["s16" if i < n_s16 else "f32" for i in range(3)]
    feeders = [Feeder(pool, *_clip(dcodec, 60 + i, 96, dev), rates[i], fmts[i]) for i in range(3)]
    _step(pool, feeders, {0: 32, 1: 32, 2: 32})
    _step(pool, feeders, {0: 32, 1: 31, 2: 30})
    size = pool.allocated_bytes()
    n, _ = prof_launches(lambda: _step(pool, feeders, {0: 32, 1: 30, 2: 31}))
    assert n == (1 if n_s16 else 0) and all(s.audio[-1].shape[1] > 0 for s in feeders) and pool.allocated_bytes() == size


def test_decode_refusals(dev, dcodec):
    with pytest.raises(ValueError, match="return_audios=False"):
        dcodec.decode_sessions(2, return_audios=False).open(sample_format="s16")
    pool = dcodec.decode_sessions(2, max_push_tokens=8)
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="int16")
    assert pool.open_slots == [] and pool.buf is None
    s = pool.open(sample_format="s16")
    audio, mel = pool.close(s)                                             # nothing was pushed: empty, in the session's format
    assert audio.dtype == torch.int16 and audio.shape == (1, 0) and mel.shape == (80, 0)
