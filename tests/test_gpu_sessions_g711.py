"""Sessions that speak G.711 (8-bit mu-law / A-law, 8 kHz) on the GPU.  Every comparison is torch.equal, and every reference is a path
that does not know the format as a property of a session: encode() / decode() / resample() on one finished clip, with the companding
done outside -- from_g711 in front (exact), the numpy restatement of tests/g711_ref.py behind.  The tiny codecs are the ones
tests/test_gpu_sessions_pcm.py builds."""
import pytest
import torch

import g711_ref as ref
from test_gpu_pcm_convert import oracle_to_s16

pytestmark = pytest.mark.gpu

SR = 24000
TEL = 8000


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


def _law_clip(n, seed, law):
    """codes of a quiet noise, with both zeros and both full scales among them"""
    x = ref.f32_to_law(torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.2, law)
    x[3:7] = torch.tensor([0x00, 0x7F, 0x80, 0xFF], dtype=torch.uint8)
    return x


def _pcm_clip(n, seed):
    x = (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.2 * 32768).round().clamp(-32768, 32767).to(torch.int16)
    x[5], x[6] = -32768, 32767
    return x


def _chunk(fmt, n, seed):
    if fmt in ref.LAWS:
        return _law_clip(n, seed, fmt)
    return _pcm_clip(n, seed) if fmt == "s16" else torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 0.2


# ------------------------------------------------------------------------------------ encode sessions
# clip -> (format, rate, seconds, step of its open(), push sizes in its own samples, steps in which it is not named)
ENC = {"u": ("ulaw", TEL, 0.9, 0, [160, 2560, 0, 1700, 1, 2560], {2}),       # 20 ms packets next to large and empty pushes
       "a": ("alaw", TEL, 0.8, 0, [2560, 3, 0, 1365], {0, 4, 5}),            # first push one step late; stalls for two steps
       "s": ("s16", 48000, 0.6, 0, [15360, 7], set()),
       "f": ("f32", SR, 0.7, 0, [7680, 0, 5000], set()),
       "v": ("alaw", TEL, 0.5, 14, [2560, 160], set()),                      # takes over u's slot: mu-law -> A-law
       "w": ("ulaw", TEL, 0.5, 14, [160, 2560], set())}                      # takes over a's slot: A-law -> mu-law
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


def _serve(codec, clips, floats, plans, as_f32):
    """one pool run over all clips; as_f32: every session opened as f32 and fed the float clip (from_g711 / from_pcm16 of the whole)"""
    pool = codec.encode_sessions(slots=4, max_push_samples=15360, sample_rates=(48000, TEL))
    slot, got, closed_at, sizes = {}, {k: [] for k in clips}, {}, []
    for step in range(max(max(p) for p in plans.values()) + 1):
        for k in clips:
            if ENC[k][3] == step:
                slot[k] = pool.open(sample_rate=ENC[k][1], sample_format="f32" if as_f32 else ENC[k][0])
        named = {k: plans[k][step] for k in clips if step in plans[k]}
        if not named:
            continue
        audio = {slot[k]: (floats if as_f32 else clips)[k][pos:pos + n] for k, (pos, n, _) in named.items()}
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
        from dmel_codec_amd.utils.pcm import from_g711, from_pcm16
        codec = make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)
        clips, floats, ref_ids = {}, {}, {}
        for k, (fmt, rate, secs, *_rest) in ENC.items():
            clips[k] = _chunk(fmt, int(secs * rate) + 7, ord(k)).to(dev)
            floats[k] = from_g711(clips[k], fmt) if fmt in ref.LAWS else (from_pcm16(clips[k]) if fmt == "s16" else clips[k])
            ref_ids[k] = codec.encode(floats[k][None], torch.tensor([clips[k].shape[0]], device=dev), sample_rate=rate)
        plans = {k: _plan(clips[k].shape[0], *ENC[k][3:]) for k in clips}
        _enc.update(codec=codec, clips=clips, floats=floats, ref=ref_ids, plans=plans, law=_serve(codec, clips, floats, plans, False),
                    f32=_serve(codec, clips, floats, plans, True))
    return _enc


def test_from_and_to_g711_equal_the_restatement(dev):
    from dmel_codec_amd.utils.pcm import from_g711, to_g711
    r = encode_run(dev)
    for k in ("u", "a"):
        law, c = ENC[k][0], r["clips"][k]
        x = from_g711(c, law)
        assert x.dtype == torch.float32 and x.shape == c.shape and torch.equal(x.cpu(), ref.law_to_f32(c, law))
        back = to_g711(x, law)
        assert back.dtype == torch.uint8 and torch.equal(back.cpu(), ref.f32_to_law(x, law))
        same = back == c                                                      # the round trip: every code but mu-law's negative zero
        assert bool(same[c != 0x7F].all()) if law == "ulaw" else bool(same.all())
        two = c[:2 * 3001].view(2, 3001)                                      # rows of odd length: the second one is not 8-byte aligned
        assert torch.equal(from_g711(two, law).cpu(), ref.law_to_f32(two, law))
        y = (torch.rand(3, 1001, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2).to(dev)
        assert torch.equal(to_g711(y, law).cpu(), ref.f32_to_law(y, law))
    with pytest.raises(ValueError, match="unknown companding law"):
        from_g711(r["clips"]["u"], "s16")
    with pytest.raises(ValueError, match="expected torch.uint8"):
        from_g711(r["clips"]["s"], "ulaw")


@pytest.mark.parametrize("clip", list(ENC))
def test_encode_sessions_equal_encode_of_the_expanded_clip(dev, clip):
    """four slots, mu-law and A-law at 8 kHz / s16 at 48 kHz / f32 at the codec's rate; staggered opens, ragged pushes with 0 samples,
    stalled slots, both law slots reopened with the other law"""
    r = encode_run(dev)
    ids, lens = r["ref"][clip]
    mine = torch.cat(r["law"]["got"][clip], dim=1)
    assert int(lens[0]) > 8 and mine.dtype == torch.int32
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    as_f32 = torch.cat(r["f32"]["got"][clip], dim=1)                          # the same session opened as f32, fed from_g711(clip, law)
    assert torch.equal(mine, as_f32)
    for a, b in zip(r["law"]["got"][clip], r["f32"]["got"][clip]):            # step by step, not only in the end
        assert torch.equal(a, b)


def test_encode_plan_covers_what_it_claims(dev):
    r = encode_run(dev)
    p, run = r["plans"], r["law"]
    assert 0 in [n for _, n, _ in p["u"].values()] and 0 in [n for _, n, _ in p["a"].values()]       # 0-sample pushes
    assert 2 not in p["u"] and 0 not in p["a"] and 4 not in p["a"] and 5 not in p["a"] and max(p["a"]) > 5               # stalled while others advance
    assert run["slot"]["v"] == run["slot"]["u"] and run["slot"]["w"] == run["slot"]["a"]             # reopened, the other law each
    assert ENC["v"][3] > run["closed_at"]["u"] and ENC["w"][3] > run["closed_at"]["a"]
    assert any(step in p["u"] and step in p["a"] and step in p["f"] for step in p["s"])               # all four formats in one step
    assert run["pool"].open_slots == [] and len(set(run["sizes"])) == 1 and run["sizes"][0] > 0      # constant from the first push on
    assert run["sizes"] == r["f32"]["sizes"]                                                          # a format sizes nothing


@pytest.mark.parametrize("n_wire", [0, 1, 3])
def test_encode_push_makes_one_convert_launch(dev, n_wire):
    codec = encode_run(dev)["codec"]
    pool = codec.encode_sessions(slots=3, max_push_samples=15360, sample_rates=(48000, TEL))
    rates = [TEL, 48000, TEL]
    fmts = [f if i < n_wire else "f32" for i, f in enumerate(["ulaw", "s16", "alaw"])]
    slots = [pool.open(sample_rate=rates[i], sample_format=fmts[i]) for i in range(3)]
    step = lambda: pool.push({s: _chunk(fmts[i], 7680 * rates[i] // SR - 100 * i, 40 + i).to(dev) for i, s in enumerate(slots)})
    for _ in range(6):                                                        # past the lookahead (~100 frames): every step emits tokens
        step()
    size = pool.allocated_bytes()
    n, ids = prof_launches(step)
    assert n == (1 if n_wire else 0) and all(t.shape[1] > 0 for t in ids.values()) and pool.allocated_bytes() == size


def test_encode_refusals_change_nothing(dev):
    r = encode_run(dev)
    codec, clip, x = r["codec"], r["clips"]["u"], r["floats"]["u"]
    ids, lens = r["ref"]["u"]
    pool = codec.encode_sessions(slots=2, max_push_samples=4000, sample_rates=(TEL,))
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_rate=TEL, sample_format="u8")
    a, b = pool.open(sample_rate=TEL, sample_format="ulaw"), pool.open(sample_rate=TEL)
    assert (a, b) == (0, 1)
    got = [pool.push({a: clip[:3000], b: x[:3000]})[a]]
    state = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b], pool.buf["samples"].clone(),
             pool.rs.buf["rows"].clone(), list(pool.rs.fill))
    for bad in ({a: x[3000:4000]}, {b: clip[3000:4000]}, {a: clip[3000:4000], b: clip[3000:4000]}, {a: clip[3000:4000].to(torch.int16)},
                {a: clip[3000:4000].to(torch.int8)}):
        with pytest.raises(ValueError, match="does not match"):
            pool.push(bad)
    now = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b])
    assert now == state[:5] and torch.equal(pool.buf["samples"], state[5]) and torch.equal(pool.rs.buf["rows"], state[6])
    assert list(pool.rs.fill) == state[7]
    got.append(pool.push({a: clip[3000:7000], b: x[3000:7000]})[a])
    got.append(pool.push({a: clip[7000:]}, final=(a,))[a])
    mine = torch.cat(got, dim=1)
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    assert pool.close(b).shape[0] == 8                                        # close() of an f32 slot in a pool that has served G.711
    s = pool.open(sample_rate=TEL, sample_format="alaw")
    pool.push({s: r["clips"]["a"][:3000]})
    assert pool.close(s).dtype == torch.int32                                 # and of a law slot: its empty last push is uint8


def test_encode_memory_is_constant_over_many_sessions(dev):
    codec = encode_run(dev)["codec"]
    pool = codec.encode_sessions(slots=2, max_push_samples=1600, sample_rates=(TEL,))
    x = _law_clip(1600 * 5, 99, "ulaw").to(dev)
    sizes, ptrs = set(), set()
    for cycle in range(6):
        a = pool.open(sample_rate=TEL, sample_format=("ulaw", "alaw")[cycle % 2])
        b = pool.open(sample_rate=TEL, sample_format=("alaw", "f32", "ulaw")[cycle % 3])
        for i in range(5):
            ca = x[1600 * i:1600 * (i + 1) - 13 * cycle]
            cb = x[1600 * i:1600 * i + 1000 + cycle]
            pool.push({a: ca, b: cb if pool.fmt[b] != "f32" else cb.float() / 256}, final=(a, b) if i == 4 else ())
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


WIRE_DTYPE = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


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
        assert audio.dtype == WIRE_DTYPE[self.fmt]
        if self.fmt != "f32" and audio.shape[1]:                  # a view of the step's packed buffer, at a multiple of 16 bytes
            assert audio.data_ptr() % 16 == 0
        self.audio.append(audio.clone())                          # a piece must survive the steps that follow
        self.mel.append(mel)

    def check(self, codec):
        from dmel_codec_amd.utils.resample import resample
        assert self.pos == self.ids.shape[1]
        T = self.ids.shape[1]
        audio, mel = codec.decode(self.ids[None], torch.tensor([T], device=self.ids.device), return_audios=True, noise=self.noise[None])
        want = audio[0] if self.rate is None else resample(audio[0], SR, self.rate)
        assert torch.equal(torch.cat(self.mel, dim=1), mel[0])               # the mel of decode(), whatever the wire
        mine = torch.cat(self.audio, dim=1)
        assert mine.shape == want.shape
        if self.fmt in ref.LAWS:                                             # the restatement's encode of the s16 oracle rounding
            assert torch.equal(mine.cpu(), torch.from_numpy(ref.encode(oracle_to_s16(want).numpy(), self.fmt)))
        elif self.fmt == "s16":
            assert torch.equal(mine.cpu(), oracle_to_s16(want))              # the bits an s16 session has without law slots beside it
        else:
            assert torch.equal(mine, want)                                   # and an f32 session


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
def test_decode_sessions_return_the_companded_decode_audio(dev, dcodec, precision):
    """4 slots: mu-law at 8 kHz / A-law at 8 kHz / s16 at 48 kHz / f32 at the vocoder's rate, 6 sessions: the A-law slot reused by a
    mu-law session, the s16 slot by an A-law one; ragged pushes with 0- and 1-token pushes, one session shorter than the lookahead"""
    codec = dcodec
    assert int(codec.vocoder.h.get("sampling_rate", SR)) == SR
    codec.set_decode_precision(precision)
    try:
        pool = codec.decode_sessions(4, max_push_tokens=32, output_sample_rates=(TEL, 48000))
        lengths = [70, 3, 45, 28, 20, 33]
        rates = [TEL, TEL, 48000, None, TEL, TEL]
        fmts = ["ulaw", "alaw", "s16", "f32", "ulaw", "alaw"]
        clips = [_clip(codec, 80 + i, T, dev) for i, T in enumerate(lengths)]
        new = lambda i: Feeder(pool, *clips[i], rates[i], fmts[i])
        f = [new(0)]
        _step(pool, f, {0: 27})
        sizes = {pool.allocated_bytes()}
        f.append(new(1))
        _step(pool, f, {0: 1, 1: 2})
        f += [new(2), new(3)]
        _step(pool, f, {0: 32, 1: 1, 2: 30, 3: 28}, final=(1, 3))          # session 1 ends after 3 tokens: shorter than the lookahead
        f.append(new(4))                                                   # takes over session 1's slot: A-law -> mu-law
        assert f[4].slot == f[1].slot
        _step(pool, f, {0: 0, 2: 15, 4: 20}, final=(2,))
        f.append(new(5))                                                   # takes over session 2's slot: s16 at 48 kHz -> A-law at 8 kHz
        assert f[5].slot == f[2].slot
        _step(pool, f, {0: 10, 4: 0, 5: 32})
        _step(pool, f, {5: 1}, final=(5,))
        sizes.add(pool.allocated_bytes())
        f[0].got(pool.close(f[0].slot))                                    # closes without tokens: the flush alone
        f[4].got(pool.close(f[4].slot))
        sizes.add(pool.allocated_bytes())
        assert pool.open_slots == [] and len(sizes) == 1 and max(pool.rs.fill) == 0
        assert all(sum(a.shape[1] for a in s.audio) > 0 for s in f)
        for s in f:
            s.check(codec)
    finally:
        codec.set_decode_precision("fp32")


@pytest.mark.parametrize("n_wire", [0, 1, 3])
def test_decode_push_makes_one_convert_launch(dev, dcodec, n_wire):
    pool = dcodec.decode_sessions(3, max_push_tokens=32, output_sample_rates=(TEL, 48000))
    rates = [TEL, 48000, TEL]
    fmts = [f if i < n_wire else "f32" for i, f in enumerate(["alaw", "s16", "ulaw"])]
    feeders = [Feeder(pool, *_clip(dcodec, 60 + i, 96, dev), rates[i], fmts[i]) for i in range(3)]
    _step(pool, feeders, {0: 32, 1: 32, 2: 32})
    _step(pool, feeders, {0: 32, 1: 31, 2: 30})
    size = pool.allocated_bytes()
    n, _ = prof_launches(lambda: _step(pool, feeders, {0: 32, 1: 30, 2: 31}))
    assert n == (1 if n_wire else 0) and all(s.audio[-1].shape[1] > 0 for s in feeders) and pool.allocated_bytes() == size


def test_decode_refusals(dev, dcodec):
    for law in ref.LAWS:
        with pytest.raises(ValueError, match="return_audios=False"):
            dcodec.decode_sessions(2, return_audios=False).open(sample_format=law)
    pool = dcodec.decode_sessions(2, max_push_tokens=8, output_sample_rates=(TEL,))
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(output_sample_rate=TEL, sample_format="u8")
    assert pool.open_slots == [] and pool.buf is None
    for law in ref.LAWS:
        s = pool.open(output_sample_rate=TEL, sample_format=law)
        audio, mel = pool.close(s)                                         # nothing was pushed: empty, in the session's format
        assert audio.dtype == torch.uint8 and audio.shape == (1, 0) and mel.shape == (80, 0)
