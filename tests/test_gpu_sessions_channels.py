"""Sessions whose wire carries interleaved channels, on the GPU.  Every comparison is torch.equal, and every reference is a path that
does not know the channel count as a property of a session: encode() of the downmixed clip, the same session opened mono "f32" and fed
the CPU restatement's chunks (tests/channels_ref.py), the same reply opened with channels=1.  The tiny codecs are the ones
tests/test_gpu_sessions_g711.py builds."""
import pytest
import torch

import channels_ref as cref
from test_gpu_sessions_g711 import SR, TEL, _chunk, _clip, _plan, make_codec, prof_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _frames(fmt, n, c, seed):
    x = _chunk(fmt, n * c, seed)
    return x.view(n, c) if c > 1 else x


# ------------------------------------------------------------------------------------ the whole-clip helpers
def test_downmix_and_fan_out_equal_the_restatement(dev):
    from dmel_codec_amd.utils.pcm import downmix, fan_out
    for fmt in ("f32", "s16", "ulaw", "alaw"):
        name = fmt if fmt in ("ulaw", "alaw") else None                     # the dtype says f32 and s16
        for c in (1, 2, 3, 8):
            x = _frames(fmt, 3001, c, 11 * c).view(3001, c)
            for k in [None] + list(range(c if c > 1 else 0)):
                y = downmix(x.to(dev), name, channel=k)
                assert y.dtype == torch.float32 and y.shape == (3001,)
                assert torch.equal(cref.words(y.cpu()), cref.words(cref.downmix(x, fmt, k)))
            rows = _frames(fmt, 2 * 1501, c, 5).view(2, 1501, c)            # rows of odd length: the second one is off the wide path
            y = downmix(rows.to(dev), name)
            assert y.shape == (2, 1501) and all(torch.equal(y[b].cpu(), cref.downmix(rows[b], fmt)) for b in range(2))
            m = (torch.rand(2, 1501, generator=torch.Generator().manual_seed(c)) * 2.4 - 1.2)
            out = fan_out(m.to(dev), c, fmt)
            assert out.dtype == cref.DTYPE[fmt] and out.shape == (2, 1501, c) and out.is_contiguous()
            assert all(torch.equal(cref.words(out[b].cpu()), cref.words(cref.fan_out(m[b], c, fmt))) for b in range(2))
            assert fan_out(m[0].to(dev), c, fmt).shape == (1501, c)
        assert downmix(torch.empty(0, 2, dtype=cref.DTYPE[fmt], device=dev), name).shape == (0,)
    assert fan_out(torch.empty(0, device=dev), 2, "s16").shape == (0, 2)


# ------------------------------------------------------------------------------------ encode sessions
# clip -> (format, rate, channels, channel, seconds, step of its open(), push sizes in its own frames, steps in which it is not named)
ENC = {"s": ("s16", 48000, 2, None, 0.6, 0, [15360, 7, 9000], set()),          # stereo 16-bit at 48 kHz, the mean
       "u": ("ulaw", TEL, 2, 1, 0.9, 0, [160, 2560, 0, 1700, 1, 2560], {2}),   # a call recording's right channel; stalls in step 2
       "t": ("f32", SR, 3, None, 0.7, 0, [7680, 0, 5001], {1}),                # three float channels at the codec's rate
       "m": ("f32", SR, 1, None, 0.7, 1, [7680, 0, 5000], set()),              # mono f32 beside them, opened a step late
       "r": ("s16", TEL, 3, 2, 0.5, 14, [2560, 161], set()),                   # takes over s's slot: stereo at 48 kHz -> channel 2 of 3 at 8 kHz
       "q": ("alaw", TEL, 1, None, 0.5, 14, [160, 2560], set())}               # takes over u's slot: stereo mu-law -> mono A-law
_enc = {}


def _serve(codec, specs, clips, plans, dev, as_mono_f32):
    """one pool run over all clips; as_mono_f32: every session opened mono f32 and fed the CPU restatement's downmix of each chunk"""
    pool = codec.encode_sessions(slots=4, max_push_samples=15360, sample_rates=(48000, TEL))
    slot, got, closed_at, sizes = {}, {k: [] for k in clips}, {}, []
    for step in range(max(max(p) for p in plans.values()) + 1):
        for k in clips:
            if specs[k][5] == step:
                fmt, rate, c, pick = specs[k][:4]
                slot[k] = pool.open(sample_rate=rate) if as_mono_f32 else pool.open(sample_rate=rate, sample_format=fmt, channels=c,
                                                                                    channel=pick)
        named = {k: plans[k][step] for k in clips if step in plans[k]}
        if not named:
            continue
        audio = {}
        for k, (pos, n, _) in named.items():
            fmt, _, c, pick = specs[k][:4]
            chunk = clips[k][pos:pos + n]
            if as_mono_f32:
                chunk = cref.downmix(chunk.cpu().view(n, c), fmt, pick).to(dev)
            audio[slot[k]] = chunk
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
        from dmel_codec_amd.utils.pcm import downmix
        codec = make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)
        clips, ref_ids = {}, {}
        for k, (fmt, rate, c, pick, secs, *_rest) in ENC.items():
            n = int(secs * rate) + 7
            clips[k] = _frames(fmt, n, c, ord(k)).to(dev)
            mono = downmix(clips[k].view(n, c), fmt if fmt in ("ulaw", "alaw") else None, channel=pick)
            ref_ids[k] = codec.encode(mono[None], torch.tensor([n], device=dev), sample_rate=rate)
        plans = {k: _plan(clips[k].shape[0], *ENC[k][5:]) for k in clips}
        _enc.update(codec=codec, clips=clips, ref=ref_ids, plans=plans, ch=_serve(codec, ENC, clips, plans, dev, False),
                    mono=_serve(codec, ENC, clips, plans, dev, True))
    return _enc


@pytest.mark.parametrize("clip", list(ENC))
def test_encode_sessions_equal_encode_of_the_downmixed_clip(dev, clip):
    """four slots -- stereo s16 at 48 kHz / stereo mu-law at 8 kHz, channel 1 / 3-channel f32 / mono f32 -- with staggered opens, ragged
    pushes with 0 frames, stalled slots, and two slots reopened with another channel count"""
    r = encode_run(dev)
    ids, lens = r["ref"][clip]
    mine = torch.cat(r["ch"]["got"][clip], dim=1)
    assert int(lens[0]) > 8 and mine.dtype == torch.int32
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    for a, b in zip(r["ch"]["got"][clip], r["mono"]["got"][clip]):            # the mono f32 session fed the restatement, step by step
        assert torch.equal(a, b)
    assert len(r["ch"]["got"][clip]) == len(r["mono"]["got"][clip])


def test_encode_plan_covers_what_it_claims(dev):
    r = encode_run(dev)
    p, run = r["plans"], r["ch"]
    assert 0 in [n for _, n, _ in p["u"].values()] and 0 in [n for _, n, _ in p["t"].values()]       # 0-frame pushes
    assert 2 not in p["u"] and 1 not in p["t"] and 2 in p["s"] and 1 in p["s"]                        # stalled while others advance
    assert run["slot"]["r"] == run["slot"]["s"] and ENC["r"][5] > run["closed_at"]["s"]               # reopened: 2 -> 3 channels
    assert run["slot"]["q"] == run["slot"]["u"] and ENC["q"][5] > run["closed_at"]["u"]               # reopened: 2 channels -> mono
    assert any(all(step in p[k] for k in "sutm") for step in p["s"])                                  # all four kinds in one step
    assert run["pool"].open_slots == [] and len(set(run["sizes"])) == 1 and run["sizes"][0] > 0      # constant from the first push on
    assert run["sizes"] == r["mono"]["sizes"]                                                         # a channel count sizes nothing


def test_two_picks_of_one_stereo_tensor_are_the_two_parties(dev):
    from dmel_codec_amd.utils.pcm import from_pcm16
    r = encode_run(dev)
    codec = r["codec"]
    n = 9000
    call = _frames("s16", n, 2, 77).to(dev)
    pool = codec.encode_sessions(slots=2, max_push_samples=4000, sample_rates=(TEL,))
    left, right = pool.open(sample_rate=TEL, sample_format="s16", channels=2, channel=0), \
        pool.open(sample_rate=TEL, sample_format="s16", channels=2, channel=1)
    got = {left: [], right: []}
    for a in range(0, n, 4000):
        piece = call[a:a + 4000]
        out = pool.push({left: piece, right: piece}, final=(left, right) if a + 4000 >= n else ())
        for s in got:
            got[s].append(out[s])
    for s, k in ((left, 0), (right, 1)):
        ids, lens = codec.encode(from_pcm16(call[:, k].contiguous())[None], torch.tensor([n], device=dev), sample_rate=TEL)
        assert torch.equal(torch.cat(got[s], dim=1), ids[0, :, :int(lens[0])])
    assert not torch.equal(torch.cat(got[left], dim=1), torch.cat(got[right], dim=1))


@pytest.mark.parametrize("n_ch", [0, 1, 3])
def test_encode_push_makes_one_convert_launch(dev, n_ch):
    codec = encode_run(dev)["codec"]
    pool = codec.encode_sessions(slots=3, max_push_samples=15360, sample_rates=(48000, TEL))
    rates = [SR, 48000, TEL]
    wire = [("f32", 3, None), ("s16", 2, None), ("ulaw", 2, 1)]               # an f32 slot with channels converts as well
    cfg = [wire[i] if i < n_ch else ("f32", 1, None) for i in range(3)]
    slots = [pool.open(sample_rate=rates[i], sample_format=cfg[i][0], channels=cfg[i][1], channel=cfg[i][2]) for i in range(3)]
    step = lambda: pool.push({s: _frames(cfg[i][0], 7680 * rates[i] // SR - 100 * i, cfg[i][1], 40 + i).to(dev)
                              for i, s in enumerate(slots)})
    for _ in range(6):                                                        # past the lookahead (~100 frames): every step emits tokens
        step()
    size = pool.allocated_bytes()
    n, ids = prof_launches(step)
    assert n == (1 if n_ch else 0) and all(t.shape[1] > 0 for t in ids.values()) and pool.allocated_bytes() == size
    mono = codec.encode_sessions(slots=3, max_push_samples=15360, sample_rates=(48000, TEL))
    mono.push({mono.open(): torch.zeros(100, device=dev)})
    assert mono.allocated_bytes() == size                                     # a mono pool's memory


def test_encode_refusals_change_nothing(dev):
    r = encode_run(dev)
    codec, clip = r["codec"], r["clips"]["u"]
    ids, lens = r["ref"]["u"]
    pool = codec.encode_sessions(slots=2, max_push_samples=4000, sample_rates=(TEL,))
    for kw in (dict(channels=9), dict(channels=0), dict(channels=2, channel=2), dict(channel=0)):
        with pytest.raises(ValueError, match="channel"):
            pool.open(sample_rate=TEL, **kw)
    assert pool.open_slots == []
    a, b = pool.open(sample_rate=TEL, sample_format="ulaw", channels=2, channel=1), pool.open()
    assert (a, b) == (0, 1)
    x = torch.randn(7200, generator=torch.Generator().manual_seed(1)).to(dev) * 0.1
    got = [pool.push({a: clip[:3000], b: x[:3000]})[a]]
    state = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b], pool.buf["samples"].clone(),
             pool.rs.buf["rows"].clone(), list(pool.rs.fill))
    nxt = clip[3000:4000]
    for bad, msg in (({a: nxt[:, 1]}, "channels=2"), ({a: nxt[:, 1].contiguous()[None]}, "channels=2"),
                     ({a: nxt.t().contiguous()}, "channels=2"), ({a: nxt.repeat(1, 2)[:, :3].contiguous()}, "channels=2"),
                     ({a: nxt.repeat(1, 2)[:, :2]}, "channels=2"), ({a: nxt.float()}, "does not match"),
                     ({a: nxt, b: x[3000:4000].view(500, 2)}, "expected mono audio"), ({a: clip[3000:7001]}, "max_push_samples")):
        with pytest.raises(ValueError, match=msg):
            pool.push(bad)
    now = (pool.sched[a].samples, pool.tail[a], pool.s0[a], pool.sched[b].samples, pool.tail[b])
    assert now == state[:5] and torch.equal(pool.buf["samples"], state[5]) and torch.equal(pool.rs.buf["rows"], state[6])
    assert list(pool.rs.fill) == state[7]
    got.append(pool.push({a: clip[3000:7000], b: x[3000:7000]})[a])
    got.append(pool.push({a: clip[7000:]}, final=(a,))[a])
    mine = torch.cat(got, dim=1)
    assert mine.shape[1] == int(lens[0]) and torch.equal(mine, ids[0, :, :int(lens[0])])
    assert pool.close(b).shape[0] == 8
    s = pool.open(sample_format="s16", channels=3)
    pool.push({s: _frames("s16", 3000, 3, 2).to(dev)})
    assert pool.close(s).dtype == torch.int32                                 # close() of a slot with channels: its empty push is (0, 3)


# ------------------------------------------------------------------------------------ decode sessions
@pytest.fixture(scope="module")
def dcodec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


class Reply:
    def __init__(self, pool, ids, noise, rate, fmt, channels):
        self.slot = pool.open(output_sample_rate=rate, sample_format=fmt, channels=channels)
        self.ids, self.noise, self.fmt, self.c, self.pos, self.audio, self.mel = ids, noise, fmt, channels, 0, [], []

    def take(self, n):
        a = self.pos
        self.pos += n
        return self.ids[:, a:self.pos], self.noise[:, 4 * a:4 * self.pos]

    def got(self, out):
        audio, mel = out
        assert audio.dtype == cref.DTYPE[self.fmt] and audio.ndim == 2 and mel.shape[0] == 80
        assert audio.shape[1] == self.c if self.c > 1 else audio.shape[0] == 1           # (n, c) interleaved, (1, n) mono
        if (self.c > 1 or self.fmt != "f32") and audio.numel():                # a view of the step's packed buffer, at a multiple of 16 bytes
            assert audio.data_ptr() % 16 == 0 and audio.is_contiguous()
        self.audio.append(audio.clone())                                      # a piece must survive the steps that follow
        self.mel.append(mel)

    def channels(self):
        """the concatenated audio as a list of mono channels"""
        a = torch.cat(self.audio, dim=0 if self.c > 1 else 1)
        return [a[:, j] for j in range(self.c)] if self.c > 1 else [a[0]]


def _step(pool, replies, plan, final=()):
    ids, noise = {}, {}
    for i, n in plan.items():
        ids[replies[i].slot], noise[replies[i].slot] = replies[i].take(n)
    out = pool.push(ids, noise=noise, final=[replies[i].slot for i in final])
    assert set(out) == set(ids)
    for i in plan:
        replies[i].got(out[replies[i].slot])


def _decode_run(codec, clips, dev, with_channels):
    """4 slots, 6 replies: stereo s16 at 48 kHz / 3-channel A-law at 8 kHz / stereo f32 / mono f32; the A-law slot reused by an
    8-channel mu-law reply, the s16 slot by a mono s16 one.  with_channels=False: the same replies opened with channels=1"""
    pool = codec.decode_sessions(4, max_push_tokens=32, output_sample_rates=(TEL, 48000))
    rates = [48000, TEL, None, None, TEL, 48000]
    fmts = ["s16", "alaw", "f32", "f32", "ulaw", "s16"]
    chans = [2, 3, 2, 1, 8, 1] if with_channels else [1] * 6
    new = lambda i: Reply(pool, *clips[i], rates[i], fmts[i], chans[i])
    f = [new(0)]
    _step(pool, f, {0: 27})
    sizes = {pool.allocated_bytes()}
    f.append(new(1))
    _step(pool, f, {0: 1, 1: 2})
    f += [new(2), new(3)]
    _step(pool, f, {0: 32, 1: 1, 2: 30, 3: 28}, final=(1, 3))                 # reply 1 ends after 3 tokens: shorter than the lookahead
    f.append(new(4))                                                          # takes over reply 1's slot: 3 channels -> 8
    assert f[4].slot == f[1].slot
    _step(pool, f, {0: 0, 2: 15, 4: 20}, final=(2,))
    f.append(new(5))                                                          # takes over reply 2's slot: stereo f32 -> mono s16
    assert f[5].slot == f[2].slot
    _step(pool, f, {0: 10, 4: 0, 5: 32})
    _step(pool, f, {5: 1}, final=(5,))
    sizes.add(pool.allocated_bytes())
    f[0].got(pool.close(f[0].slot))                                           # closes without tokens: the flush alone
    f[4].got(pool.close(f[4].slot))
    sizes.add(pool.allocated_bytes())
    assert pool.open_slots == [] and len(sizes) == 1 and max(pool.rs.fill) == 0
    return f, sizes


@pytest.mark.parametrize("precision", ["fp32", "fp32_bf16x3"])
def test_decode_sessions_return_every_channel_of_the_mono_reply(dev, dcodec, precision):
    codec = dcodec
    codec.set_decode_precision(precision)
    try:
        clips = [_clip(codec, 80 + i, T, dev) for i, T in enumerate([70, 3, 45, 28, 20, 33])]
        many, size_many = _decode_run(codec, clips, dev, True)
        mono, size_mono = _decode_run(codec, clips, dev, False)
        assert size_many == size_mono                                         # a channel count sizes nothing
        for a, b in zip(many, mono):
            want = b.channels()[0]
            assert want.numel() > 0 and len(a.channels()) == a.c
            for ch in a.channels():                                           # every channel: the bits of the mono reply
                assert torch.equal(cref.words(ch.contiguous()), cref.words(want))
            assert torch.equal(torch.cat(a.mel, dim=1), torch.cat(b.mel, dim=1))
            assert [p.shape[0] if a.c > 1 else p.shape[1] for p in a.audio] == [p.shape[1] for p in b.audio]       # piece by piece
        T = clips[3][0].shape[1]                                              # and the mono f32 reply is decode()'s
        audio, mel = codec.decode(clips[3][0][None], torch.tensor([T], device=dev), return_audios=True, noise=clips[3][1][None])
        assert torch.equal(many[3].channels()[0], audio[0, 0]) and torch.equal(torch.cat(many[3].mel, dim=1), mel[0])
    finally:
        codec.set_decode_precision("fp32")


@pytest.mark.parametrize("n_ch", [0, 1, 3])
def test_decode_push_makes_one_convert_launch(dev, dcodec, n_ch):
    pool = dcodec.decode_sessions(3, max_push_tokens=32, output_sample_rates=(TEL, 48000))
    rates = [None, 48000, TEL]
    wire = [("f32", 2), ("s16", 2), ("alaw", 3)]                              # an f32 reply with channels converts as well
    cfg = [wire[i] if i < n_ch else ("f32", 1) for i in range(3)]
    replies = [Reply(pool, *_clip(dcodec, 60 + i, 96, dev), rates[i], *cfg[i]) for i in range(3)]
    _step(pool, replies, {0: 32, 1: 32, 2: 32})
    _step(pool, replies, {0: 32, 1: 31, 2: 30})
    size = pool.allocated_bytes()
    n, _ = prof_launches(lambda: _step(pool, replies, {0: 32, 1: 30, 2: 31}))
    assert n == (1 if n_ch else 0) and all(s.audio[-1].numel() > 0 for s in replies) and pool.allocated_bytes() == size


def test_decode_refusals(dev, dcodec):
    with pytest.raises(ValueError, match="return_audios=False"):
        dcodec.decode_sessions(2, return_audios=False).open(channels=2)
    pool = dcodec.decode_sessions(2, max_push_tokens=8, output_sample_rates=(TEL,))
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match="channels="):
            pool.open(output_sample_rate=TEL, channels=bad)
    assert pool.open_slots == [] and pool.buf is None
    for fmt, c in (("f32", 2), ("s16", 3), ("ulaw", 8)):
        s = pool.open(output_sample_rate=TEL, sample_format=fmt, channels=c)
        audio, mel = pool.close(s)                                            # nothing was pushed: empty, in the session's shape and format
        assert audio.dtype == cref.DTYPE[fmt] and audio.shape == (0, c) and mel.shape == (80, 0)
