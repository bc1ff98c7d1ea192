"""Decode sessions that shape their replies (decode_sessions(shape=True), open(shape=), set_gain / stop) on the GPU.  Every comparison
is equality.  A shaping session's concatenated audio is held to its wire chain (resample, format, channels) applied, over the whole
clip, to shape.scan(tones.splice(raw, inserts), requests, config, end): raw is decode()'s audio for an exact session and, for a
session that emits early with a cross-fade, its audio in a pool built without the option that runs the same script.  That pool is
also the reference of the mel pieces, of frames_emitted, of the session that does not shape and of the launch counts."""
import math

import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import pcm, shape, tones
from dmel_codec_amd.utils.resample import resample
from dmel_codec_amd.utils.shape import ShapeConfig
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

F, UP, RATE = 4, 256, 24000                            # mel frames per token, samples per frame, the vocoder's rate (the tiny codec)
MAX_PUSH = 16
FAMILIES = ("shape", "tones", "small", "pcm_convert", "crossfade", "stream_fork", "stream_pack", "dtmf", "voice", "conv_igemm", "aa_snake",
            "stft_logmel", "aa_snake_bwd", "conv_wgrad", "train_elementwise")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(700, n_mels=80, dmel_groups=8, encoder_layers=2).to(dev)


def clip(codec, seed, T, dev):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 175, (8, T), generator=g, dtype=torch.int32).to(dev)
    noise = torch.randn(codec.decoder.residual_channels, T * 4, generator=g).to(dev)
    return ids, noise


_decoded = {}


def decoded(codec, seed, T, dev):
    """decode() of the whole clip: (audio (n,), mel (80, m)) on the device, computed once"""
    if (seed, T) not in _decoded:
        if T == 0:
            _decoded[seed, T] = (torch.zeros(0, device=dev), torch.zeros(80, 0, device=dev))
        else:
            ids, noise = clip(codec, seed, T, dev)
            out = codec.decode(ids[None].contiguous(), torch.tensor([T], device=dev), return_audios=True, noise=noise[None].contiguous())
            _decoded[seed, T] = (out[0][0, 0].clone(), out[1][0].clone())
    return _decoded[seed, T]


def counts():
    torch.cuda.synchronize()
    return {f: _lib.prof_read(f)["launches"] for f in FAMILIES}


class Session:
    def __init__(self, pool, codec, dev, seed, T, kw, cfg, shaping):
        self.ids, self.noise = clip(codec, seed, T, dev)
        extra = dict(shape=cfg) if shaping and cfg is not None else {}
        self.slot, self.pos, self.audio, self.mel, self.emitted = pool.open(**kw, **extra), 0, [], [], []

    def take(self, n):
        a, self.pos = self.pos, self.pos + n
        return self.ids[:, a:self.pos], self.noise[:, F * a:F * self.pos]


# the sessions: 0 exact f32 at the vocoder's rate; 1 s16 stereo at 48 kHz, blocks of 64; 2 u-law at 8 kHz; 3 emits at once and
# cross-fades; 4 s16, sends a tone and ducks across it; 5 does not shape, leaves at 8 kHz and sends a tone (its last step places the
# step's resampler chunks, those of the shaping slots included); 6 exact, stopped in the middle of its reply, no limiter;
# 7 early, stopped; 8 stopped with nothing received
SESSIONS = [(410, 40, {}, True), (411, 36, dict(output_sample_rate=48000, sample_format="s16", channels=2), ShapeConfig(block_samples=64)),
            (412, 46, dict(output_sample_rate=8000, sample_format="ulaw"), True),
            (413, 20, dict(lookahead_frames=0, crossfade_samples=64), True), (414, 30, dict(sample_format="s16"), True),
            (415, 24, dict(output_sample_rate=8000), None),
            (416, 20, {}, ShapeConfig(limit=False)), (417, 8, dict(lookahead_frames=0, crossfade_samples=64), ShapeConfig(block_samples=32)),
            (418, 0, dict(sample_format="s16"), True)]
BEEP = tones.tone_program(1000, 30, RATE, ramp_ms=3)
# ("gain", session, dB, ramp ms, None | samples beyond now), ("stop", session, fade ms), ("send", session, program), ("open", session),
# (plan, final)
SCRIPT = [("gain", 1, 9.0, 20, None),
          ({0: 7, 1: 5, 2: 16, 3: 3, 4: 6, 5: 6, 6: 10, 7: 4}, ()),
          ("gain", 0, 10.0, 30, None), ("gain", 3, -12.0, 10, None), ("send", 4, BEEP), ("gain", 4, -15.0, 15, None), ("send", 5, BEEP),
          ({0: 0, 1: 11, 2: 0, 3: 0, 4: 5, 5: 5, 6: 10, 7: 4}, ()),
          ("gain", 2, 12.0, 5, None), ("gain", 0, -math.inf, 50, None), ("gain", 1, -6.0, 40, 1000),
          ("stop", 6, 20), ("stop", 7, 10), ("open", 8), ("stop", 8, 20),
          ({0: 16, 1: 9, 2: 9, 3: 5, 4: 8, 5: 0}, ()),
          ("gain", 0, 0.0, 100, None), ("gain", 4, 0.0, 30, None), ("gain", 3, 6.0, 300, None), ("gain", 3, 3.0, 0, 100),
          ({0: 1, 1: 11, 2: 5, 3: 8, 4: 11, 5: 13}, (1,)),
          ({0: 16, 2: 16, 3: 0, 5: 0}, (5,)),
          ({0: 0, 2: 0, 3: 4, 4: 0}, (0, 4)),
          ({2: 0, 3: 0}, (2, 3))]


def cfg_of(k):
    c = SESSIONS[k][3]
    return ShapeConfig() if c is True else c


def ms(v):
    return int(math.floor(v * RATE / 1000.0 + 0.5))


def run_script(codec, dev, shaping, park=None):
    """-> dict(ses, requests {session: [(P, g1, ramp)]}, ends {session: E}, inserts, steps, pool); park: (push index, pool factory, dict):
    before that push every open session is parked and restored into the pool the factory builds"""
    pool = codec.decode_sessions(9, max_push_tokens=MAX_PUSH, output_sample_rates=(48000, 8000), early_emit=True, crossfade_samples=64,
                                 tones=True, shape=shaping)
    ses = {k: Session(pool, codec, dev, *SESSIONS[k], shaping) for k in range(8)}
    requests, ends, inserts, steps, n_push = {k: [] for k in range(9)}, {}, {k: [] for k in range(9)}, [], 0
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        for item in SCRIPT:
            if item[0] == "open":
                ses[item[1]] = Session(pool, codec, dev, *SESSIONS[item[1]], shaping)
                continue
            if item[0] == "send":
                _, k, program = item
                inserts[k].append((F * ses[k].pos * UP, program))
                assert pool.send_tones(ses[k].slot, program) == tones.length(program)
                continue
            if item[0] == "gain":
                if shaping:
                    _, k, db, ramp_ms, ahead = item
                    now = pool.samples_fed(ses[k].slot)
                    at = pool.set_gain(ses[k].slot, db, ramp_ms, None if ahead is None else now + ahead)
                    assert at == now + (ahead or 0)
                    requests[k].append((at, 0.0 if db == -math.inf else 10.0 ** (db / 20.0), ms(ramp_ms)))
                continue
            if item[0] == "stop":
                _, k, fade_ms = item
                s = ses[k].slot
                if shaping:
                    now = pool.samples_fed(s)
                    requests[k].append((now, 0.0, ms(fade_ms)))
                    ends[k] = now + ms(fade_ms)
                    audio, mel = pool.stop(s, fade_ms)
                else:
                    audio, mel = pool.close(s)
                assert s not in pool.open_slots
                ses[k].audio.append(audio.clone()), ses[k].mel.append(mel)
                ses[k].slot = None
                continue
            plan, final = item
            if park is not None and n_push == park[0]:
                other, live = park[1](), [k for k in ses if ses[k].slot is not None]
                snaps = pool.park([ses[k].slot for k in live])
                moved, filler = {}, other.open()                            # slot 0 is taken while the sessions arrive: none keeps its index
                for k, s in zip(live[::-1], other.restore([snaps[ses[k].slot] for k in live[::-1]])):
                    moved[k], ses[k].slot = (ses[k].slot, s), s
                other.drop(filler)
                park[2].update(snaps=snaps, home=pool, moved=moved)
                pool = other
            n_push += 1
            ids, noise = {}, {}
            for k, n in plan.items():
                ids[ses[k].slot], noise[ses[k].slot] = ses[k].take(n)
            shapers = [k for k in plan if shaping and SESSIONS[k][3] is not None]
            fed = {k: pool.samples_fed(ses[k].slot) for k in shapers}
            before = counts()
            out = pool.push(ids, noise=noise, final=[ses[k].slot for k in final])
            after = counts()
            served = [k for k in shapers if k in final or pool.samples_fed(ses[k].slot) > fed[k]]
            reports = pool.shaped() if shaping else {}
            audio_n = {}
            for k in plan:
                audio, mel = out[ses[k].slot]
                ses[k].audio.append(audio.clone())
                ses[k].mel.append(mel)
                e = sum(m.shape[1] for m in ses[k].mel)
                ses[k].emitted.append(e)
                audio_n[k] = audio.numel()
                if k not in final:
                    assert pool.frames_emitted(ses[k].slot) == e
                    if k in shapers:
                        rep, N = reports[ses[k].slot], cfg_of(k).block(RATE)
                        assert rep.samples_in == pool.samples_fed(ses[k].slot) and rep.samples_in - rep.samples_out == pool.shold[ses[k].slot]
                        assert rep.peak_out <= float(torch.tensor(cfg_of(k).ceiling, dtype=torch.float32)) and rep.block == N
                        pk, gn = pool.shape_blocks(ses[k].slot)
                        assert pk.shape == gn.shape and pk.shape[0] == (rep.blocks if len(ses[k].audio) == 1 else pk.shape[0])
            for k in final:
                ses[k].slot = None
            steps.append(dict(delta={f: after[f] - before[f] for f in FAMILIES}, served=served, audio_n=audio_n, plan=plan, final=final))
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert pool.open_slots == []
    return dict(ses=ses, requests=requests, ends=ends, inserts=inserts, steps=steps, pool=pool)


_runs = {}


def runs(codec, dev):
    if not _runs:
        _runs["shape"] = run_script(codec, dev, True)
        _runs["plain"] = run_script(codec, dev, False)
    return _runs


def cat_audio(s):
    return torch.cat([a if a.ndim == 2 and a.shape[0] != 1 else a.reshape(-1) for a in s.audio])


def wire(k, x):
    """the whole-clip wire chain of session k over x (n,) at the vocoder's rate"""
    kw = SESSIONS[k][2]
    rate, fmt, ch = kw.get("output_sample_rate", RATE), kw.get("sample_format", "f32"), kw.get("channels", 1)
    y = resample(x[None], RATE, rate)[0] if rate != RATE else x
    if ch > 1:
        return pcm.fan_out(y, ch, fmt)
    return y if fmt == "f32" else pcm.to_pcm16(y) if fmt == "s16" else pcm.to_g711(y, fmt)


def expected(r, k, codec, dev):
    """the contract sentence for session k of the run r"""
    seed, T, kw, _ = SESSIONS[k]
    raw = cat_audio(runs(codec, dev)["plain"]["ses"][k]) if "lookahead_frames" in kw else decoded(codec, seed, T, dev)[0]
    assert raw.dtype == torch.float32 and raw.shape == (T * F * UP,)
    z = tones.splice(raw.cpu().numpy(), r["inserts"][k], RATE)
    y = shape.scan(z, r["requests"][k], cfg_of(k), RATE, end=r["ends"].get(k), final=True)[0]
    return wire(k, y.to(dev)), z.shape[0]


def test_every_shaping_session_is_the_wire_chain_over_the_scan(dev, codec):
    r = runs(codec, dev)
    t, p = r["shape"]["ses"], r["plain"]["ses"]
    for k, (seed, T, kw, cfg) in enumerate(SESSIONS):
        got = cat_audio(t[k])
        if cfg is None:                                                      # the session that does not shape: piece for piece
            assert len(t[k].audio) == len(p[k].audio) and all(torch.equal(a, b) for a, b in zip(t[k].audio, p[k].audio))
            raw = decoded(codec, seed, T, dev)[0]
            assert torch.equal(got, wire(k, torch.from_numpy(tones.splice(raw.cpu().numpy(), r["shape"]["inserts"][k], RATE)).to(dev)))
        else:
            want, n_z = expected(r["shape"], k, codec, dev)
            assert len(r["shape"]["requests"][k]) > 0
            assert got.dtype == want.dtype and got.shape == want.shape, (k, got.shape, want.shape)
            assert torch.equal(got, want), f"session {k}: {int((got != want).sum())} of {got.numel()} samples differ"
        # mel pieces and frames_emitted are the plain pool's
        assert t[k].emitted == p[k].emitted and len(t[k].mel) == len(p[k].mel)
        assert all(torch.equal(a, b) for a, b in zip(t[k].mel, p[k].mel))
    # the stops: an exact session in the middle of its reply (its flush is longer than the fade), an early one, one with nothing
    e = r["shape"]["ends"]
    assert e[6] < 20 * F * UP and cat_audio(t[6]).shape[0] == e[6] and cat_audio(p[6]).shape[0] == 20 * F * UP
    assert cat_audio(t[7]).shape[0] == min(e[7], cat_audio(p[7]).shape[0]) and cat_audio(t[8]).numel() == 0
    assert float(cat_audio(t[6])[-1].abs()) < 1e-4                            # the fade reached silence


def test_one_shape_launch_per_serving_step_and_nothing_else_changes(dev, codec):
    r = runs(codec, dev)
    st, sp = r["shape"]["steps"], r["plain"]["steps"]
    assert len(st) == len(sp) == 7
    for a, b in zip(st, sp):
        assert a["delta"]["shape"] == (1 if a["served"] else 0) and b["delta"]["shape"] == 0, (a, b)
        for f in FAMILIES:
            if f not in ("shape", "small", "pcm_convert"):
                assert a["delta"][f] == b["delta"][f], (f, a, b)

        # the shape launch is one record of "small" as well.  A limiter holds samples back and hands them out later, so a step's audio
        # may be there in one pool and not in the other, and audio takes the launches audio takes: ONE resample launch in a step in
        # which a session at another rate gets samples, ONE convert launch in a step in which a session with a wire format or
        # channels does (one record of "small" each, the convert launch one of "pcm_convert" too).  Both follow from the audio each
        # pool returned in the step
        def launches(step, option):
            return int(any(step["audio_n"][k] and option(SESSIONS[k][2]) for k in step["plan"]))
        resamples = [launches(x, lambda kw: "output_sample_rate" in kw) for x in (a, b)]
        converts = [launches(x, lambda kw: "sample_format" in kw or "channels" in kw) for x in (a, b)]
        assert a["delta"]["pcm_convert"] == converts[0] and b["delta"]["pcm_convert"] == converts[1], (a, b)
        assert a["delta"]["small"] - b["delta"]["small"] == a["delta"]["shape"] + resamples[0] - resamples[1] + converts[0] - converts[1], (a, b)
    assert sum(bool(a["served"]) for a in st) >= 5
    # a step of the shape pool that serves no shaping slot shows the plain pool's records, family by family
    pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, shape=True)
    bare = codec.decode_sessions(2, max_push_tokens=MAX_PUSH)
    ids, noise = clip(codec, 415, 24, dev)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        deltas = []
        for q in (pool, bare):
            s = q.open()
            before = counts()
            q.push({s: ids[:, :16]}, noise={s: noise[:, :64]})
            q.push({s: ids[:, 16:]}, noise={s: noise[:, 64:]}, final=(s,))
            after = counts()
            deltas.append({f: after[f] - before[f] for f in FAMILIES})
        assert deltas[0] == deltas[1] and deltas[0]["shape"] == 0
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert not any(k.startswith("shape") for k in bare.buf) and bare.allocated_bytes() < pool.allocated_bytes()


def test_park_in_the_middle_of_a_ramp_and_of_a_block(dev, codec):
    r, info = runs(codec, dev), {}
    moved = run_script(codec, dev, True, park=(2, lambda: codec.decode_sessions(
        11, max_push_tokens=MAX_PUSH, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64, tones=True, shape=True), info))
    snaps = info["snaps"]
    shaping = [sn for sn in snaps.values() if "shape" in sn.meta]
    assert len(shaping) == 5 and len(snaps) == 6 and all(sn.meta["version"] == 1 for sn in snaps.values())
    assert any(sg[0] <= sn.meta["shape_fed"] < sg[0] + sg[3] for sn in shaping for sg in sn.meta["shape_segments"])      # inside a ramp
    assert any(sn.meta["shape_hold"] % ShapeConfig.from_dict(sn.meta["shape"]).block(RATE) for sn in shaping)              # inside a block
    assert all(sn.meta["layout"][-1][:3] == ["shape", 1, ShapeConfig.from_dict(sn.meta["shape"]).state_words(RATE)] for sn in shaping
               if sn.meta["shape_fed"])
    assert sum(a != b for a, b in info["moved"].values()) >= 5 and info["home"].open_slots == []      # into other slots of another pool
    for k in range(9):
        a, b = moved["ses"][k], r["shape"]["ses"][k]
        assert len(a.audio) == len(b.audio) and all(torch.equal(x, y) for x, y in zip(a.audio, b.audio)), k
        assert all(torch.equal(x, y) for x, y in zip(a.mel, b.mel)) and a.emitted == b.emitted
    # a pool without the option refuses the snapshot of a shaping session and takes no slot
    plain = codec.decode_sessions(4, max_push_tokens=MAX_PUSH, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64,
                                  tones=True)
    for sn in shaping:
        with pytest.raises(ValueError, match="shape=True"):
            plain.restore([sn])
    assert plain.open_slots == []


def test_refusals_on_a_live_pool(dev, codec):
    pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, early_emit=True, shape=True)
    a, b = pool.open(shape=True, lookahead_frames=0), pool.open()            # a session that emits at once: its shaper has samples
    ids, noise = clip(codec, 415, 24, dev)
    pool.push({a: ids[:, :16], b: ids[:, :16]}, noise={a: noise[:, :64], b: noise[:, :64]})
    fed = pool.samples_fed(a)
    assert fed > 0
    for call, match in ((lambda: pool.set_gain(a, 0.0, at_sample=fed - 1), "anchor"), (lambda: pool.set_gain(a, 13.0), "max_gain"),
                        (lambda: pool.stop(b), "without shape="), (lambda: pool.set_gain(b, 0.0), "without shape=")):
        with pytest.raises(ValueError, match=match):
            call()
    assert pool.open_slots == [a, b] and pool.sreq[a] == []
    held = pool.shold[a]
    audio, mel = pool.stop(a, fade_ms=5)
    # the session had handed out all it received: its stream ends inside the fade, and what the limiter held is what is left
    assert 120 <= held < 240 and audio.shape == (1, held) and float(audio.abs().max()) <= float(torch.tensor(0.98, dtype=torch.float32))
    assert pool.open_slots == [b]
    with pytest.raises(RuntimeError):
        pool.set_gain(a, 0.0)
    pool.drop(b)
