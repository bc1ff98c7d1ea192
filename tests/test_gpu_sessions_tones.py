"""Decode sessions that send DTMF keys and tones (decode_sessions(tones=True), send_dtmf / send_tones) on the GPU.  Every comparison
is equality.  A session's concatenated audio is held to its wire chain (resample, format, channels) applied, over the whole clip, to
tones.splice(raw, inserts): raw is decode()'s audio for an exact session and, for the session that emits early with a cross-fade,
its audio in a pool built without tones that runs the same script.  That pool is also the reference of the mel pieces, of
frames_emitted, of the session that never sends and of the launch counts."""
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import pcm, tones
from dmel_codec_amd.utils.resample import resample
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

F, UP, RATE = 4, 256, 24000                            # mel frames per token, samples per frame, the vocoder's rate (the tiny codec)
MAX_PUSH = 16
# every profile family of the library: the kernels' own and the per-launch counters of the session pools
FAMILIES = ("tones", "small", "pcm_convert", "crossfade", "stream_fork", "stream_pack", "dtmf", "voice", "conv_igemm", "aa_snake",
            "stft_logmel", "aa_snake_bwd", "conv_wgrad", "train_elementwise")
ALL_KEYS = "0123456789*#ABCD"


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
    def __init__(self, pool, codec, dev, seed, T, **open_kw):
        self.ids, self.noise = clip(codec, seed, T, dev)
        self.slot, self.pos, self.audio, self.mel, self.emitted = pool.open(**open_kw), 0, [], [], []

    def take(self, n):
        a, self.pos = self.pos, self.pos + n
        return self.ids[:, a:self.pos], self.noise[:, F * a:F * self.pos]


# the sessions: 0 exact f32 at the vocoder's rate; 1 s16 stereo at 48 kHz; 2 u-law at 8 kHz; 3 emits at once and cross-fades;
# 4 never sends; 5 s16 at the vocoder's rate, opened late, gets keys and ends without a token
SESSIONS = [(310, 40, {}), (311, 36, dict(output_sample_rate=48000, sample_format="s16", channels=2)),
            (312, 46, dict(output_sample_rate=8000, sample_format="ulaw")), (313, 20, dict(lookahead_frames=0, crossfade_samples=64)),
            (314, 24, {}), (315, 0, dict(sample_format="s16"))]
BEEP = tones.tone_program(1000, 30, RATE, ramp_ms=3)
RING = tones.tone_program([440, 480], 40, RATE, level_dbfs=-16, gap_ms=10)
# ("send", session, program, at_frame | None | "emitted"), ("open", session), (plan, final)
SCRIPT = [({0: 7, 1: 5, 2: 16, 3: 3, 4: 6}, ()),
          ("send", 0, tones.dtmf_program("12", RATE, 40, 30), None),          # a default anchor: frame 28
          ("send", 3, tones.dtmf_program("5", RATE, 40, 30), None),           # behind the fade tail: it waits for the next piece
          ({0: 0, 1: 11, 2: 0, 3: 0, 4: 5}, ()),
          ("send", 1, BEEP, None), ("send", 1, tones.dtmf_program("9#", RATE, 40, 30), 64),   # two requests on one anchor
          ("send", 2, tones.dtmf_program("A0", RATE, 60, 40), None),
          ({0: 16, 1: 9, 2: 9, 3: 5, 4: 0}, ()),
          ("send", 0, RING, 60),                                              # an explicit anchor inside what was received
          ("send", 3, BEEP, None), ("send", 3, RING, None),
          ({0: 1, 1: 11, 2: 5, 3: 8, 4: 13}, (1,)),
          ("open", 5), ("send", 5, tones.dtmf_program("42", RATE, 40, 30), None),
          ({0: 16, 2: 16, 3: 0, 4: 0, 5: 0}, (4, 5)),
          ("send", 2, BEEP, "emitted"),                                       # due at once: a push without tokens serves it
          ("send", 0, tones.dtmf_program("7", RATE, 40, 30), None),           # just before close
          ({0: 0, 2: 0, 3: 4}, (0,)),
          ({2: 0, 3: 0}, (2, 3))]


def run_script(codec, dev, with_tones, park=None):
    """-> dict(ses, inserts {session: [(P, program)]}, steps [dict(delta, served, audio_n, plan, final)], pool); park: (push index,
    pool factory, dict): before that push every open session is parked and restored into the pool the factory builds"""
    pool = codec.decode_sessions(6, max_push_tokens=MAX_PUSH, output_sample_rates=(48000, 8000), early_emit=True, crossfade_samples=64,
                                 tones=with_tones)
    ses = {k: Session(pool, codec, dev, *SESSIONS[k][:2], **SESSIONS[k][2]) for k in range(5)}
    inserts, queue, steps, n_push = {k: [] for k in range(6)}, {k: [] for k in range(6)}, [], 0
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        for item in SCRIPT:
            if item[0] == "open":
                ses[item[1]] = Session(pool, codec, dev, *SESSIONS[item[1]][:2], **SESSIONS[item[1]][2])
                continue
            if item[0] == "send":
                _, k, program, at = item
                s = ses[k].slot
                at = pool.frames_emitted(s) if at == "emitted" else F * ses[k].pos if at is None else at
                queue[k].append((at, tones.length(program)))
                inserts[k].append((at * UP, program))
                if with_tones:
                    assert pool.send_tones(s, program, None if item[3] is None else at) == tones.length(program)
                    assert pool.tones_pending(s) == queue[k]
                continue
            plan, final = item
            if park is not None and n_push == park[0]:
                other, live = park[1](), [k for k in ses if ses[k].slot is not None]
                snaps = pool.park([ses[k].slot for k in live])
                moved, filler = {}, other.open()                            # slot 0 is taken while the sessions arrive: none keeps its index
                for k, s in zip(live[::-1], other.restore([snaps[ses[k].slot] for k in live[::-1]])):       # the last session first
                    moved[k], ses[k].slot = (ses[k].slot, s), s
                other.drop(filler)
                park[2].update(snaps=snaps, home=pool, moved=moved)
                pool = other
            n_push += 1
            ids, noise = {}, {}
            for k, n in plan.items():
                ids[ses[k].slot], noise[ses[k].slot] = ses[k].take(n)
            before = counts()
            out = pool.push(ids, noise=noise, final=[ses[k].slot for k in final])
            after = counts()
            served, audio_n = [], {}
            for k in plan:
                audio, mel = out[ses[k].slot]
                ses[k].audio.append(audio.clone())
                ses[k].mel.append(mel)
                e = sum(m.shape[1] for m in ses[k].mel)
                ses[k].emitted.append(e)
                if k not in final:
                    assert pool.frames_emitted(ses[k].slot) == e
                # the rule, from what the test itself knows: the speech handed out ends at e * up, less the fade tail that waits
                fades = "crossfade_samples" in SESSIONS[k][2]
                h1 = e * UP - (64 if fades and e and k not in final else 0)
                due = [at for at, _ in queue[k] if k in final or at * UP <= h1]
                audio_n[k] = audio.numel()
                if due:
                    served.append(k)
                    del queue[k][:len(due)]
                if with_tones and k not in final:
                    assert pool.tones_pending(ses[k].slot) == queue[k], (k, n_push)
            for k in final:
                ses[k].slot = None
            steps.append(dict(delta={f: after[f] - before[f] for f in FAMILIES}, served=served, audio_n=audio_n, plan=plan, final=final))
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert pool.open_slots == [] and all(not q for q in queue.values())
    return dict(ses=ses, inserts=inserts, steps=steps, pool=pool)


_runs = {}


def runs(codec, dev):
    if not _runs:
        _runs["tones"] = run_script(codec, dev, True)
        _runs["plain"] = run_script(codec, dev, False)
    return _runs


def cat_audio(s):
    return torch.cat([a if a.ndim == 2 and a.shape[0] != 1 else a.reshape(-1) for a in s.audio])


def spliced(raw, inserts, dev):
    return torch.from_numpy(tones.splice(raw.cpu().numpy(), inserts, RATE)).to(dev)


def wire(k, x):
    """the whole-clip wire chain of session k over x (n,) at the vocoder's rate"""
    kw = SESSIONS[k][2]
    rate, fmt, ch = kw.get("output_sample_rate", RATE), kw.get("sample_format", "f32"), kw.get("channels", 1)
    y = resample(x[None], RATE, rate)[0] if rate != RATE else x
    if ch > 1:
        return pcm.fan_out(y, ch, fmt)
    return y if fmt == "f32" else pcm.to_pcm16(y) if fmt == "s16" else pcm.to_g711(y, fmt)


def test_every_session_is_the_wire_chain_over_the_splice(dev, codec):
    r = runs(codec, dev)
    t, p = r["tones"]["ses"], r["plain"]["ses"]
    for k, (seed, T, kw) in enumerate(SESSIONS):
        raw = cat_audio(p[k]) if "lookahead_frames" in kw else decoded(codec, seed, T, dev)[0]
        assert raw.dtype == torch.float32 and raw.shape == (T * F * UP,)
        if not kw:                                                           # an exact f32 session of the plain pool IS decode()
            assert torch.equal(cat_audio(p[k]), raw)
        inserts = r["tones"]["inserts"][k]
        assert (len(inserts) > 0) == (k != 4)
        want = wire(k, spliced(raw, inserts, dev))
        got = cat_audio(t[k])
        assert got.dtype == want.dtype and got.shape == want.shape, (k, got.shape, want.shape)
        assert torch.equal(got, want), f"session {k}: {int((got != want).sum())} of {got.numel()} samples differ"
        # mel pieces and frames_emitted are the plain pool's
        assert t[k].emitted == p[k].emitted and len(t[k].mel) == len(p[k].mel)
        assert all(torch.equal(a, b) for a, b in zip(t[k].mel, p[k].mel))
        assert torch.equal(torch.cat(t[k].mel, dim=1), decoded(codec, seed, T, dev)[1]) or "lookahead_frames" in kw
    # the session that never sends: piece for piece
    assert len(t[4].audio) == len(p[4].audio) and all(torch.equal(a, b) for a, b in zip(t[4].audio, p[4].audio))


def test_one_tone_launch_per_serving_step_and_nothing_else_changes(dev, codec):
    r = runs(codec, dev)
    st, sp = r["tones"]["steps"], r["plain"]["steps"]
    assert len(st) == len(sp) == 7
    bares = []
    for a, b in zip(st, sp):
        assert a["served"] == b["served"]                                    # the test's own rule, from the frames both pools emitted
        assert a["delta"]["tones"] == (1 if a["served"] else 0) and b["delta"]["tones"] == 0, (a, b)
        for f in FAMILIES:
            if f not in ("tones", "small", "pcm_convert"):
                assert a["delta"][f] == b["delta"][f], (f, a, b)
        # the tone launch is one record of "small" as well.  A slot served without a speech piece of its own has audio where the
        # plain pool's has none, and audio takes the launches audio takes: a pool makes ONE resample launch in a step in which a
        # session at another rate gets samples, and ONE convert launch in a step in which a session with a wire format or channels
        # does; each is one record of "small", the convert launch one of "pcm_convert" too.  Both follow from the audio each pool
        # returned in the step, so the difference is known exactly
        def launches(step, option):
            return int(any(step["audio_n"][k] and option(SESSIONS[k][2]) for k in step["plan"]))
        resamples = [launches(x, lambda kw: "output_sample_rate" in kw) for x in (a, b)]
        converts = [launches(x, lambda kw: "sample_format" in kw or "channels" in kw) for x in (a, b)]
        bare = any(b["audio_n"][k] == 0 for k in a["served"])
        bares.append(bare)
        assert a["delta"]["pcm_convert"] == converts[0] and b["delta"]["pcm_convert"] == converts[1], (a, b)
        assert a["delta"]["small"] - b["delta"]["small"] == a["delta"]["tones"] + resamples[0] - resamples[1] + converts[0] - converts[1], (a, b)
        if not bare:                                                         # every served slot had speech: no launch but the tone launch
            assert resamples[0] == resamples[1] and converts[0] == converts[1], (a, b)
    assert sum(bool(a["served"]) for a in st) >= 4 and not st[0]["served"] and not st[1]["served"]
    assert any(set(a["served"]) - set(a["final"]) for a in st) and any(bares)
    plain, pool = r["plain"]["pool"], r["tones"]["pool"]
    assert not any(k.startswith("tone") for k in plain.buf) and plain.allocated_bytes() < pool.allocated_bytes()
    assert tuple(pool.buf["tone_stage"].shape) == (6, pool.cap * UP + 2 * RATE) and pool.buf["tone_sine"].shape == (RATE,)
    assert pool.rs.max_push == pool.cap * UP + 2 * RATE and plain.rs.max_push == plain.cap * UP and pool.cap == plain.cap


def test_park_with_pending_requests_and_restore_elsewhere(dev, codec):
    r = runs(codec, dev)
    info = {}
    moved = run_script(codec, dev, True, park=(3, lambda: codec.decode_sessions(
        8, max_push_tokens=24, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64, tones=True), info))
    snaps = info["snaps"]
    # another number of slots, another max_push_tokens, and every session with requests in another slot than it left
    assert moved["pool"].S == 8 != info["home"].S and moved["pool"].max_push == 24 != info["home"].max_push
    assert len(info["moved"]) == 5 and all(was != now for was, now in info["moved"].values())
    assert tuple(moved["pool"].buf["tone_stage"].shape) == (8, moved["pool"].cap * UP + 2 * RATE)
    assert sum(len(sn.meta["tones"]) for sn in snaps.values()) >= 5 and info["home"].open_slots == []
    assert all(sn.meta["tone_samples"] == sum(tones.length(p) for _, p in sn.meta["tones"]) for sn in snaps.values())
    for k in range(6):
        a, b = moved["ses"][k], r["tones"]["ses"][k]
        assert len(a.audio) == len(b.audio) and all(torch.equal(x, y) for x, y in zip(a.audio, b.audio)), k
        assert all(torch.equal(x, y) for x, y in zip(a.mel, b.mel)) and a.emitted == b.emitted
    # a pool without tones refuses the snapshots that carry requests and takes no slot; it takes the one that carries none
    bare = codec.decode_sessions(6, max_push_tokens=24, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64)
    with_requests = [sn for sn in snaps.values() if sn.meta["tones"]]
    for sn in with_requests:
        with pytest.raises(ValueError, match="tones=True"):
            bare.restore([sn])
    with pytest.raises(ValueError, match="tones=True"):
        bare.restore(snaps)
    assert bare.open_slots == []
    none = [sn for sn in snaps.values() if not sn.meta["tones"]]
    assert none and bare.restore(none) == list(range(len(none)))
    small = codec.decode_sessions(6, max_push_tokens=24, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64,
                                  tones=True, max_tone_samples=100)
    with pytest.raises(ValueError, match="max_tone_samples"):
        small.restore(with_requests[:1])
    assert small.open_slots == []


def listen(dev, audio, **open_kw):
    """the keys an encode session with a DTMF detector hears in `audio` (its wire's dtype, at its wire's rate)"""
    enc = make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)
    pool = enc.encode_sessions(1, max_push_samples=7680, sample_rates=(8000,), dtmf=True)
    s = pool.open(dtmf=True, **open_kw)
    for a in range(0, audio.shape[0], 7680):
        pool.push({s: audio[a:a + 7680]})
    return pool.dtmf()[s].digits


def talk(codec, dev, **open_kw):
    pool = codec.decode_sessions(1, max_push_tokens=MAX_PUSH, output_sample_rates=(8000,), tones=True, max_tone_samples=3 * RATE)
    s = pool.open(**open_kw)
    ids, noise = clip(codec, 320, 6, dev)
    first = pool.push({s: ids}, noise={s: noise})[s][0]
    assert pool.send_dtmf(s, ALL_KEYS) == 16 * 3840 and pool.send_dtmf(s, "1")
    return torch.cat([first, pool.close(s)[0]], dim=1)[0]


def test_round_trip_into_a_listening_session(dev, codec):
    audio = talk(codec, dev)
    assert audio.dtype == torch.float32 and audio.shape == (6 * F * UP + 17 * 3840,)
    assert listen(dev, audio) == ALL_KEYS + "1"


def test_round_trip_through_the_ulaw_8k_wire(dev, codec):
    audio = talk(codec, dev, output_sample_rate=8000, sample_format="ulaw")
    assert audio.dtype == torch.uint8 and audio.shape == ((6 * F * UP + 17 * 3840) // 3,)
    assert listen(dev, audio, sample_rate=8000, sample_format="ulaw") == ALL_KEYS + "1"
