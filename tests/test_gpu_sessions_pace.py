"""Decode sessions that pace their replies (decode_sessions(pace=True), open(pace=), set_pace) on the GPU.  Every comparison is
equality.  A pacing session's concatenated audio is held to its wire chain (resample, format, channels) applied, over the whole clip,
to pace.scan(raw, requests, config, final=True) -- and to shape.scan of that where the session also shapes: raw is decode()'s audio
for an exact session and, for a session that emits early with a cross-fade, its audio in a pool built without the option that runs the
same script.  That pool is also the reference of the mel pieces, of frames_emitted, of the session that does not pace and of the
launch counts."""
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import pace, pcm, shape
from dmel_codec_amd.utils.pace import PaceConfig
from dmel_codec_amd.utils.resample import resample
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

F, UP, RATE = 4, 256, 24000                            # mel frames per token, samples per frame, the vocoder's rate (the tiny codec)
MAX_PUSH = 16
FAMILIES = ("pace", "shape", "tones", "small", "pcm_convert", "crossfade", "stream_fork", "stream_pack", "conv_igemm", "aa_snake")


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
    """decode()'s audio (n,) of the whole clip on the device, computed once"""
    if (seed, T) not in _decoded:
        ids, noise = clip(codec, seed, T, dev)
        out = codec.decode(ids[None].contiguous(), torch.tensor([T], device=dev), return_audios=True, noise=noise[None].contiguous())
        _decoded[seed, T] = out[0][0, 0].clone()
    return _decoded[seed, T]


def counts():
    torch.cuda.synchronize()
    return {f: _lib.prof_read(f)["launches"] for f in FAMILIES}


# the sessions: 0 f32 at the vocoder's rate; 1 s16 stereo at 48 kHz with a short hop; 2 u-law at 8 kHz; 3 emits at once and cross-fades;
# 4 paces and shapes, with a gain request and a stop; 5 does not pace and leaves at 8 kHz; 6 paces at 1000: the plain audio
SHORT = PaceConfig(hop_ms=5.0, search_ms=3.0, initial_permille=800)
SESSIONS = [(510, 72, {}, True), (511, 58, dict(output_sample_rate=48000, sample_format="s16", channels=2), SHORT),
            (512, 66, dict(output_sample_rate=8000, sample_format="ulaw"), True),
            (513, 20, dict(lookahead_frames=0, crossfade_samples=64), True), (514, 15, {}, True),
            (515, 20, dict(output_sample_rate=8000), None), (516, 18, dict(sample_format="s16"), True)]
# ("pace", session, permille, None | samples beyond now), ("gain", session, dB), ("stop", session), (plan, final)
# An exact session of this codec hands out its first frame with its 33rd token (geo.hold_frames = 131): sessions 0 .. 2 speak from the
# third push on, and the requests behind it fall into the middle of their replies
SCRIPT = [("pace", 0, 1250, None), ("pace", 2, 700, None), ("pace", 3, 1500, None), ("pace", 4, 1300, None), ("pace", 0, 600, 3000),
          ({0: 16, 1: 16, 2: 16, 3: 3, 4: 6, 5: 6, 6: 10}, ()),
          ("pace", 1, 1900, 2000), ("pace", 3, 550, None), ("gain", 4, -6.0),
          ({0: 16, 1: 16, 2: 16, 3: 6, 4: 9, 5: 5, 6: 0}, ()),
          ("pace", 3, 1000, 1), ("stop", 4),
          ({0: 16, 1: 16, 2: 16, 3: 5, 5: 0, 6: 8}, (6,)),
          ("pace", 0, 2000, 500), ("pace", 2, 1111, None), ("pace", 1, 650, None),
          ({0: 16, 1: 10, 2: 13, 3: 6, 5: 9}, (1,)),
          ({0: 8, 2: 5, 3: 0, 5: 0}, (0, 2, 3, 5))]
OTHER_CUT = [({0: 16, 1: 2, 2: 1, 3: 11}, ()), ({0: 16, 1: 16, 2: 16, 3: 0}, ()), ({0: 16, 1: 16, 2: 16, 3: 9}, (3,)),
             ({0: 16, 1: 16, 2: 16}, ()), ({0: 8, 1: 8, 2: 16}, (0, 1)), ({2: 1}, (2,))]


def cfg_of(k):
    c = SESSIONS[k][3]
    return PaceConfig() if c is True else c


def build(codec, pacing, slots=8):
    return codec.decode_sessions(slots, max_push_tokens=MAX_PUSH, output_sample_rates=(48000, 8000), early_emit=True, crossfade_samples=64,
                                 shape=True, **(dict(pace=True) if pacing else {}))


class Session:
    def __init__(self, pool, codec, dev, k, pacing):
        seed, T, kw, cfg = SESSIONS[k]
        self.ids, self.noise = clip(codec, seed, T, dev)
        extra = dict(pace=cfg) if pacing and cfg is not None else {}
        if pacing and k == 4:
            extra["shape"] = True
        self.slot, self.pos, self.audio, self.mel, self.emitted = pool.open(**kw, **extra), 0, [], [], []

    def take(self, n):
        a, self.pos = self.pos, self.pos + n
        return self.ids[:, a:self.pos], self.noise[:, F * a:F * self.pos]


def run_script(codec, dev, pacing, script=SCRIPT, members=range(7), upfront=None, park=None):
    """-> dict(ses, requests {session: [(P, permille)]}, gains, ends, steps, pool).  upfront: {session: requests} made before the first
    push instead of the script's; park: (push index, pool factory, dict): before that push every open session is parked and restored
    into the pool the factory builds"""
    pool = build(codec, pacing)
    ses = {k: Session(pool, codec, dev, k, pacing) for k in members}
    requests, gains, ends, steps, n_push = {k: [] for k in members}, {4: []}, {}, [], 0
    for k, reqs in (upfront or {}).items():
        for P, permille in reqs:
            assert pool.set_pace(ses[k].slot, permille, P) == P
            requests[k].append((P, permille))
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        for item in script:
            if item[0] == "pace":
                _, k, permille, ahead = item
                if pacing and upfront is None and k in ses:
                    now = pool.pace_fed(ses[k].slot)
                    at = pool.set_pace(ses[k].slot, permille, None if ahead is None else now + ahead)
                    assert at == now + (ahead or 0)
                    requests[k].append((at, permille))
                continue
            if item[0] == "gain":
                if pacing:
                    at = pool.set_gain(ses[item[1]].slot, item[2], 20.0)
                    assert at == pool.samples_fed(ses[item[1]].slot)
                    gains[4].append((at, 10.0 ** (item[2] / 20.0), 480))
                continue
            if item[0] == "stop":
                s = ses[item[1]].slot
                if pacing:
                    now = pool.samples_fed(s)
                    gains[4].append((now, 0.0, 480))
                    ends[4] = now + 480
                    audio, mel = pool.stop(s, 20.0)
                else:
                    audio, mel = pool.close(s)
                assert s not in pool.open_slots
                ses[item[1]].audio.append(audio.clone()), ses[item[1]].mel.append(mel)
                ses[item[1]].slot = None
                continue
            plan, final = item
            if park is not None and n_push == park[0]:
                other, live = park[1](), [k for k in ses if ses[k].slot is not None]
                snaps = pool.park([ses[k].slot for k in live])
                filler = other.open()                                         # slot 0 is taken while the sessions arrive: none keeps its index
                for k, s in zip(live[::-1], other.restore([snaps[ses[k].slot] for k in live[::-1]])):
                    ses[k].slot = s
                other.drop(filler)
                park[2].update(snaps=snaps, home=pool)
                pool = other
            n_push += 1
            ids, noise = {}, {}
            for k, n in plan.items():
                ids[ses[k].slot], noise[ses[k].slot] = ses[k].take(n)
            pacers = [k for k in plan if pacing and SESSIONS[k][3] is not None]
            fed = {k: pool.pace_fed(ses[k].slot) for k in pacers}
            before = counts()
            out = pool.push(ids, noise=noise, final=[ses[k].slot for k in final])
            after = counts()
            served = [k for k in pacers if k in final or pool.pace_fed(ses[k].slot) > fed[k]]
            reports = pool.paced() if pacing else {}
            audio_n = {}
            for k in plan:
                audio, mel = out[ses[k].slot]
                ses[k].audio.append(audio.clone())
                ses[k].mel.append(mel)
                ses[k].emitted.append(sum(m.shape[1] for m in ses[k].mel))
                audio_n[k] = audio.numel()
                if k not in final:
                    assert pool.frames_emitted(ses[k].slot) == ses[k].emitted[-1]
                    if k in pacers:
                        rep, (H, D) = reports[ses[k].slot], cfg_of(k).samples(RATE)
                        assert rep.samples_in == pool.pace_fed(ses[k].slot) and rep.frames == pool.pints[ses[k].slot][0]
                        assert rep.frames == rep.natural + rep.searched + rep.quiet
                        off, sc = pool.pace_frames(ses[k].slot)
                        assert off.dtype == torch.int32 and off.shape == sc.shape and int(off.abs().max() if off.numel() else 0) <= D
            for k in final:
                ses[k].slot = None
            steps.append(dict(delta={f: after[f] - before[f] for f in FAMILIES}, served=served, audio_n=audio_n, plan=plan, final=final))
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert pool.open_slots == []
    return dict(ses=ses, requests=requests, gains=gains, ends=ends, steps=steps, pool=pool)


_runs = {}


def runs(codec, dev):
    if not _runs:
        _runs["pace"] = run_script(codec, dev, True)
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


def raw_of(k, codec, dev):
    seed, T, kw, _ = SESSIONS[k]
    if "lookahead_frames" not in kw:
        return decoded(codec, seed, T, dev)
    early = cat_audio(runs(codec, dev)["plain"]["ses"][k])                    # f32 at the vocoder's rate in the plain pool
    assert early.dtype == torch.float32 and early.shape == (T * F * UP,)
    return early


def expected(r, k, codec, dev):
    """the contract sentence for session k of the run r"""
    y = pace.scan(raw_of(k, codec, dev).cpu().numpy(), r["requests"][k], cfg_of(k), RATE, final=True)[0]
    if k == 4:
        y = shape.scan(y, r["gains"][4], shape.ShapeConfig(), RATE, end=r["ends"].get(4), final=True)[0]
    return wire(k, y.to(dev))


def test_every_pacing_session_is_the_wire_chain_over_the_scan(dev, codec):
    r = runs(codec, dev)
    t, p = r["pace"]["ses"], r["plain"]["ses"]
    for k, (seed, T, kw, cfg) in enumerate(SESSIONS):
        got = cat_audio(t[k])
        if cfg is None:                                                      # the session that does not pace: piece for piece
            assert len(t[k].audio) == len(p[k].audio) and all(torch.equal(a, b) for a, b in zip(t[k].audio, p[k].audio))
        else:
            want = expected(r["pace"], k, codec, dev)
            assert got.dtype == want.dtype and got.shape == want.shape, (k, got.shape, want.shape)
            assert torch.equal(got, want), f"session {k}: {int((got != want).sum())} of {got.numel()} samples differ"
        # mel pieces and frames_emitted are the plain pool's
        assert t[k].emitted == p[k].emitted and len(t[k].mel) == len(p[k].mel)
        assert all(torch.equal(a, b) for a, b in zip(t[k].mel, p[k].mel))
    # the rates took hold: session 0 speaks faster, then slower, then twice as fast; session 2 slower; both differ from the plain audio
    assert len(r["pace"]["requests"][0]) == 3 and len(r["pace"]["requests"][3]) == 3 and r["pace"]["requests"][2][1][0] > 0
    assert cat_audio(t[2]).shape[0] != cat_audio(p[2]).shape[0] and cat_audio(t[1]).shape[0] != cat_audio(p[1]).shape[0]
    # rate 1000 is the plain session's audio
    assert torch.equal(cat_audio(t[6]), cat_audio(p[6])) and cat_audio(t[6]).dtype == torch.int16
    # the stop ends the PACED stream at E
    assert cat_audio(t[4]).shape[0] == r["pace"]["ends"][4] and float(cat_audio(t[4])[-1].abs()) < 1e-4


def test_another_cut_of_the_same_tokens_gives_the_same_bits(dev, codec):
    r = runs(codec, dev)["pace"]
    again = run_script(codec, dev, True, script=OTHER_CUT, members=range(4), upfront={k: r["requests"][k] for k in range(4)})
    for k in range(3):                                                       # the exact sessions: the same stream however it was cut
        assert torch.equal(cat_audio(again["ses"][k]), cat_audio(r["ses"][k])), k
    # the early session's stream depends on its cuts (what it decoded ahead): held to the contract on its own plain run
    plain = run_script(codec, dev, False, script=OTHER_CUT, members=range(4))
    raw = cat_audio(plain["ses"][3])
    want = pace.scan(raw.cpu().numpy(), again["requests"][3], cfg_of(3), RATE, final=True)[0].to(dev)
    assert torch.equal(cat_audio(again["ses"][3]), want)


def test_one_pace_launch_per_serving_step_and_nothing_else_changes(dev, codec):
    r = runs(codec, dev)
    st, sp = r["pace"]["steps"], r["plain"]["steps"]
    assert len(st) == len(sp) == 5
    for a, b in zip(st, sp):
        assert a["delta"]["pace"] == (1 if a["served"] else 0) and b["delta"]["pace"] == 0, (a, b)
        for f in ("tones", "crossfade", "stream_fork", "stream_pack", "conv_igemm", "aa_snake"):
            assert a["delta"][f] == b["delta"][f], (f, a, b)
    assert all(a["served"] for a in st)
    # a step of the pace pool that serves no pacing slot shows the plain pool's records, family by family, and so does a pool built
    # without the option: it has no pace buffers and sizes what it sized
    pool, bare = build(codec, True, 2), build(codec, False, 2)
    ids, noise = clip(codec, 515, 20, dev)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        deltas, audio = [], []
        for q in (pool, bare):
            s = q.open(output_sample_rate=8000, sample_format="s16")
            before = counts()
            a1 = q.push({s: ids[:, :16]}, noise={s: noise[:, :64]})[s][0]
            a2 = q.push({s: ids[:, 16:]}, noise={s: noise[:, 64:]}, final=(s,))[s][0]
            after = counts()
            deltas.append({f: after[f] - before[f] for f in FAMILIES})
            audio.append((a1.clone(), a2.clone()))
        assert deltas[0] == deltas[1] and deltas[0]["pace"] == 0
        assert all(torch.equal(x, y) for x, y in zip(*audio))
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert not any(k.startswith("pace") for k in bare.buf) and bare.allocated_bytes() < pool.allocated_bytes()
    assert bare.chain_w == bare.cap * UP and pool.chain_w == pace.max_out(pool.cap * UP + 64, 512, 512)


def test_park_mid_reply_into_another_pool_and_a_branch(dev, codec):
    r, info = runs(codec, dev), {}
    moved = run_script(codec, dev, True, park=(3, lambda: codec.decode_sessions(
        11, max_push_tokens=MAX_PUSH, output_sample_rates=(8000, 48000), early_emit=True, crossfade_samples=64, shape=True, pace=True), info))
    snaps = info["snaps"]
    pacing = [sn for sn in snaps.values() if "pace" in sn.meta]
    assert len(pacing) == 4 and len(snaps) == 5 and info["home"].open_slots == []
    assert all(sn.meta["layout"][-1][:3] == ["pace", 1, PaceConfig.from_dict(sn.meta["pace"]).state_words(RATE)] for sn in pacing
               if sn.meta["pace_ints"][3])
    assert any(sn.meta["pace_requests"] for sn in pacing) and sum(sn.meta["pace_ints"][0] > 0 for sn in pacing) >= 3
    for k in range(7):
        a, b = moved["ses"][k], r["pace"]["ses"][k]
        assert len(a.audio) == len(b.audio) and all(torch.equal(x, y) for x, y in zip(a.audio, b.audio)), k
        assert all(torch.equal(x, y) for x, y in zip(a.mel, b.mel)) and a.emitted == b.emitted
    # a pool without the option refuses the snapshot of a pacing session and takes no slot
    plain = build(codec, False, 4)
    for sn in pacing:
        with pytest.raises(ValueError, match="pace=True"):
            plain.restore([sn])
    assert plain.open_slots == []
    # a branch: two continuations of one snapshot, both the uninterrupted session, piece for piece
    ids, noise = clip(codec, 510, 30, dev)

    def reply(pool, branch):
        s = pool.open(pace=True, lookahead_frames=0)                         # emits at once: its pacer is in the middle of its stream
        pool.set_pace(s, 1400)
        first = pool.push({s: ids[:, :14]}, noise={s: noise[:, :56]})[s][0].clone()
        assert pool.pace_fed(s) > 0 and pool.paced()[s].searched > 0
        slots = [s]
        if branch:
            snap = pool.snapshot([s])[s]
            slots.append(pool.restore([snap])[0])
            assert pool.pace_fed(slots[1]) == pool.pace_fed(s) and pool.paced()[slots[1]] == pool.paced()[s]
        at = {pool.set_pace(q, 800) for q in slots}
        assert at == {pool.pace_fed(s)}
        out = pool.push({q: ids[:, 14:] for q in slots}, noise={q: noise[:, 56:] for q in slots}, final=slots)
        if branch:
            late = pool.restore([snap])[0]                                   # the snapshot outlives its session; dropped, it leaves no trace
            pool.drop(late)
            assert pool.open_slots == [] and pool.pcfg[late] is None and pool.preq[late] == []
        return first, [out[q][0] for q in slots]

    first, (alone,) = reply(build(codec, True, 3), False)
    again, (one, two) = reply(build(codec, True, 3), True)
    assert torch.equal(first, again) and torch.equal(one, alone) and torch.equal(two, alone) and alone.shape[1] > 0


def test_a_tone_beside_a_pacing_session_places_the_paced_piece(dev, codec):
    """where the tone launch of a step places the resampler's chunks behind their tails, the paced piece is among them"""
    ids, noise = clip(codec, 512, 40, dev)

    def reply(tones_on):
        pool = codec.decode_sessions(2, max_push_tokens=MAX_PUSH, output_sample_rates=(8000,), early_emit=True, pace=True,
                                     **(dict(tones=True) if tones_on else {}))
        a, b = pool.open(output_sample_rate=8000, pace=True, lookahead_frames=0), pool.open(output_sample_rate=8000, lookahead_frames=0)
        pool.set_pace(a, 1300)
        got = []
        for j, (lo, hi) in enumerate(((0, 16), (16, 32), (32, 40))):
            if tones_on and j == 1:
                assert pool.send_dtmf(b, "5") > 0                             # due in this step: slot b leaves at 8 kHz, the step is placed
            out = pool.push({q: ids[:, lo:hi] for q in (a, b)}, noise={q: noise[:, 4 * lo:4 * hi] for q in (a, b)}, final=(a, b) if hi == 40 else ())
            got.append(out[a][0].clone())
        return torch.cat(got, 1)

    with_tone, without = reply(True), reply(False)
    assert torch.equal(with_tone, without) and with_tone.shape[1] > 0


def test_refusals_on_a_live_pool(dev, codec):
    bare = build(codec, False, 2)
    with pytest.raises(ValueError, match="pace=True"):
        bare.open(pace=True)
    b0 = bare.open()
    for call in (lambda: bare.set_pace(b0, 1200), lambda: bare.paced(), lambda: bare.pace_frames(b0), lambda: bare.pace_fed(b0)):
        with pytest.raises(ValueError, match="pace=True"):
            call()
    assert bare.open_slots == [b0]
    with pytest.raises(ValueError, match="return_audios"):
        codec.decode_sessions(2, max_push_tokens=MAX_PUSH, return_audios=False, pace=True)
    with pytest.raises(ValueError, match="bool"):
        codec.decode_sessions(2, max_push_tokens=MAX_PUSH, pace=PaceConfig())
    pool = codec.decode_sessions(3, max_push_tokens=MAX_PUSH, early_emit=True, tones=True, pace=True)
    with pytest.raises(ValueError, match="hop"):
        pool.open(pace=PaceConfig(hop_ms=1.0))
    with pytest.raises(ValueError, match="PaceConfig"):
        pool.open(pace=1250)
    assert pool.open_slots == []
    a, b = pool.open(pace=True, lookahead_frames=0), pool.open()             # a session that emits at once: its pacer has samples
    ids, noise = clip(codec, 515, 20, dev)
    pool.push({a: ids[:, :16], b: ids[:, :16]}, noise={a: noise[:, :64], b: noise[:, :64]})
    fed = pool.pace_fed(a)
    assert fed > 0 and pool.paced()[a].samples_in == fed and list(pool.paced()) == [a]
    for call, match in ((lambda: pool.set_pace(a, 1200, at_sample=fed - 1), "not in front of"), (lambda: pool.set_pace(a, 499), "permille"),
                        (lambda: pool.set_pace(a, 2001), "permille"), (lambda: pool.set_pace(a, 1200.0), "permille"),
                        (lambda: pool.set_pace(b, 1200), "without pace="), (lambda: pool.pace_frames(b), "without pace="),
                        (lambda: pool.pace_fed(b), "without pace="), (lambda: pool.send_dtmf(a, "1"), "paces its reply"),
                        (lambda: pool.send_tones(a, [(1000, 0, 0.5, 0.0, 480, 0, 0)]), "paces its reply")):
        with pytest.raises(ValueError, match=match):
            call()
    assert pool.preq[a] == [] and pool.tq[a] == []
    assert pool.set_pace(a, 1500, fed + 100) == fed + 100
    with pytest.raises(ValueError, match="not in front of"):
        pool.set_pace(a, 900, fed + 99)                                     # in front of an earlier request
    for i in range(7):
        pool.set_pace(a, 900 + i, fed + 100 + i)
    with pytest.raises(ValueError, match="ninth"):
        pool.set_pace(a, 1000, fed + 1000)
    assert len(pool.preq[a]) == 8 and pool.send_dtmf(b, "1") > 0             # the session beside it sends its tones
    audio, mel = pool.close(a)
    assert audio.shape[1] > 0 and pool.open_slots == [b]
    with pytest.raises(RuntimeError):
        pool.set_pace(a, 1000)
    pool.drop(b)
