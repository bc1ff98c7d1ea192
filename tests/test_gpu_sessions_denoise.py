"""Encode sessions with a noise suppressor (EncodeSessions(denoise=True), open(denoise=)) on the GPU.  Every comparison is equality:
the ids of a denoising session are those of encode() of the host rule's output (utils/denoise.py: scan) over the codec-rate samples
the whole-clip path produces for the session's wire; after every step pool.denoised() is the report of the host state up to the
session's samples and denoise_frames() the matching slice of the host's frame powers; sessions without a suppressor, in the same pool
or in a pool without the option, keep the ids of encode(); the suppressor costs exactly one launch in every step in which a denoising
session gained samples; DTMF reports do not change, the leveller and the voice detector see the suppressed samples, the rules of all
options compose in the order of the launches, and the state travels with snapshot / restore."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import conceal, denoise, echo, level, pcm, voice
from dmel_codec_amd.utils.denoise import DenoiseConfig
from dmel_codec_amd.utils.level import LevelConfig
from dmel_codec_amd.utils.resample import resample
from dmel_codec_amd.utils.voice import VoiceConfig
from test_dtmf_cpu import keyed_clip
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR = 24000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


class Launches:
    """the profile counters of the block, read behind every step"""
    FAMILIES = ("denoise", "level", "dtmf", "voice", "small", "stft_logmel", "conv_igemm")

    def __enter__(self):
        from dmel_codec_amd import _lib
        self._lib = _lib
        _lib.prof_reset(); _lib.prof_enable(True)
        return self

    def read(self):
        torch.cuda.synchronize()
        return {f: self._lib.prof_read(f)["launches"] for f in self.FAMILIES}

    def __exit__(self, *exc):
        self._lib.prof_enable(False); self._lib.prof_reset()


def noisy_clip(rate, seed, scale=1.0):
    """0.7 s at `rate`: noise from the first sample, a tone in it from 0.3 s on, a quieter stretch at the end"""
    rng = np.random.default_rng(seed)
    n = rate * 7 // 10
    t = np.arange(n) / rate
    x = 0.02 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t) * (t >= 0.3) * (1.0 - 0.7 * (t >= 0.55))
    return (scale * x).astype(np.float32)


# session -> (wire rate, format, channels, open(denoise=), push sizes in the wire's samples (cycled)); index 2 of every denoising
# session's sizes is 0, so that one step gives no suppressor a sample; each ends with its clip, in different steps
SESSIONS = {"f32": (24000, "f32", 1, True, [5000, 101, 0, 3000]),
            "s16": (8000, "s16", 1, DenoiseConfig(frame_samples=256, learn_frames=5, alpha=0.9, floor_gain=0.2), [2500, 100, 0, 1700, 2560]),
            "ulaw": (8000, "ulaw", 1, DenoiseConfig(frame_samples=64, learn_frames=8), [2000, 37, 0, 1500]),
            "plain": (24000, "f32", 1, None, [7680, 0, 100])}
_run = {}


def wire_clip(name, dev):
    """-> (what the session is pushed, the mono f32 clip at the wire's rate encode() takes, the codec-rate samples on the host)"""
    rate, fmt, ch, _, _ = SESSIONS[name]
    x = torch.from_numpy(noisy_clip(rate, len(name) + rate)).to(dev)
    if fmt == "s16":
        wire = (x * 32768).round().clamp(-32768, 32767).to(torch.int16)
        mono = pcm.from_pcm16(wire)
    elif fmt == "ulaw":
        wire = pcm.to_g711(x, "ulaw")
        mono = pcm.from_g711(wire, "ulaw")
    else:
        wire = mono = x
    return wire, mono, resample(mono[None], rate, SR)[0].cpu().contiguous()


def script_run(codec, dev, with_denoise):
    """all sessions of SESSIONS in one pool, step by step -> per session: ids pieces, reports, frame slices; the launches per step"""
    pool = codec.encode_sessions(slots=5, max_push_samples=7680, sample_rates=(8000,), denoise=with_denoise)
    clips = {k: wire_clip(k, dev) for k in SESSIONS}
    slot = {k: pool.open(sample_rate=v[0], sample_format=v[1], channels=v[2], denoise=v[3] if with_denoise else None)
            for k, v in SESSIONS.items()}
    st = {k: dict(pos=0, i=0, ids=[], reports=[], pieces=[], done=False) for k in SESSIONS}
    steps = []
    with Launches() as ln:
        before = ln.read()
        while not all(s["done"] for s in st.values()):
            named, final = {}, []
            for k, s in st.items():
                if s["done"]:
                    continue
                sizes, total = SESSIONS[k][4], clips[k][0].shape[0]
                n = min(sizes[s["i"] % len(sizes)], total - s["pos"])
                named[k] = clips[k][0][s["pos"]:s["pos"] + n]
                s["pos"], s["i"] = s["pos"] + n, s["i"] + 1
                if s["pos"] == total:
                    final.append(k)
            out = pool.push({slot[k]: x for k, x in named.items()}, final=[slot[k] for k in final])
            after = ln.read()
            reports = pool.denoised()
            for k in named:
                st[k]["ids"].append(out[slot[k]])
                if with_denoise and SESSIONS[k][3] is not None:
                    st[k]["reports"].append(reports[slot[k]])
                    st[k]["pieces"].append(tuple(t.cpu() for t in pool.denoise_frames(slot[k])))
            if with_denoise:                                                # who reports: sessions with a suppressor, open or just ended
                live = {slot[k] for k, s in st.items() if SESSIONS[k][3] is not None and (not s["done"])}
                assert set(reports) == live, (set(reports), live)
            else:
                assert reports == {}
            for k in final:
                st[k]["done"] = True
            steps.append(dict(named=list(named), delta={f: after[f] - before[f] for f in after}))
            before = after
    assert pool.open_slots == []
    return dict(st=st, steps=steps, clips=clips, pool=pool)


def runs(codec, dev):
    if not _run:
        _run.update(denoise=script_run(codec, dev, True), plain=script_run(codec, dev, False))
    return _run


def encode_of(codec, dev, x, **kw):
    ids, lens = codec.encode(x.to(dev)[None], torch.tensor([x.shape[0]], device=dev), **kw)
    return ids[0, :, :int(lens[0])]


@pytest.mark.parametrize("session", [k for k in SESSIONS if SESSIONS[k][3] is not None])
def test_ids_reports_and_frames_equal_the_host_rule_on_the_codec_rate_clip(dev, codec, session):
    r = runs(codec, dev)["denoise"]
    s, ref = r["st"][session], r["clips"][session][2]
    cfg = denoise.as_config(SESSIONS[session][3])
    N = cfg.frame_samples
    y, whole, _, _ = denoise.scan(ref, cfg)
    assert torch.equal(torch.cat(s["ids"], dim=1), encode_of(codec, dev, y)), session
    state, at = denoise.fresh_state(), 0
    for j, (rep, (pin, pout)) in enumerate(zip(s["reports"], s["pieces"])):
        assert at <= rep.total_samples <= ref.shape[0], (session, j)
        _, state, p, q = denoise.scan(ref[at:rep.total_samples], cfg, state)
        want = denoise.report(state, N, SR, cfg.learn_frames)
        assert rep == want, (session, j, rep, want)
        assert pin.dtype == torch.float32 and torch.equal(pin, p) and torch.equal(pout, q), (session, j)
        at = rep.total_samples
    assert at == ref.shape[0] and len(s["reports"]) >= 4 and torch.equal(state, whole)      # the final push flushed the resampler
    assert any(a.total_samples == b.total_samples for a, b in zip(s["reports"], s["reports"][1:]))   # a step without a sample
    last = s["reports"][-1]
    assert not last.learning and last.frames == ref.shape[0] // (N // 2) and last.delay_samples == N
    assert 0.0 < last.power_out < last.power_in                             # no gain exceeds 1, and the noise bins lie below it
    assert not torch.equal(y, ref) and not y[:N].any()                      # the suppressor did something, and delays by N


def test_sessions_without_a_suppressor_keep_the_ids_of_encode(dev, codec):
    r = runs(codec, dev)
    for k in SESSIONS:
        mono = r["plain"]["clips"][k][1]
        kw = {} if SESSIONS[k][0] == SR else dict(sample_rate=SESSIONS[k][0])
        ids = encode_of(codec, dev, mono, **kw)
        assert torch.equal(torch.cat(r["plain"]["st"][k]["ids"], dim=1), ids), k               # a pool built without the option
        same = torch.equal(torch.cat(r["denoise"]["st"][k]["ids"], dim=1), ids)
        assert same == (SESSIONS[k][3] is None), k                          # in the denoising pool: only the session without one


def test_one_more_launch_per_step_that_gained_samples_and_none_without_the_option(dev, codec):
    r = runs(codec, dev)
    assert len(r["denoise"]["steps"]) == len(r["plain"]["steps"]) >= 6
    samples = {k: 0 for k in SESSIONS}
    idx = {k: 0 for k in SESSIONS}
    with_samples = 0
    for sv, sp in zip(r["denoise"]["steps"], r["plain"]["steps"]):
        assert sv["named"] == sp["named"]
        new = 0
        for k in sv["named"]:
            if SESSIONS[k][3] is not None:
                rep = r["denoise"]["st"][k]["reports"][idx[k]]
                new += rep.total_samples - samples[k]
                samples[k], idx[k] = rep.total_samples, idx[k] + 1
        expect = 1 if new else 0
        with_samples += expect
        assert sv["delta"]["denoise"] == expect and sp["delta"]["denoise"] == 0, (sv, sp)
        # everything else is what the pool without the option launches ("small" carries the suppressor's own record too)
        assert sv["delta"]["small"] == sp["delta"]["small"] + expect, (sv, sp)
        assert all(sv["delta"][f] == sp["delta"][f] for f in ("level", "dtmf", "voice", "stft_logmel", "conv_igemm")), (sv, sp)
    assert 0 < with_samples < len(r["denoise"]["steps"])                    # both kinds of step occurred
    plain, with_rows = r["plain"]["pool"], r["denoise"]["pool"]
    assert not any(k.startswith("denoise") for k in plain.buf) and plain.allocated_bytes() < with_rows.allocated_bytes()
    assert tuple(with_rows.buf["denoise"].shape) == (5, 3092) and with_rows.buf["denoise_in"].shape == with_rows.buf["denoise_out"].shape == \
        (5, with_rows.codec_push // 32 + 2)


def test_every_option_together_composes_the_host_rules_in_the_order_of_the_launches(dev, codec):
    """conceal -> echo -> DTMF -> denoise -> level -> STFT -> voice on one f32 session: the DTMF reports are those of the same pool
    without the suppressor, the ids those of encode() of level(denoise(echo(conceal(x)))), the voice flags those of that clip's mel"""
    rng = np.random.default_rng(9)
    x = keyed_clip(SR, 307, [6, 1, 12], rng)
    x = (x + 0.01 * rng.standard_normal(x.shape[0])).astype(np.float32)
    far = (0.2 * rng.standard_normal(x.shape[0])).astype(np.float32)
    x[200:] += 0.3 * far[:-200]                                               # an echo of the far end, 200 samples late
    dcfg, vcfg = DenoiseConfig(frame_samples=256, learn_frames=6), VoiceConfig(release_frames=10)
    opts = dict(voice=vcfg, dtmf=True, level=True, echo=True, conceal=True)
    every = codec.encode_sessions(slots=2, max_push_samples=7680, denoise=True, **{k: True for k in opts})
    without = codec.encode_sessions(slots=2, max_push_samples=7680, **{k: True for k in opts})
    a, b = every.open(denoise=dcfg, **opts), without.open(**opts)
    lost_at = {1: 480}                                                        # push 1 is preceded by 480 lost samples
    xd, fd = torch.from_numpy(x).to(dev), torch.from_numpy(far).to(dev)
    ids, flags, counts, cuts, ranges, at, j = [], [], [], [], [], 0, 0
    while at < x.shape[0]:
        gap = lost_at.get(j, 0)
        n = min(1500, x.shape[0] - at - gap)
        if gap:
            ranges.append((at, at + gap))
        lo, hi = at, at + gap + n
        fin = hi >= x.shape[0]
        kw = dict(far={a: fd[lo:hi]}, lost={a: gap} if gap else None)
        ids.append(every.push({a: xd[lo + gap:hi]}, final=(a,) if fin else (), **kw)[a])
        without.push({b: xd[lo + gap:hi]}, final=(b,) if fin else (), far={b: fd[lo:hi]}, lost={b: gap} if gap else None)
        assert every.dtmf()[a] == without.dtmf()[b]                         # the detector's reports do not change with denoise
        assert all(torch.equal(u, v) for u, v in zip(every.dtmf_blocks(a), without.dtmf_blocks(b)))
        f, c = every.voice_frames(a)
        flags.append(f.cpu()), counts.append(c.cpu())
        cuts.append((lo, hi))
        at, j = hi, j + 1
    assert every.dtmf()[a].digits and len(cuts) >= 3
    x0 = x.copy()
    for lo, hi in ranges:
        x0[lo:hi] = 0.0
    y1 = conceal.scan(x0, ranges, conceal.ConcealConfig(), None, SR)[0]
    state, parts = None, []
    for lo, hi in cuts:                                                      # the canceller's steps: the far chunk, then the microphone chunk
        e, state, _, _ = echo.scan(y1[lo:hi], far[lo:hi], echo.EchoConfig(), state)
        parts.append(e)
    y2 = torch.cat(parts)
    y3, dstate, _, _ = denoise.scan(y2, dcfg)
    y4 = level.scan(y3, LevelConfig(), None, SR)[0]
    assert not torch.equal(y3, y2) and not torch.equal(y4, y3)
    assert torch.equal(torch.cat(ids, dim=1), encode_of(codec, dev, y4))
    mel = codec.encode_mel_transform(y4.to(dev)[None])[0].cpu().contiguous()
    _, f, c = voice.scan(mel, vcfg, voice.fresh_state(80))
    assert torch.equal(torch.cat(flags), f) and torch.equal(torch.cat(counts), c)
    assert every.denoised() == {a: denoise.report(dstate, 256, SR, 6)}
    assert every.levels()[a] == level.report(level.scan(y3, LevelConfig(), None, SR)[1], 240, SR)


def test_a_session_parked_mid_hop_goes_on_in_another_slot_of_a_pool_of_another_size(dev, codec):
    x = torch.from_numpy(noisy_clip(SR, 21)).to(dev)
    cfg = DenoiseConfig(learn_frames=4)
    home = codec.encode_sessions(slots=3, max_push_samples=4096, denoise=True)
    away = codec.encode_sessions(slots=2, max_push_samples=7680, denoise=True)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    stay, move = home.open(denoise=cfg), home.open(denoise=cfg)
    other = away.open(denoise=True)                                         # a neighbour, so that the target has buffers and history
    away.push({other: x[:3000]})
    where, slot, moved_at, got = home, move, None, []
    for j, a in enumerate(range(0, x.shape[0], 1500)):                      # 1500 = 5 * 256 + 220: every cut lies inside a hop
        piece, last = x[a:a + 1500], a + 1500 >= x.shape[0]
        fin = lambda s: (s,) if last else ()
        if where is home:
            out = home.push({stay: piece, slot: piece}, final=fin(stay) + fin(slot))
            ids = (out[stay], out[slot])
            reps = home.denoised()
            reps, frames = (reps[stay], reps[slot]), (home.denoise_frames(stay), home.denoise_frames(slot))
        else:
            ids = (home.push({stay: piece}, final=fin(stay))[stay], away.push({slot: piece}, final=fin(slot))[slot])
            reps, frames = (home.denoised()[stay], away.denoised()[slot]), (home.denoise_frames(stay), away.denoise_frames(slot))
        got.append(ids[1])
        assert torch.equal(ids[0], ids[1]) and reps[0] == reps[1], (j, reps)
        assert torch.equal(frames[0][0], frames[1][0]) and torch.equal(frames[0][1], frames[1][1]), j
        if where is home and j == 2:                                        # park it mid-hop, behind the learning frames
            assert not reps[1].learning and reps[1].total_samples % 256 == 148
            snap = home.park([slot])[slot]
            assert snap.meta["denoise"] == cfg.as_dict() and snap.meta["layout"][-1][:3] == ["denoise", 1, 3092]
            home.buf["denoise"][slot] = 0x7F7F7F7F
            away.buf["denoise"][1 - other] = 0x7F7F7F7F                     # the free row it lands in is no zeroed one
            with pytest.raises(ValueError, match="denoise=True"):
                bare.restore([snap])
            assert bare.open_slots == []
            [slot] = away.restore([snap.cpu().to(dev)])
            assert away.denoised()[slot] == reps[1] and away.denoise_frames(slot)[0].numel() == 0   # the state came along; the step's words did not
            where, moved_at = away, j
    assert moved_at == 2 and reps[0].total_samples == x.shape[0]
    y, state, _, _ = denoise.scan(x.cpu(), cfg)
    assert reps[1] == denoise.report(state, 512, SR, 4) and torch.equal(torch.cat(got, dim=1), encode_of(codec, dev, y))
    # a session without a suppressor in the denoising pool: its snapshot is the one of a pool without the option, byte for byte
    a, b = home.open(), bare.open()
    home.push({a: x[:4096]}), bare.push({b: x[:4096]})
    sa, sb = home.snapshot([a])[a], bare.snapshot([b])[b]
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob) and "denoise" not in sa.meta


def test_refusals(dev, codec):
    x = torch.from_numpy(noisy_clip(SR, 3)).to(dev)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, denoise=True)
    with pytest.raises(ValueError, match="denoise=True"):
        bare.open(denoise=True)
    with pytest.raises(ValueError):
        pool.open(denoise="yes")
    with pytest.raises(ValueError):
        codec.encode_sessions(slots=2, denoise=DenoiseConfig())
    assert bare.open_slots == [] and pool.open_slots == []
    s = pool.open(denoise=True)
    pool.push({s: x[:1000]})
    snap = pool.snapshot([s])[s]
    with pytest.raises(ValueError, match="denoise=True"):
        bare.restore([snap])
    assert bare.open_slots == []
    with pytest.raises(ValueError, match="suppressor"):
        bare.denoise_frames(0)
    # the launch itself: tensors of the wrong kind are refused before the C entry
    t = denoise.transform_table().to(dev)
    rows = torch.zeros(1, 600, device=dev)
    state = torch.zeros(1, denoise.STATE_WORDS, dtype=torch.int32, device=dev)
    out = torch.zeros(1, 8, device=dev)
    for kw in (dict(state=state[:, :16].contiguous()), dict(transform=t[:100].contiguous()), dict(power_out=torch.zeros(1, 9, device=dev)),
               dict(n_new=[601]), dict(configs=[None]), dict(power_in=torch.zeros(1, 1, device=dev), power_out=torch.zeros(1, 1, device=dev))):
        args = dict(samples=rows, first=[0], n_new=[600], configs=[DenoiseConfig()], state=state, power_in=out, power_out=out.clone(),
                    transform=t)
        args.update(kw)
        with pytest.raises((ValueError, RuntimeError)):
            denoise.denoise_items(**args)
    assert not state.any() and not rows.any()
