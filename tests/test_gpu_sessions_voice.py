"""Encode sessions with voice detection (EncodeSessions(voice=True), open(voice=)) on the GPU.  Every comparison is equality: after
every step, pool.voice() is the report of the host rule (utils/voice.py: scan) run over the whole-clip transform's mel up to the
session's frames, and voice_frames() the matching slice of its flags and counts; the ids are those of the same script in a pool
without the option; the detector costs exactly one launch in every step in which a session with detection received frames."""
import math

import pytest
import torch

from dmel_codec_amd.utils import pcm, voice
from dmel_codec_amd.utils.voice import VoiceConfig
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR, HOP = 24000, 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


def make_clip(seconds, noise_dbfs, bursts, seed, rate=SR):
    """white noise at noise_dbfs (None: digital silence) with the 20-harmonic burst of 150 Hz over each [a, b) s of `bursts`"""
    g = torch.Generator().manual_seed(seed)
    n = int(seconds * rate)
    x = torch.zeros(n) if noise_dbfs is None else torch.randn(n, generator=g) * 10.0 ** (noise_dbfs / 20.0)
    t = torch.arange(n, dtype=torch.float64) / rate
    tone = sum(torch.sin(2 * math.pi * 150 * k * t) / k for k in range(1, 21)) * 0.1
    for a, b in bursts:
        x = x + torch.where((t >= a) & (t < b), tone, torch.zeros_like(tone)).float()
    return x


class Launches:
    """the profile counters of the block, read behind every step"""
    FAMILIES = ("voice", "small", "stft_logmel", "conv_igemm")

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


# session -> (clip, open(voice=), push sizes (cycled)); each ends with its clip, so they end in different steps
SESSIONS = {"burst": (dict(seconds=1.9, noise_dbfs=-40, bursts=[(0.4, 0.9)], seed=1), VoiceConfig(release_frames=20), [7680, 100, 0, 7680]),
            "noise": (dict(seconds=1.3, noise_dbfs=-30, bursts=[], seed=2), True, [0, 7680, 100, 7680, 7680]),
            "late": (dict(seconds=1.1, noise_dbfs=None, bursts=[(0.5, 1.1)], seed=3), VoiceConfig(bands=(0, 60), min_bands=3), [100, 7680, 7680, 0]),
            "plain": (dict(seconds=1.3, noise_dbfs=-30, bursts=[], seed=2), None, [7680, 0, 100])}
_run = {}


def script_run(codec, dev, with_voice):
    """all sessions of SESSIONS in one pool, step by step -> per session: ids pieces, reports, frame slices; the launches per step"""
    pool = codec.encode_sessions(slots=5, max_push_samples=7680, voice=with_voice)
    clips = {k: make_clip(**SESSIONS[k][0]).to(dev) for k in SESSIONS}
    slot = {k: pool.open(voice=SESSIONS[k][1] if with_voice else None) for k in SESSIONS}
    st = {k: dict(pos=0, i=0, ids=[], reports=[], pieces=[], done=False) for k in SESSIONS}
    steps = []
    with Launches() as ln:
        before = ln.read()
        while not all(s["done"] for s in st.values()):
            named, final = {}, []
            for k, s in st.items():
                if s["done"]:
                    continue
                sizes, total = SESSIONS[k][2], clips[k].shape[0]
                n = min(sizes[s["i"] % len(sizes)], total - s["pos"])
                named[k] = clips[k][s["pos"]:s["pos"] + n]
                s["pos"], s["i"] = s["pos"] + n, s["i"] + 1
                if s["pos"] == total:
                    final.append(k)
            out = pool.push({slot[k]: x for k, x in named.items()}, final=[slot[k] for k in final])
            after = ln.read()
            reports = pool.voice()
            for k in named:
                st[k]["ids"].append(out[slot[k]])
                if with_voice and SESSIONS[k][1] is not None:
                    st[k]["reports"].append(reports[slot[k]])
                    st[k]["pieces"].append(tuple(t.cpu() for t in pool.voice_frames(slot[k])))
            if with_voice:                                                  # who reports: sessions with detection, open or just ended
                live = {slot[k] for k, s in st.items() if SESSIONS[k][1] is not None and (not s["done"])}
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
        _run.update(voice=script_run(codec, dev, True), plain=script_run(codec, dev, False))
    return _run


@pytest.mark.parametrize("session", [k for k in SESSIONS if SESSIONS[k][1] is not None])
def test_reports_equal_the_host_scan_of_the_whole_clip_mel_after_every_step(dev, codec, session):
    r = runs(codec, dev)["voice"]
    s, clip = r["st"][session], r["clips"][session]
    cfg = voice.as_config(SESSIONS[session][1])
    mel = codec.encode_mel_transform(clip[None])[0].cpu().contiguous()     # the whole clip's frames: the session's are their bits
    assert mel.shape == (80, clip.shape[0] // HOP)
    state, at = voice.fresh_state(80), 0
    for j, (rep, (flags, counts)) in enumerate(zip(s["reports"], s["pieces"])):
        assert at <= rep.frames <= mel.shape[1], (session, j)
        state, f, c = voice.scan(mel[:, at:rep.frames].contiguous(), cfg, state)
        assert rep == voice.report(state, HOP, SR), (session, j, rep, voice.report(state, HOP, SR))
        assert flags.dtype == torch.uint8 and torch.equal(flags, f) and torch.equal(counts, c), (session, j)
        at = rep.frames
    assert at == mel.shape[1] and len(s["reports"]) >= 4                    # the final push flushed the last frames
    assert any(a.frames == b.frames for a, b in zip(s["reports"], s["reports"][1:]))       # a step without a frame: the report stands
    last = s["reports"][-1]
    if session == "burst":                                                  # 0.4 s is frame 37.5, 0.9 s frame 84.4; 4 = n_fft / hop
        assert last.starts == 1 and last.end_of_turn and abs(last.speech_start - 37) <= 4 and abs(last.speech_end - 84) <= 4
        assert last.silence_frames == last.frames - last.speech_end and any(x.speaking for x in s["reports"])
        assert last.samples(last.speech_start) == last.speech_start * HOP and last.seconds(last.frames) == last.frames * HOP / SR
    elif session == "noise":
        assert last.starts == 0 and not last.end_of_turn and last.speech_start is None
    else:                                                                   # it ends while it speaks
        assert last.starts == 1 and last.speaking and not last.end_of_turn and abs(last.speech_start - 47) <= 4


def test_ids_are_those_of_a_pool_without_detection(dev, codec):
    r = runs(codec, dev)
    for k in SESSIONS:
        a, b = r["voice"]["st"][k]["ids"], r["plain"]["st"][k]["ids"]
        assert len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)), k
        clip = r["voice"]["clips"][k]
        ids, lens = codec.encode(clip[None], torch.tensor([clip.shape[0]], device=dev))
        assert torch.equal(torch.cat(a, dim=1), ids[0, :, :int(lens[0])]), k


def test_one_more_launch_per_step_that_has_frames_and_none_without_the_option(dev, codec):
    r = runs(codec, dev)
    assert len(r["voice"]["steps"]) == len(r["plain"]["steps"]) >= 6
    frames = {k: 0 for k in SESSIONS}
    idx = {k: 0 for k in SESSIONS}
    with_frames = 0
    for sv, sp in zip(r["voice"]["steps"], r["plain"]["steps"]):
        assert sv["named"] == sp["named"]
        new = 0
        for k in sv["named"]:
            if SESSIONS[k][1] is not None:
                rep = r["voice"]["st"][k]["reports"][idx[k]]
                new += rep.frames - frames[k]
                frames[k], idx[k] = rep.frames, idx[k] + 1
        expect = 1 if new else 0
        with_frames += expect
        assert sv["delta"]["voice"] == expect and sp["delta"]["voice"] == 0, (sv, sp)
        # everything else is what the pool without the option launches ("small" carries the detector's own record too)
        assert sv["delta"]["small"] == sp["delta"]["small"] + expect, (sv, sp)
        assert sv["delta"]["stft_logmel"] == sp["delta"]["stft_logmel"] and sv["delta"]["conv_igemm"] == sp["delta"]["conv_igemm"], (sv, sp)
    assert 0 < with_frames < len(r["voice"]["steps"])                       # both kinds of step occurred
    assert "voice" not in r["plain"]["pool"].buf and r["plain"]["pool"].allocated_bytes() < r["voice"]["pool"].allocated_bytes()


def test_a_48k_s16_stereo_session_equals_the_scan_of_the_mel_encode_sees(dev, codec):
    left = make_clip(1.0, -40, [(0.3, 0.7)], 11, rate=48000)
    right = make_clip(1.0, -40, [(0.35, 0.7)], 12, rate=48000)
    clip = (torch.stack([left, right], dim=1) * 32768).round().clamp(-32768, 32767).to(torch.int16).to(dev)
    mono = pcm.downmix(clip, "s16")
    mel = codec.encode_mel_transform(mono[None], sample_rate=48000)[0].cpu().contiguous()
    cfg = VoiceConfig(release_frames=12)
    pool = codec.encode_sessions(slots=2, max_push_samples=7000, sample_rates=(48000,), voice=True)
    s = pool.open(sample_rate=48000, sample_format="s16", channels=2, voice=cfg)
    t = pool.open()                                                         # a neighbour without detection, pushed to at the end
    state, at, got, pos = voice.fresh_state(80), 0, [], 0
    sizes = [7000, 100, 0, 7000]
    j = 0
    while pos < clip.shape[0]:
        n = min(sizes[j % len(sizes)], clip.shape[0] - pos)
        pos, j = pos + n, j + 1
        got.append(pool.push({s: clip[pos - n:pos]}, final=(s,) if pos == clip.shape[0] else ())[s])
        rep = pool.voice()[s]
        flags, counts = pool.voice_frames(s)
        state, f, c = voice.scan(mel[:, at:rep.frames].contiguous(), cfg, state)
        assert rep == voice.report(state, HOP, SR) and torch.equal(flags.cpu(), f) and torch.equal(counts.cpu(), c), j
        at = rep.frames
    assert at == mel.shape[1] and rep.starts == 1 and rep.end_of_turn
    ids, lens = codec.encode(mono[None], torch.tensor([mono.shape[0]], device=dev), sample_rate=48000)
    assert torch.equal(torch.cat(got, dim=1), ids[0, :, :int(lens[0])])
    assert pool.voice() == {s: rep}                                         # ended in the most recent push: still reported
    pool.push({t: mono[:100]})
    assert pool.voice() == {}                                               # and no longer after the next one


def test_a_session_parked_while_it_speaks_goes_on_in_another_pool(dev, codec):
    clip = make_clip(1.6, -40, [(0.3, 1.0)], 21).to(dev)
    cfg = VoiceConfig(release_frames=15, bands=(2, 78))
    home = codec.encode_sessions(slots=3, max_push_samples=4096, voice=True)
    away = codec.encode_sessions(slots=2, max_push_samples=7680, voice=True)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    assert home.cap != away.cap
    stay, move = home.open(voice=cfg), home.open(voice=cfg)
    other = away.open(voice=True)                                           # a neighbour, so that the target has buffers and history
    away.push({other: clip[:3000]})
    where, slot, moved_at = home, move, None
    for j, a in enumerate(range(0, clip.shape[0], 3000)):
        piece, last = clip[a:a + 3000], a + 3000 >= clip.shape[0]
        fin = lambda s: (s,) if last else ()
        if where is home:
            out = home.push({stay: piece, slot: piece}, final=fin(stay) + fin(slot))
            ids = (out[stay], out[slot])
            reps = home.voice()
            reps, frames = (reps[stay], reps[slot]), (home.voice_frames(stay), home.voice_frames(slot))
        else:
            ids = (home.push({stay: piece}, final=fin(stay))[stay], away.push({slot: piece}, final=fin(slot))[slot])
            reps, frames = (home.voice()[stay], away.voice()[slot]), (home.voice_frames(stay), away.voice_frames(slot))
        assert torch.equal(ids[0], ids[1]) and reps[0] == reps[1], (j, reps)
        assert torch.equal(frames[0][0], frames[1][0]) and torch.equal(frames[0][1], frames[1][1]), j
        if where is home and reps[1].speaking and not last:                 # park it mid-speech, once
            snap = home.park([slot])[slot]
            assert snap.meta["voice"] == cfg.as_dict() and snap.meta["layout"][-1][:3] == ["voice", 1, 88]
            home.buf["voice"][slot] = 0x7F7F7F7F
            away.buf["voice"][1 - other] = 0x7F7F7F7F                       # the free row it lands in is no zeroed one
            with pytest.raises(ValueError, match="voice=True"):
                bare.restore([snap])
            assert bare.open_slots == []
            [slot] = away.restore([snap.cpu().to(dev)])
            assert away.voice()[slot] == reps[1] and away.voice_frames(slot)[0].numel() == 0      # the state came along; the step's bytes did not
            where, moved_at = away, j
    assert moved_at is not None and reps[0].end_of_turn and reps[0].starts == 1 and reps[0].frames == clip.shape[0] // HOP
    # a session without detection in the voice pool: its snapshot is the one of a pool without the option, byte for byte
    a, b = home.open(), bare.open()
    home.push({a: clip[:4096]}), bare.push({b: clip[:4096]})
    sa, sb = home.snapshot([a])[a], bare.snapshot([b])[b]
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob) and "voice" not in sa.meta
