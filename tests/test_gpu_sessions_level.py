"""Encode sessions with an input leveller (EncodeSessions(level=True), open(level=)) on the GPU.  Every comparison is equality: the ids
of a levelled session are those of encode() of the host rule's output (utils/level.py: scan) over the codec-rate samples the
whole-clip path produces for the session's wire; after every step pool.levels() is the report of the host state up to the session's
samples and level_blocks() the matching slice of the host's block outputs; sessions without a leveller, in the same pool or in a pool
without the option, keep the ids of encode(); the leveller costs exactly one launch in every step in which a levelled session gained
samples; DTMF reports do not change, the voice detector sees the levelled mel, and the state travels with snapshot / restore."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import level, pcm, voice
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
    FAMILIES = ("level", "dtmf", "voice", "small", "stft_logmel", "conv_igemm")

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


def level_clip(rate, seed, scale=1.0):
    """0.56 s at `rate`: silence, a quiet stretch, a loud one (which the gain of the quiet one drives into the ceiling), silence, a
    stretch in between -- a tone in noise each"""
    rng = np.random.default_rng(seed)
    parts = []
    for ms, amp in ((30, 0.0), (180, 0.02), (140, 0.6), (60, 0.0), (150, 0.1)):
        n = rate * ms // 1000
        t = np.arange(n) / rate
        parts.append(amp * (0.7 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * rng.standard_normal(n)))
    return (scale * np.concatenate(parts)).astype(np.float32)


# session -> (wire rate, format, channels, open(level=), push sizes in the wire's samples (cycled)); index 2 of every levelled
# session's sizes is 0, so that one step gives no leveller a sample; each ends with its clip, in different steps
SESSIONS = {"f32": (24000, "f32", 1, True, [5000, 101, 0, 3000]),
            "s16st": (48000, "s16", 2, LevelConfig(block_samples=100, target_peak=0.3, release=0.1), [7000, 100, 0, 7000, 7680]),
            "ulaw": (8000, "ulaw", 1, True, [2000, 37, 0, 1500]),
            "plain": (24000, "f32", 1, None, [7680, 0, 100])}
_run = {}


def wire_clip(name, dev):
    """-> (what the session is pushed, the mono f32 clip at the wire's rate encode() takes, the codec-rate samples on the host)"""
    rate, fmt, ch, _, _ = SESSIONS[name]
    x = torch.from_numpy(level_clip(rate, len(name) + rate)).to(dev)
    if fmt == "s16":
        wire = (torch.stack([x, 0.8 * x], dim=1) * 32768).round().clamp(-32768, 32767).to(torch.int16)
        mono = pcm.downmix(wire, "s16")
    elif fmt == "ulaw":
        wire = pcm.to_g711(x, "ulaw")
        mono = pcm.from_g711(wire, "ulaw")
    else:
        wire = mono = x
    return wire, mono, resample(mono[None], rate, SR)[0].cpu().contiguous()


def script_run(codec, dev, with_level):
    """all sessions of SESSIONS in one pool, step by step -> per session: ids pieces, reports, block slices; the launches per step"""
    pool = codec.encode_sessions(slots=5, max_push_samples=7680, sample_rates=(48000, 8000), level=with_level)
    clips = {k: wire_clip(k, dev) for k in SESSIONS}
    slot = {k: pool.open(sample_rate=v[0], sample_format=v[1], channels=v[2], level=v[3] if with_level else None) for k, v in SESSIONS.items()}
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
            reports = pool.levels()
            for k in named:
                st[k]["ids"].append(out[slot[k]])
                if with_level and SESSIONS[k][3] is not None:
                    st[k]["reports"].append(reports[slot[k]])
                    st[k]["pieces"].append(tuple(t.cpu() for t in pool.level_blocks(slot[k])))
            if with_level:                                                  # who reports: sessions with a leveller, open or just ended
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
        _run.update(level=script_run(codec, dev, True), plain=script_run(codec, dev, False))
    return _run


def encode_of(codec, dev, x, **kw):
    ids, lens = codec.encode(x.to(dev)[None], torch.tensor([x.shape[0]], device=dev), **kw)
    return ids[0, :, :int(lens[0])]


@pytest.mark.parametrize("session", [k for k in SESSIONS if SESSIONS[k][3] is not None])
def test_ids_reports_and_blocks_equal_the_host_rule_on_the_codec_rate_clip(dev, codec, session):
    r = runs(codec, dev)["level"]
    s, ref = r["st"][session], r["clips"][session][2]
    cfg = level.as_config(SESSIONS[session][3])
    N = cfg.block(SR)
    y, whole, _, _ = level.scan(ref, cfg, None, SR)
    assert torch.equal(torch.cat(s["ids"], dim=1), encode_of(codec, dev, y)), session
    state, at = level.fresh_state(), 0
    for j, (rep, (peaks, gains)) in enumerate(zip(s["reports"], s["pieces"])):
        assert at <= rep.total_samples <= ref.shape[0], (session, j)
        _, state, p, g = level.scan(ref[at:rep.total_samples], cfg, state, SR)
        assert rep == level.report(state, N, SR, cfg.initial_gain), (session, j, rep, level.report(state, N, SR, cfg.initial_gain))
        assert peaks.dtype == torch.float32 and torch.equal(peaks, p) and torch.equal(gains, g), (session, j)
        at = rep.total_samples
    assert at == ref.shape[0] and len(s["reports"]) >= 4 and torch.equal(state, whole)      # the final push flushed the resampler
    assert any(a.total_samples == b.total_samples for a, b in zip(s["reports"], s["reports"][1:]))   # a step without a sample
    last = s["reports"][-1]
    assert last.locked and last.blocks == ref.shape[0] // N and last.clamped > 0 and last.held_blocks > 0 and last.peak_out <= 1.0
    assert not torch.equal(y, ref)                                          # the leveller did something


def test_sessions_without_a_leveller_keep_the_ids_of_encode(dev, codec):
    r = runs(codec, dev)
    for k in SESSIONS:
        mono = r["plain"]["clips"][k][1]
        kw = {} if SESSIONS[k][0] == SR else dict(sample_rate=SESSIONS[k][0])
        ids = encode_of(codec, dev, mono, **kw)
        assert torch.equal(torch.cat(r["plain"]["st"][k]["ids"], dim=1), ids), k               # a pool built without the option
        same = torch.equal(torch.cat(r["level"]["st"][k]["ids"], dim=1), ids)
        assert same == (SESSIONS[k][3] is None), k                          # in the level pool: only the session without one


def test_one_more_launch_per_step_that_gained_samples_and_none_without_the_option(dev, codec):
    r = runs(codec, dev)
    assert len(r["level"]["steps"]) == len(r["plain"]["steps"]) >= 6
    samples = {k: 0 for k in SESSIONS}
    idx = {k: 0 for k in SESSIONS}
    with_samples = 0
    for sv, sp in zip(r["level"]["steps"], r["plain"]["steps"]):
        assert sv["named"] == sp["named"]
        new = 0
        for k in sv["named"]:
            if SESSIONS[k][3] is not None:
                rep = r["level"]["st"][k]["reports"][idx[k]]
                new += rep.total_samples - samples[k]
                samples[k], idx[k] = rep.total_samples, idx[k] + 1
        expect = 1 if new else 0
        with_samples += expect
        assert sv["delta"]["level"] == expect and sp["delta"]["level"] == 0, (sv, sp)
        # everything else is what the pool without the option launches ("small" carries the leveller's own record too)
        assert sv["delta"]["small"] == sp["delta"]["small"] + expect, (sv, sp)
        assert all(sv["delta"][f] == sp["delta"][f] for f in ("dtmf", "voice", "stft_logmel", "conv_igemm")), (sv, sp)
    assert 0 < with_samples < len(r["level"]["steps"])                      # both kinds of step occurred
    plain, with_rows = r["plain"]["pool"], r["level"]["pool"]
    assert not any(k.startswith("level") for k in plain.buf) and plain.allocated_bytes() < with_rows.allocated_bytes()
    assert tuple(with_rows.buf["level"].shape) == (5, 16) and with_rows.buf["level_peak"].shape == with_rows.buf["level_gain"].shape == \
        (5, with_rows.codec_push // 32 + 2)


def test_dtmf_reads_the_samples_as_received_and_voice_the_levelled_mel(dev, codec):
    x = torch.from_numpy(keyed_clip(SR, 307, [6, 1, 12], np.random.default_rng(9))).to(dev)
    y = level.scan(x.cpu(), LevelConfig(), None, SR)[0]
    assert not torch.equal(y, x.cpu())
    vcfg = VoiceConfig(release_frames=10)
    every = codec.encode_sessions(slots=2, max_push_samples=7680, voice=True, dtmf=True, level=True)
    only_d = codec.encode_sessions(slots=2, max_push_samples=7680, dtmf=True)
    a, b = every.open(voice=vcfg, dtmf=True, level=True), only_d.open(dtmf=True)
    t = every.open()                                                        # a neighbour without options, pushed to at the end
    ids, flags, counts = [], [], []
    for at in range(0, x.shape[0], 5000):
        piece, fin = x[at:at + 5000], at + 5000 >= x.shape[0]
        ids.append(every.push({a: piece}, final=(a,) if fin else ())[a])
        only_d.push({b: piece}, final=(b,) if fin else ())
        assert every.dtmf()[a] == only_d.dtmf()[b]                          # the detector's reports do not change with level
        assert all(torch.equal(u, v) for u, v in zip(every.dtmf_blocks(a), only_d.dtmf_blocks(b)))
        f, c = every.voice_frames(a)
        flags.append(f.cpu()), counts.append(c.cpu())
    assert every.dtmf()[a].digits == "62*" and torch.equal(torch.cat(ids, dim=1), encode_of(codec, dev, y))
    mel = codec.encode_mel_transform(y.to(dev)[None])[0].cpu().contiguous()  # the mel of the LEVELLED clip
    state, f, c = voice.scan(mel, vcfg, voice.fresh_state(80))
    assert torch.equal(torch.cat(flags), f) and torch.equal(torch.cat(counts), c)
    assert every.voice()[a] == voice.report(state, codec.encode_mel_transform.hop_length, SR)
    rep = every.levels()[a]
    assert rep == level.report(level.scan(x.cpu(), LevelConfig(), None, SR)[1], 240, SR) and every.levels() == {a: rep}
    every.push({t: x[:100]})
    assert every.levels() == {}                                             # ended two pushes ago: no longer reported


def test_a_session_parked_mid_block_goes_on_in_a_pool_of_another_size(dev, codec):
    x = torch.from_numpy(level_clip(SR, 21)).to(dev)
    cfg = LevelConfig(release=0.2)
    home = codec.encode_sessions(slots=3, max_push_samples=4096, level=True)
    away = codec.encode_sessions(slots=2, max_push_samples=7680, level=True)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    stay, move = home.open(level=cfg), home.open(level=cfg)
    other = away.open(level=True)                                           # a neighbour, so that the target has buffers and history
    away.push({other: x[:3000]})
    where, slot, moved_at, got = home, move, None, []
    for j, a in enumerate(range(0, x.shape[0], 1500)):                      # 1500 = 6 * 240 + 60: every cut lies inside a block
        piece, last = x[a:a + 1500], a + 1500 >= x.shape[0]
        fin = lambda s: (s,) if last else ()
        if where is home:
            out = home.push({stay: piece, slot: piece}, final=fin(stay) + fin(slot))
            ids = (out[stay], out[slot])
            reps = home.levels()
            reps, blocks = (reps[stay], reps[slot]), (home.level_blocks(stay), home.level_blocks(slot))
        else:
            ids = (home.push({stay: piece}, final=fin(stay))[stay], away.push({slot: piece}, final=fin(slot))[slot])
            reps, blocks = (home.levels()[stay], away.levels()[slot]), (home.level_blocks(stay), away.level_blocks(slot))
        got.append(ids[1])
        assert torch.equal(ids[0], ids[1]) and reps[0] == reps[1], (j, reps)
        assert torch.equal(blocks[0][0], blocks[1][0]) and torch.equal(blocks[0][1], blocks[1][1]), j
        if where is home and j == 2:                                        # park it mid-block, locked, with a gain that is moving
            assert reps[1].locked and reps[1].total_samples % 240 == 180
            snap = home.park([slot])[slot]
            assert snap.meta["level"] == cfg.as_dict() and snap.meta["layout"][-1][:3] == ["level", 1, 16]
            home.buf["level"][slot] = 0x7F7F7F7F
            away.buf["level"][1 - other] = 0x7F7F7F7F                       # the free row it lands in is no zeroed one
            with pytest.raises(ValueError, match="level=True"):
                bare.restore([snap])
            assert bare.open_slots == []
            [slot] = away.restore([snap.cpu().to(dev)])
            assert away.levels()[slot] == reps[1] and away.level_blocks(slot)[0].numel() == 0   # the state came along; the step's words did not
            where, moved_at = away, j
    assert moved_at == 2 and reps[0].total_samples == x.shape[0]
    y, state, _, _ = level.scan(x.cpu(), cfg, None, SR)
    assert reps[1] == level.report(state, 240, SR) and torch.equal(torch.cat(got, dim=1), encode_of(codec, dev, y))
    # a session without a leveller in the level pool: its snapshot is the one of a pool without the option, byte for byte
    a, b = home.open(), bare.open()
    home.push({a: x[:4096]}), bare.push({b: x[:4096]})
    sa, sb = home.snapshot([a])[a], bare.snapshot([b])[b]
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob) and "level" not in sa.meta
