"""Encode sessions with DTMF detection (EncodeSessions(dtmf=True), open(dtmf=)) on the GPU.  Every comparison is equality: after every
step, pool.dtmf() is the report of the host rule (utils/dtmf.py: scan) run over the codec-rate samples the whole-clip path produces
for the session's wire, up to the session's samples, and dtmf_blocks() the matching slice of its bytes; the ids are those of the
same script in a pool without the option and those of encode(); the detector costs exactly one launch in every step in which a
session with a detector gained samples; the state travels with snapshot / restore."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import dtmf, pcm
from dmel_codec_amd.utils.dtmf import DtmfConfig
from dmel_codec_amd.utils.resample import resample
from dmel_codec_amd.utils.voice import VoiceConfig
from test_dtmf_cpu import keyed_clip
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR, N = 24000, 307


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


class Launches:
    """the profile counters of the block, read behind every step"""
    FAMILIES = ("dtmf", "voice", "small", "stft_logmel", "conv_igemm")

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


# session -> (wire rate, format, channels, keys played, open(dtmf=), push sizes in the wire's samples (cycled)); index 2 of every
# detector session's sizes is 0, so that one step gives no detector a sample; each ends with its clip, in different steps
SESSIONS = {"f32": (24000, "f32", 1, [1, 4, 9, 13, 15, 2, 7], True, [5000, 100, 0, 3000]),
            "s16st": (48000, "s16", 2, [0, 5, 10, 12, 3], DtmfConfig(misses=3), [7000, 100, 0, 7000, 7680]),
            "ulaw": (8000, "ulaw", 1, [14, 8, 6, 11], True, [2000, 37, 0, 2560]),
            "plain": (24000, "f32", 1, [3, 3], None, [7680, 0, 100])}
_run = {}


def wire_clip(name, dev):
    """-> (what the session is pushed, the mono f32 clip at the wire's rate encode() takes, the codec-rate samples on the host)"""
    rate, fmt, ch, keys, _, _ = SESSIONS[name]
    x = torch.from_numpy(keyed_clip(rate, N * rate // SR, keys, np.random.default_rng(len(name) + rate))).to(dev)
    if fmt == "s16":
        wire = (torch.stack([x, 0.8 * x], dim=1) * 32768).round().clamp(-32768, 32767).to(torch.int16)
        mono = pcm.downmix(wire, "s16")
    elif fmt == "ulaw":
        wire = pcm.to_g711(x, "ulaw")
        mono = pcm.from_g711(wire, "ulaw")
    else:
        wire = mono = x
    return wire, mono, resample(mono[None], rate, SR)[0].cpu().contiguous()


def script_run(codec, dev, with_dtmf):
    """all sessions of SESSIONS in one pool, step by step -> per session: ids pieces, reports, block slices; the launches per step"""
    pool = codec.encode_sessions(slots=5, max_push_samples=7680, sample_rates=(48000, 8000), dtmf=with_dtmf)
    clips = {k: wire_clip(k, dev) for k in SESSIONS}
    slot = {k: pool.open(sample_rate=v[0], sample_format=v[1], channels=v[2], dtmf=v[4] if with_dtmf else None) for k, v in SESSIONS.items()}
    st = {k: dict(pos=0, i=0, ids=[], reports=[], pieces=[], done=False) for k in SESSIONS}
    steps = []
    with Launches() as ln:
        before = ln.read()
        while not all(s["done"] for s in st.values()):
            named, final = {}, []
            for k, s in st.items():
                if s["done"]:
                    continue
                sizes, total = SESSIONS[k][5], clips[k][0].shape[0]
                n = min(sizes[s["i"] % len(sizes)], total - s["pos"])
                named[k] = clips[k][0][s["pos"]:s["pos"] + n]
                s["pos"], s["i"] = s["pos"] + n, s["i"] + 1
                if s["pos"] == total:
                    final.append(k)
            out = pool.push({slot[k]: x for k, x in named.items()}, final=[slot[k] for k in final])
            after = ln.read()
            reports = pool.dtmf()
            for k in named:
                st[k]["ids"].append(out[slot[k]])
                if with_dtmf and SESSIONS[k][4] is not None:
                    st[k]["reports"].append(reports[slot[k]])
                    st[k]["pieces"].append(tuple(t.cpu() for t in pool.dtmf_blocks(slot[k])))
            if with_dtmf:                                                   # who reports: sessions with a detector, open or just ended
                live = {slot[k] for k, s in st.items() if SESSIONS[k][4] is not None and (not s["done"])}
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
        _run.update(dtmf=script_run(codec, dev, True), plain=script_run(codec, dev, False))
    return _run


@pytest.mark.parametrize("session", [k for k in SESSIONS if SESSIONS[k][4] is not None])
def test_reports_equal_the_host_scan_of_the_codec_rate_samples_after_every_step(dev, codec, session):
    r = runs(codec, dev)["dtmf"]
    s, ref = r["st"][session], r["clips"][session][2]
    cfg = dtmf.as_config(SESSIONS[session][4])
    state, at = dtmf.fresh_state(), 0
    for j, (rep, (decided, pressed)) in enumerate(zip(s["reports"], s["pieces"])):
        assert at <= rep.samples <= ref.shape[0], (session, j)
        state, d, p = dtmf.scan(ref[at:rep.samples], cfg, state, SR)
        assert rep == dtmf.report(state, N, SR), (session, j, rep, dtmf.report(state, N, SR))
        assert decided.dtype == torch.uint8 and torch.equal(decided, d) and torch.equal(pressed, p), (session, j)
        at = rep.samples
    assert at == ref.shape[0] and len(s["reports"]) >= 4                    # the final push flushed the resampler's last samples
    assert any(a.samples == b.samples for a, b in zip(s["reports"], s["reports"][1:]))     # a step without a sample: the report stands
    last = s["reports"][-1]
    assert last.blocks == ref.shape[0] // N and last.down is None
    assert last.digits == "".join(dtmf.KEYS[k] for k in SESSIONS[session][3])           # the keys that were played, on every wire


def test_ids_are_those_of_a_pool_without_detection_and_of_encode(dev, codec):
    r = runs(codec, dev)
    for k in SESSIONS:
        a, b = r["dtmf"]["st"][k]["ids"], r["plain"]["st"][k]["ids"]
        assert len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)), k
        mono = r["dtmf"]["clips"][k][1]
        kw = {} if SESSIONS[k][0] == SR else dict(sample_rate=SESSIONS[k][0])
        ids, lens = codec.encode(mono[None], torch.tensor([mono.shape[0]], device=dev), **kw)
        assert torch.equal(torch.cat(a, dim=1), ids[0, :, :int(lens[0])]), k


def test_one_more_launch_per_step_that_gained_samples_and_none_without_the_option(dev, codec):
    r = runs(codec, dev)
    assert len(r["dtmf"]["steps"]) == len(r["plain"]["steps"]) >= 6
    samples = {k: 0 for k in SESSIONS}
    idx = {k: 0 for k in SESSIONS}
    with_samples = 0
    for sv, sp in zip(r["dtmf"]["steps"], r["plain"]["steps"]):
        assert sv["named"] == sp["named"]
        new = 0
        for k in sv["named"]:
            if SESSIONS[k][4] is not None:
                rep = r["dtmf"]["st"][k]["reports"][idx[k]]
                new += rep.samples - samples[k]
                samples[k], idx[k] = rep.samples, idx[k] + 1
        expect = 1 if new else 0
        with_samples += expect
        assert sv["delta"]["dtmf"] == expect and sp["delta"]["dtmf"] == 0, (sv, sp)
        # everything else is what the pool without the option launches ("small" carries the detector's own record too)
        assert sv["delta"]["small"] == sp["delta"]["small"] + expect, (sv, sp)
        assert all(sv["delta"][f] == sp["delta"][f] for f in ("voice", "stft_logmel", "conv_igemm")), (sv, sp)
    assert 0 < with_samples < len(r["dtmf"]["steps"])                       # both kinds of step occurred
    plain, with_rows = r["plain"]["pool"], r["dtmf"]["pool"]
    assert not any(k.startswith("dtmf") for k in plain.buf) and plain.allocated_bytes() < with_rows.allocated_bytes()
    assert tuple(with_rows.buf["dtmf"].shape) == (5, 128) and with_rows.buf["dtmf_decided"].shape == with_rows.buf["dtmf_pressed"].shape == \
        (5, with_rows.codec_push // 32 + 2)


def test_a_session_that_ended_stays_reported_for_one_push_and_voice_is_independent(dev, codec):
    x = torch.from_numpy(keyed_clip(SR, N, [6, 1, 12], np.random.default_rng(9))).to(dev)
    both = codec.encode_sessions(slots=2, max_push_samples=7680, voice=True, dtmf=True)
    only_d = codec.encode_sessions(slots=2, max_push_samples=7680, dtmf=True)
    only_v = codec.encode_sessions(slots=2, max_push_samples=7680, voice=True)
    vcfg = VoiceConfig(release_frames=10)
    a, b, c = both.open(voice=vcfg, dtmf=True), only_d.open(dtmf=True), only_v.open(voice=vcfg)
    t = both.open()                                                         # a neighbour without detectors, pushed to at the end
    for at in range(0, x.shape[0], 5000):
        piece, fin = x[at:at + 5000], at + 5000 >= x.shape[0]
        ids = [p.push({s: piece}, final=(s,) if fin else ())[s] for p, s in ((both, a), (only_d, b), (only_v, c))]
        assert torch.equal(ids[0], ids[1]) and torch.equal(ids[0], ids[2])
        assert both.dtmf()[a] == only_d.dtmf()[b] and both.voice()[a] == only_v.voice()[c]
        assert all(torch.equal(u, v) for u, v in zip(both.dtmf_blocks(a), only_d.dtmf_blocks(b)))
    rep = both.dtmf()[a]
    assert rep.digits == "62*" and rep.samples == x.shape[0] and both.dtmf() == {a: rep}     # ended in the most recent push: still reported
    both.push({t: x[:100]})
    assert both.dtmf() == {} and both.voice() == {}                         # and no longer after the next one


def test_a_session_parked_while_a_key_is_down_goes_on_in_another_pool(dev, codec):
    x = torch.from_numpy(keyed_clip(SR, N, [10, 3, 13, 4], np.random.default_rng(21))).to(dev)
    cfg = DtmfConfig(misses=3)
    home = codec.encode_sessions(slots=3, max_push_samples=4096, dtmf=True)
    away = codec.encode_sessions(slots=2, max_push_samples=7680, dtmf=True)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    stay, move = home.open(dtmf=cfg), home.open(dtmf=cfg)
    other = away.open(dtmf=True)                                            # a neighbour, so that the target has buffers and history
    away.push({other: x[:3000]})
    where, slot, moved_at = home, move, None
    for j, a in enumerate(range(0, x.shape[0], 1500)):
        piece, last = x[a:a + 1500], a + 1500 >= x.shape[0]
        fin = lambda s: (s,) if last else ()
        if where is home:
            out = home.push({stay: piece, slot: piece}, final=fin(stay) + fin(slot))
            ids = (out[stay], out[slot])
            reps = home.dtmf()
            reps, blocks = (reps[stay], reps[slot]), (home.dtmf_blocks(stay), home.dtmf_blocks(slot))
        else:
            ids = (home.push({stay: piece}, final=fin(stay))[stay], away.push({slot: piece}, final=fin(slot))[slot])
            reps, blocks = (home.dtmf()[stay], away.dtmf()[slot]), (home.dtmf_blocks(stay), away.dtmf_blocks(slot))
        assert torch.equal(ids[0], ids[1]) and reps[0] == reps[1], (j, reps)
        assert torch.equal(blocks[0][0], blocks[1][0]) and torch.equal(blocks[0][1], blocks[1][1]), j
        if where is home and reps[1].down is not None and not last:         # park it while the key is down, once
            snap = home.park([slot])[slot]
            assert snap.meta["dtmf"] == cfg.as_dict() and snap.meta["layout"][-1][:3] == ["dtmf", 1, 128]
            home.buf["dtmf"][slot] = 0x7F7F7F7F
            away.buf["dtmf"][1 - other] = 0x7F7F7F7F                        # the free row it lands in is no zeroed one
            with pytest.raises(ValueError, match="dtmf=True"):
                bare.restore([snap])
            assert bare.open_slots == []
            [slot] = away.restore([snap.cpu().to(dev)])
            assert away.dtmf()[slot] == reps[1] and away.dtmf_blocks(slot)[0].numel() == 0      # the state came along; the step's bytes did not
            where, moved_at = away, j
    assert moved_at is not None and reps[0].digits == "9A04" and reps[0].total == 4 and reps[0].samples == x.shape[0]
    # a session without a detector in the dtmf pool: its snapshot is the one of a pool without the option, byte for byte
    a, b = home.open(), bare.open()
    home.push({a: x[:4096]}), bare.push({b: x[:4096]})
    sa, sb = home.snapshot([a])[a], bare.snapshot([b])[b]
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob) and "dtmf" not in sa.meta
