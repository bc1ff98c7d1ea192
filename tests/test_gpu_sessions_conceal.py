"""Encode sessions that conceal lost packets (EncodeSessions(conceal=True), open(conceal=), push(lost=)) on the GPU.  Every comparison
is equality: the ids of a concealing session are those of encode() of the host rule's output (utils/conceal.py: scan) over the
silence-filled stream at the codec's rate, with the ranges conceal.damaged maps the lost wire frames to, on four wires fed 20 ms
packets with single and double drops; they differ from the ids of the silence-filled stream; pool.concealed() is the report of the
host state; the option costs exactly one launch in a step in which a concealing session gained samples and none elsewhere; a
neighbour without it keeps the ids of encode(); with echo, DTMF and a leveller the session equals the host chain conceal, echo,
DTMF, level; a DTMF key held across a lost packet is one key press with the option and two without; a session parked inside a run
with a damaged range pending behind its resampler goes on in another pool; the refusals leave everything as it was."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import conceal, dtmf, echo, level, pcm, tones
from dmel_codec_amd.utils.conceal import ConcealConfig
from dmel_codec_amd.utils.dtmf import DtmfConfig
from dmel_codec_amd.utils.echo import EchoConfig
from dmel_codec_amd.utils.level import LevelConfig
from dmel_codec_amd.utils.resample import resample
from test_conceal_cpu import voiced
from test_echo_cpu import echo_path, echoed
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR, MS = 24000, 20
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(571, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


def encode_of(codec, dev, x):
    x = torch.as_tensor(x)
    ids, lens = codec.encode(x.to(dev)[None], torch.tensor([x.shape[0]], device=dev))
    return ids[0, :, :int(lens[0])]


def count_launches(fn):
    """the "conceal" and "small" launch records of fn()"""
    from dmel_codec_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {f: _lib.prof_read(f)["launches"] for f in ("conceal", "small")}
    finally:
        _lib.prof_enable(False); _lib.prof_reset()


class Wire:
    """one session's wire: its packets of 20 ms, the ones that never arrive, and what the host rules make of it"""

    def __init__(self, dev, clip24, rate, fmt, channels, drops, cfg):
        self.rate, self.fmt, self.ch, self.drops, self.cfg = rate, fmt, channels, set(drops), cfg
        x = torch.from_numpy(clip24).to(dev)
        if rate != SR:
            x = resample(x[None], SR, rate)[0]
        if channels > 1:                                                     # two different channels whose mean is the clip
            x = torch.stack([x * 1.25, x * 0.75], dim=1)
        if fmt == "s16":
            x = pcm.to_pcm16(x)
        elif fmt in ("ulaw", "alaw"):
            x = pcm.to_g711(x, fmt)
        self.frames = rate * MS // 1000
        self.wire = x[:x.shape[0] // self.frames * self.frames].contiguous()
        self.packets = self.wire.shape[0] // self.frames
        assert all(0 < k < self.packets - 1 for k in self.drops)             # the stream neither begins nor ends with a lost packet

    def lost_wire(self):
        return [(k * self.frames, (k + 1) * self.frames) for k in sorted(self.drops)]

    def filled(self):
        """the wire with the format's silence in the place of the lost packets -> the stream at the codec's rate, f32, on the host"""
        w = self.wire.clone()
        for lo, hi in self.lost_wire():
            w[lo:hi] = conceal.SILENCE[self.fmt]
        if self.ch > 1:
            x = pcm.downmix(w, self.fmt)
        elif self.fmt == "f32":
            x = w
        else:
            x = pcm.from_pcm16(w) if self.fmt == "s16" else pcm.from_g711(w, self.fmt)
        if self.rate != SR:
            x = resample(x[None], self.rate, SR)[0]
        return x.cpu().contiguous()

    def ranges(self, n):
        """the damaged ranges inside n codec-rate samples"""
        return [(lo, min(hi, n)) for lo, hi in conceal.damaged(self.lost_wire(), self.rate, SR) if lo < n]

    def concealed(self):
        x0 = self.filled()
        return (x0,) + conceal.scan(x0, self.ranges(x0.shape[0]), self.cfg, None, SR)

    def step(self, k):
        """what packet time k pushes: None while nothing arrives; else (chunk, frames lost in front of it)"""
        if k in self.drops or k >= self.packets:
            return None
        n = 0
        while k - 1 - n in self.drops:
            n += 1
        return self.wire[k * self.frames:(k + 1) * self.frames], n * self.frames


def run(pool, wires, extra=None):
    """every wire packet by packet, one step per packet time -> ({slot: ids}, the steps with a conceal launch, the steps)"""
    ids, steps, launched = {s: [] for s in wires}, 0, 0
    for k in range(max(w.packets for w in wires.values())):
        audio, lost, final = {}, {}, []
        for s, w in wires.items():
            got = w.step(k)
            if got is None:
                continue
            audio[s] = got[0]
            if got[1]:
                lost[s] = got[1]
            if k == w.packets - 1:
                final.append(s)
        if not audio:
            continue
        before = {s: pool.sched[s].samples for s in audio}
        kw = dict(lost=lost) if lost or k % 2 else {}                        # lost={} and no argument are the same
        if extra is not None:
            kw.update(extra(k, audio))
        out, launches = count_launches(lambda: pool.push(audio, final=final, **kw))
        # a concealing slot gained samples at the codec's rate (the last push of a stream always releases some)
        gained = [s for s in audio if pool.ccfg[s] is not None and (s in final or pool.sched[s].samples > before[s])]
        assert launches["conceal"] == int(bool(gained)), (k, launches, gained)
        launched += launches["conceal"]
        steps += 1
        for s in audio:
            ids[s].append(out[s])
    return {s: torch.cat(v, dim=1) for s, v in ids.items()}, launched, steps


def test_ids_and_reports_equal_the_host_rule_on_four_wires_next_to_a_plain_session(dev, codec):
    pool = codec.encode_sessions(slots=5, max_push_samples=4096, sample_rates=(8000, 48000), conceal=True)
    other = ConcealConfig(hold_ms=5.0, fade_ms=30.0, recover_ms=2.5)
    wires = {
        pool.open(conceal=True): Wire(dev, voiced(117.0), SR, "f32", 1, {20, 41, 42}, ConcealConfig()),
        pool.open(conceal=other, sample_rate=48000, sample_format="s16", channels=2): Wire(dev, voiced(163.0, seed=1), 48000, "s16", 2, {15, 33, 34, 60}, other),
        pool.open(conceal=True, sample_rate=8000, sample_format="ulaw"): Wire(dev, voiced(211.7, seed=2), 8000, "ulaw", 1, {25, 26, 50}, ConcealConfig()),
        pool.open(conceal=True, sample_rate=8000, sample_format="alaw"): Wire(dev, voiced(87.3, seed=3), 8000, "alaw", 1, {30, 55, 56, 57}, ConcealConfig()),
    }
    plain = pool.open()
    wires[plain] = Wire(dev, voiced(297.0, seed=4), SR, "f32", 1, (), None)  # the neighbour loses nothing
    assert set(pool.concealed()) == set(wires) - {plain} and pool.conceal_onsets(0)[0].numel() == 0
    ids, launched, steps = run(pool, wires)
    assert pool.open_slots == [] and 60 < launched <= steps == 75
    reports = pool.concealed()
    for s, w in wires.items():
        if s == plain:
            assert torch.equal(ids[s], encode_of(codec, dev, w.wire))        # the neighbour keeps encode()'s ids
            continue
        x0, y, state, periods, scores = w.concealed()
        assert len(periods) == len(w.ranges(x0.shape[0])) >= 2 and all(p > 0 for p in periods.tolist()), (s, periods)
        assert torch.equal(ids[s], encode_of(codec, dev, y)), s
        assert not torch.equal(ids[s], encode_of(codec, dev, x0)), s        # and not the ids of the silence-filled stream
        if s in reports:                                                     # the sessions that ended in the last push
            assert reports[s] == conceal.report(state, SR), (s, reports[s])
    assert len(reports) >= 2


def test_the_report_and_the_onsets_follow_the_steps(dev, codec):
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, conceal=True)
    w = Wire(dev, voiced(163.0, 24000), SR, "f32", 1, {10, 11, 30}, ConcealConfig())
    s = pool.open(conceal=True)
    x0, y, state, periods, scores = w.concealed()
    got_p, got_q, st = [], [], None
    for k in range(w.packets - 1):
        step = w.step(k)
        if step is None:
            continue
        pool.push({s: step[0]}, lost={s: step[1]})
        p, q = pool.conceal_onsets(s)
        assert p.numel() == int(step[1] > 0)
        got_p.append(p.cpu()), got_q.append(q.cpu())
        a, b = (k + 1) * 480 - 480 - step[1], (k + 1) * 480                  # the host rule over the same samples
        _, st, _, _ = conceal.scan(x0[a:b], [(0, step[1])] if step[1] else [], ConcealConfig(), st, SR)
        assert pool.concealed()[s] == conceal.report(st, SR), k
        assert torch.equal(pool.buf["conceal"][s].cpu(), st), k              # the whole row: counters and ring
    assert torch.equal(torch.cat(got_p), periods) and torch.equal(torch.cat(got_q), scores)
    rep = pool.concealed()[s]
    assert (rep.lost_samples, rep.runs, rep.longest_run, rep.muted_samples, rep.open) == (1440, 2, 960, 0, False)


def test_a_pool_or_a_step_without_the_option_launches_what_it_always_did(dev, codec):
    x = torch.from_numpy(voiced(117.0, 4800)).to(dev)
    bare, with_rows = codec.encode_sessions(slots=2, max_push_samples=4096), codec.encode_sessions(slots=2, max_push_samples=4096, conceal=True)
    a, b = bare.open(), with_rows.open()
    for at in range(0, 4800, 480):
        (ia, la), (ib, lb) = (count_launches(lambda: p.push({s: x[at:at + 480]})) for p, s in ((bare, a), (with_rows, b)))
        assert la == lb and la["conceal"] == 0 and torch.equal(ia[a], ib[b]), (at, la, lb)
    assert set(with_rows.buf) - set(bare.buf) == {"conceal", "conceal_period", "conceal_score", "conceal_tab"}
    assert tuple(with_rows.buf["conceal"].shape) == (2, conceal.ROW_WORDS) and not with_rows.buf["conceal"].any()
    assert set(bare.buf) == {"mel", "hist", "skip", "feat", "samples", "scratch", "stft_tab", "pcm_tab"} and bare.concealed() == {}
    sa, sb = bare.snapshot([a])[a], with_rows.snapshot([b])[b]               # without the option: the snapshot of a pool without it
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob)


def test_with_echo_dtmf_and_a_leveller_the_session_equals_the_host_chain(dev, codec):
    """conceal, echo, DTMF, level: the canceller, the detector and the leveller see the concealed samples"""
    n = 36000
    far = (np.random.default_rng(5).standard_normal(n) * 0.05).astype(f32)
    mic = voiced(163.0, n, seed=6) + echoed(far, echo_path(seed=7, taps=40, delay=8, gain=0.3))
    mic = tones.splice(mic.astype(f32), [(19200, tones.dtmf_program("7", SR, tone_ms=100, gap_ms=40))], SR)      # 140 ms longer
    far = np.concatenate([far, np.zeros(mic.shape[0] - n, f32)])
    ecfg, lcfg, ccfg = EchoConfig(taps=64, block_samples=16), LevelConfig(release=0.2), ConcealConfig()
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, conceal=True, echo=True, dtmf=True, level=True)
    s = pool.open(conceal=ccfg, echo=ecfg, dtmf=True, level=lcfg)
    w = Wire(dev, mic, SR, "f32", 1, {12, 35, 36, 42}, ccfg)                 # 42: inside the key
    dfar = torch.from_numpy(far).to(dev)
    sent = [0]

    def far_of(k, audio):                                                    # the far end keeps the true timeline: up to the step's last sample
        upto = (k + 1) * 480
        chunk, sent[0] = dfar[sent[0]:upto], upto
        return dict(far={s: chunk})

    ids, launched, steps = run(pool, {s: w}, far_of)
    x0, y, cstate, _, _ = w.concealed()
    es, estate = [], None
    for at in range(0, y.shape[0], 4800):                                   # in pieces: one call takes at most 39232 far samples ahead
        piece, estate, _, _ = echo.scan(y[at:at + 4800], far[at:at + 4800], ecfg, estate)
        es.append(piece)
    e = torch.cat(es)
    assert torch.equal(ids[s], encode_of(codec, dev, level.scan(e, lcfg, None, SR)[0]))
    assert pool.concealed()[s] == conceal.report(cstate, SR) and pool.echoes()[s] == echo.report(estate, 16, SR)
    assert pool.echoes()[s].far_missing == 0
    keys = pool.dtmf()[s]
    assert keys == dtmf.report(dtmf.scan(e, DtmfConfig(), None, SR)[0], DtmfConfig().block(SR), SR) and keys.digits == "7"
    assert pool.levels()[s] == level.report(level.scan(e, lcfg, None, SR)[1], 240, SR)


def test_a_key_held_across_a_lost_packet_is_one_key_press_with_the_option_and_two_without(dev, codec):
    base = (np.random.default_rng(3).standard_normal(SR) * 0.002).astype(f32)
    sig = tones.splice(base, [(7200, tones.dtmf_program("5", SR, tone_ms=200, gap_ms=40))], SR)
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, conceal=True, dtmf=True)
    on, off = pool.open(conceal=True, dtmf=True), pool.open(dtmf=True)
    w = Wire(dev, sig, SR, "f32", 1, {18}, ConcealConfig())                  # samples [8640, 9120): inside the key
    for k in range(w.packets):
        step = w.step(k)
        if step is None:
            continue
        chunk, n = step
        zeros = torch.cat((torch.zeros(n, device=dev), chunk))               # what a caller without the option can do: push zeros
        pool.push({on: chunk, off: zeros}, lost={on: n})
    keys = pool.dtmf()
    assert keys[on].digits == "5" and keys[off].digits == "55"
    assert pool.concealed()[on].runs == 1 and pool.concealed()[on].period > 0


def test_a_session_parked_inside_a_run_behind_a_resampler_goes_on_in_another_pool(dev, codec):
    cfg = ConcealConfig(hold_ms=8.0)
    w = Wire(dev, voiced(117.0, seed=8), 8000, "ulaw", 1, {30, 31, 52}, cfg)
    home = codec.encode_sessions(slots=3, max_push_samples=4096, sample_rates=(8000,), conceal=True)
    away = codec.encode_sessions(slots=2, max_push_samples=2000, sample_rates=(8000, 16000), conceal=True)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096, sample_rates=(8000,))
    stay, move = home.open(conceal=cfg, sample_rate=8000, sample_format="ulaw"), home.open(conceal=cfg, sample_rate=8000, sample_format="ulaw")
    neighbour = away.open(conceal=True)
    away.push({neighbour: torch.from_numpy(voiced(297.0, 3000)).to(dev)[:2000]})
    where, slot, got, kept = home, move, [], []
    empty = w.wire[:0]
    for k in range(w.packets):
        step = w.step(k)
        if step is None:
            continue
        chunk, n = step
        fin = lambda s: (s,) if k == w.packets - 1 else ()
        # the hole is pushed on its own, in front of the packet behind it: a step of lost frames and no audio
        for audio, lost in (((empty, n), (chunk, 0)) if n else ((chunk, 0),)):
            last = audio is chunk
            if where is home:
                out = home.push({stay: audio, slot: audio}, final=(fin(stay) + fin(slot)) if last else (), lost={stay: lost, slot: lost})
                a, b = out[stay], out[slot]
            else:
                a = home.push({stay: audio}, final=fin(stay) if last else (), lost={stay: lost})[stay]
                b = away.push({slot: audio}, final=fin(slot) if last else (), lost={slot: lost})[slot]
            assert torch.equal(a, b), k
            kept.append(a), got.append(b)
            if lost == 320 and where is home:                                # inside the run, its end not released yet
                rep = home.concealed()[slot]
                assert rep.open and rep.runs == 1 and home._lost[slot] and home._lost_open[slot]
                lo, hi = home._lost[slot][0]
                assert lo == home.sched[slot].samples and hi == conceal.damaged(w.lost_wire()[:2], 8000, SR)[0][1] and hi - lo == 3 * (7 + 7)      # the outputs whose 15-frame windows end behind the hole
                snap = home.park([slot])[slot]
                assert snap.meta["conceal"] == cfg.as_dict() and snap.meta["conceal_lost"] == [[lo, hi]] and snap.meta["conceal_open"] is True
                assert snap.meta["layout"][-1][:3] == ["conceal", 1, conceal.ROW_WORDS]
                home.buf["conceal"][slot] = 0x7F7F7F7F
                away.buf["conceal"][1 - neighbour] = 0x7F7F7F7F              # the free row it lands in is no zeroed one
                with pytest.raises(ValueError, match="conceal=True"):
                    bare.restore([snap])
                assert bare.open_slots == []
                [slot] = away.restore([snap.cpu().to(dev)])
                assert away.concealed()[slot] == rep and away._lost[slot] == [(lo, hi)] and away.conceal_onsets(slot)[0].numel() == 0
                where = away
    assert where is away
    x0, y, state, periods, _ = w.concealed()
    assert len(periods) == 2 and torch.equal(torch.cat(got, dim=1), encode_of(codec, dev, y))
    assert away.concealed()[slot] == conceal.report(state, SR) == home.concealed()[stay]


def test_refusals_leave_everything_as_it_was(dev, codec):
    x = torch.from_numpy(voiced(117.0, 4800)).to(dev)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    with pytest.raises(ValueError, match="conceal=True"):
        bare.open(conceal=True)
    s = bare.open()
    with pytest.raises(ValueError, match="conceal=True"):
        bare.push({s: x[:480]}, lost={s: 480})
    assert bare.buf is None and bare.sched[s].samples == 0                   # refused before anything was allocated or launched
    pool = codec.encode_sessions(slots=3, max_push_samples=4096, conceal=True)
    c, q = pool.open(conceal=True), pool.open()
    pool.push({c: x[:1000], q: x[:1000]}, lost={c: 0})
    before = pool.buf["conceal"].clone()
    for lost, why in (({q: 480}, "no concealment"), ({c: -1}, "count"), ({c: 480.0}, "count"), ({c: True}, "count"), ({2: 480}, "not among"),
                      ({c: 4096 - 479}, "max_push_samples")):
        with pytest.raises(ValueError, match=why):
            pool.push({c: x[1000:1480], q: x[1000:1480]}, lost=lost)
        torch.cuda.synchronize()
        assert pool.sched[c].samples == 1000 and pool._lost[c] == [] and torch.equal(pool.buf["conceal"], before), why
    pool.push({c: x[1000:1480], q: x[1000:1480]}, lost={c: 4096 - 480})      # exactly the bound
    assert pool.concealed()[c].lost_samples == 4096 - 480 and pool.sched[c].samples == 1000 + 4096
    with pytest.raises(ValueError, match="conceal=True"):
        bare.restore([pool.snapshot([c])[c]])
