"""Encode sessions with an echo canceller (EncodeSessions(echo=True), open(echo=), push(far=)) on the GPU.  Every comparison is
equality: the ids of an echo session are those of encode() of the host rule's output (utils/echo.py: scan) over the codec-rate
samples the whole-clip path produces for the session's wire, however the samples and the far end were cut; with a leveller behind
it, of encode() of level.scan of that; its DTMF report is dtmf.scan's over the cancelled samples; pool.echoes() is the report of
the host state; a session without a canceller keeps the ids of encode(); the canceller costs exactly one launch in a step in which
a session with one gained samples or far samples; a key the agent sends is read from its echo without the canceller and not with
it; the state and the far samples queued ahead travel with snapshot / restore; a pool without the option refuses all of it."""
import numpy as np
import pytest
import torch

from dmel_codec_amd.utils import dtmf, echo, level, pcm, tones
from dmel_codec_amd.utils.dtmf import DtmfConfig
from dmel_codec_amd.utils.echo import EchoConfig
from dmel_codec_amd.utils.level import LevelConfig
from dmel_codec_amd.utils.resample import resample
from test_echo_cpu import echo_path, echoed
from test_gpu_parity import make_codec

pytestmark = pytest.mark.gpu

SR = 24000
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def codec(dev):
    return make_codec(570, n_mels=80, dmel_groups=8, vocoder=None, decoder_layers=1, residual_channels=70).to(dev)


def encode_of(codec, dev, x, **kw):
    ids, lens = codec.encode(x.to(dev)[None], torch.tensor([x.shape[0]], device=dev), **kw)
    return ids[0, :, :int(lens[0])]


def line(seed, n=12000, key_at=None):
    """-> (far, mic) at the codec's rate: what the agent says -- noise, with a DTMF key spliced in at key_at -- and what comes back
    through a path of 40 taps behind 8 samples, with a little noise of the line"""
    far = (np.random.default_rng(seed).standard_normal(n) * 0.05).astype(f32)
    if key_at is not None:
        far = tones.splice(far, [(key_at, tones.dtmf_program("5", SR, tone_ms=80, gap_ms=40))], SR)
    mic = echoed(far, echo_path(seed=seed + 1, taps=40, delay=8, gain=0.3))
    return far, mic + (np.random.default_rng(seed + 2).standard_normal(far.shape[0]) * 1e-4).astype(f32)


def count_launches(fn):
    """the "echo" and "small" launch records of fn()"""
    from dmel_codec_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {f: _lib.prof_read(f)["launches"] for f in ("echo", "small")}
    finally:
        _lib.prof_enable(False); _lib.prof_reset()


def test_ids_reports_and_dtmf_equal_the_host_rules_on_two_wires_next_to_a_plain_session(dev, codec):
    pool = codec.encode_sessions(slots=3, max_push_samples=4096, sample_rates=(8000,), echo=True, level=True, dtmf=True)
    ca, cb = EchoConfig(taps=64, block_samples=16), EchoConfig(taps=128, block_samples=32, delay_samples=5, mu=0.7)
    lcfg = LevelConfig(release=0.2)
    # A: f32 at the codec's rate; B: s16 at 8 kHz with a leveller and a DTMF detector behind the canceller; P: no option
    far_a, mic_a = line(40)
    far_b, mic24 = line(50, key_at=7200)
    mic8 = resample(torch.from_numpy(mic24).to(dev)[None], SR, 8000)[0]
    wire_b = (mic8 * 32768).round().clamp(-32768, 32767).to(torch.int16)
    x_b = resample(pcm.from_pcm16(wire_b)[None], 8000, SR)[0].cpu().contiguous()       # B's clip at the codec's rate
    far_b = np.concatenate([far_b, np.zeros(max(0, x_b.shape[0] - far_b.shape[0]), f32)])
    _, plain = line(60)
    a, b, p = pool.open(echo=ca), pool.open(sample_rate=8000, sample_format="s16", echo=cb, level=lcfg, dtmf=True), pool.open()
    assert pool.echoes()[a].total_samples == 0 and pool.echo_blocks(a)[0].numel() == 0
    wires = {a: torch.from_numpy(mic_a).to(dev), b: wire_b, p: torch.from_numpy(plain).to(dev)}
    fars = {a: torch.from_numpy(far_a).to(dev), b: torch.from_numpy(far_b).to(dev)}
    # uneven pushes (cycled; a 0 is an empty push) and uneven far pushes: the far end leads by 500 samples, then by what the
    # sizes leave; B's far sizes are three times its wire's, the ratio of the rates
    sizes = {a: [3000, 17, 0, 2500, 4096], b: [1000, 0, 333, 1365], p: [4096, 100]}
    far_sizes = {a: [3500, 0, 17, 2500, 4096], b: [3600, 1000, 0, 4095]}
    pos, fpos, i = {s: 0 for s in wires}, {s: 0 for s in fars}, 0
    ids, blocks, echo_steps = {s: [] for s in wires}, {a: [], b: []}, 0
    while pos:
        named, far, final = {}, {}, []
        for s in list(pos):
            n = min(sizes[s][i % len(sizes[s])], wires[s].shape[0] - pos[s])
            named[s] = wires[s][pos[s]:pos[s] + n]
            pos[s] += n
            if s in fars:
                m = fars[s].shape[0] - fpos[s] if pos[s] == wires[s].shape[0] else min(far_sizes[s][i % len(far_sizes[s])], fars[s].shape[0] - fpos[s])
                if m or i % 2:                                               # an empty far tensor is fine too
                    far[s] = fars[s][fpos[s]:fpos[s] + m]
                fpos[s] += m
            if pos[s] == wires[s].shape[0]:
                final.append(s)
        expect = int(any((named[s].shape[0] or (s in far and far[s].shape[0])) for s in named if s in fars))
        out, launches = count_launches(lambda: pool.push(named, final=final, far=far))
        assert launches["echo"] == expect, (i, launches)
        echo_steps += expect
        for s in named:
            ids[s].append(out[s])
            if s in fars:
                blocks[s].append(tuple(t.cpu() for t in pool.echo_blocks(s)))
        for s in final:
            del pos[s]
        i += 1
    assert pool.open_slots == [] and 3 < echo_steps <= i
    reports, keys = pool.echoes(), pool.dtmf()
    assert set(reports) <= {a, b} and b in reports                           # b ended in the last push; a may have ended earlier
    # A
    ea, sa, ia, ra = echo.scan(mic_a, far_a, ca)
    assert torch.equal(torch.cat(ids[a], dim=1), encode_of(codec, dev, ea))
    assert torch.equal(torch.cat([u for u, _ in blocks[a]]), ia) and torch.equal(torch.cat([v for _, v in blocks[a]]), ra)
    assert not torch.equal(torch.cat(ids[a], dim=1), encode_of(codec, dev, torch.from_numpy(mic_a)))
    if a in reports:
        assert reports[a] == echo.report(sa, 16, SR)
    rep_a = echo.report(sa, 16, SR)
    assert rep_a.far_missing == 0 and rep_a.erle_db > 20 and rep_a.adapted_blocks > rep_a.blocks // 2
    # B: canceller, then DTMF, then leveller
    eb, sb, ib, rb = echo.scan(x_b, far_b, cb)
    assert reports[b] == echo.report(sb, 32, SR) and reports[b].far_missing == 0 and reports[b].total_samples == x_b.shape[0]
    assert torch.equal(torch.cat([u for u, _ in blocks[b]]), ib) and torch.equal(torch.cat([v for _, v in blocks[b]]), rb)
    yb = level.scan(eb, lcfg, None, SR)[0]
    assert torch.equal(torch.cat(ids[b], dim=1), encode_of(codec, dev, yb))
    assert keys[b] == dtmf.report(dtmf.scan(eb, DtmfConfig(), None, SR)[0], DtmfConfig().block(SR), SR)
    assert pool.levels()[b] == level.report(level.scan(eb, lcfg, None, SR)[1], 240, SR)
    # P
    assert torch.equal(torch.cat(ids[p], dim=1), encode_of(codec, dev, torch.from_numpy(plain)))


def test_the_agents_own_key_is_read_from_its_echo_without_the_canceller_and_not_with_it(dev, codec):
    far, mic = line(31, key_at=7200)                                         # 0.3 s of noise to adapt on, then the key
    # the host rules alone behave this way on this signal
    assert dtmf.report(dtmf.scan(mic, DtmfConfig(), None, SR)[0]).digits == "5"
    for cfg in (EchoConfig(taps=64, block_samples=16), EchoConfig(taps=128, block_samples=32)):
        e = echo.scan(mic, far, cfg)[0]
        assert dtmf.report(dtmf.scan(e, DtmfConfig(), None, SR)[0]).digits == ""
    pool = codec.encode_sessions(slots=3, max_push_samples=4096, echo=True, dtmf=True)
    bare, small, large = pool.open(dtmf=True), pool.open(dtmf=True, echo=EchoConfig(taps=64, block_samples=16)), \
        pool.open(dtmf=True, echo=EchoConfig(taps=128, block_samples=32))
    dmic, dfar = torch.from_numpy(mic).to(dev), torch.from_numpy(far).to(dev)
    for at in range(0, mic.shape[0], 1920):                                  # 80 ms pushes
        piece, x = dmic[at:at + 1920], dfar[at:at + 1920]
        pool.push({bare: piece, small: piece, large: piece}, far={small: x, large: x})
    keys = pool.dtmf()
    assert keys[bare].digits == "5" and keys[small].digits == "" and keys[large].digits == ""
    assert keys[small] == dtmf.report(dtmf.scan(echo.scan(mic, far, EchoConfig(taps=64, block_samples=16))[0], DtmfConfig(), None, SR)[0])
    reps = pool.echoes()
    assert set(reps) == {small, large} and reps[small].erle_db > 20 and reps[small].far_missing == 0


def test_a_session_parked_mid_block_with_far_samples_queued_goes_on_in_another_pool(dev, codec):
    far, mic = line(70)
    cfg = EchoConfig(taps=128, block_samples=32, delay_samples=3)
    home = codec.encode_sessions(slots=3, max_push_samples=4096, echo=True)
    away = codec.encode_sessions(slots=2, max_push_samples=7680, echo=True, far_room_samples=5000)
    tight = codec.encode_sessions(slots=2, max_push_samples=4096, echo=True, far_room_samples=100)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    stay, move = home.open(echo=cfg), home.open(echo=cfg)
    other = away.open(echo=True)                                             # a neighbour, so that the target has buffers and history
    dmic, dfar = torch.from_numpy(mic).to(dev), torch.from_numpy(far).to(dev)
    away.push({other: dmic[:3000]}, far={other: dfar[:3000]})
    where, slot, moved_at, got, fa = home, move, None, [], 0
    for j, a in enumerate(range(0, mic.shape[0], 1500)):                     # 1500 = 46 * 32 + 28: every cut lies inside a block
        piece, last = dmic[a:a + 1500], a + 1500 >= mic.shape[0]
        fb = far.shape[0] if last else min(far.shape[0], a + 1500 + 700)     # the far end is queued 700 samples ahead
        x, fa = dfar[fa:fb], fb
        fin = lambda s: (s,) if last else ()
        if where is home:
            out = home.push({stay: piece, slot: piece}, final=fin(stay) + fin(slot), far={stay: x, slot: x})
            ids, reps = (out[stay], out[slot]), home.echoes()
            reps, blocks = (reps[stay], reps[slot]), (home.echo_blocks(stay), home.echo_blocks(slot))
        else:
            ids = (home.push({stay: piece}, final=fin(stay), far={stay: x})[stay], away.push({slot: piece}, final=fin(slot), far={slot: x})[slot])
            reps, blocks = (home.echoes()[stay], away.echoes()[slot]), (home.echo_blocks(stay), away.echo_blocks(slot))
        got.append(ids[1])
        assert torch.equal(ids[0], ids[1]) and reps[0] == reps[1], (j, reps)
        assert torch.equal(blocks[0][0], blocks[1][0]) and torch.equal(blocks[0][1], blocks[1][1]), j
        if where is home and j == 2:                                         # park it mid-block, adapting, with far samples queued
            assert reps[1].total_samples % 32 == 20 and reps[1].far_ahead == 700 and reps[1].adapted_blocks > 50
            snap = home.park([slot])[slot]
            assert snap.meta["echo"] == cfg.as_dict() and snap.meta["echo_far"] == 5200
            lo, hi = echo.far_live(cfg, 4500, 5200)
            assert [seg[:3] for seg in snap.meta["layout"][-2:]] == [["echo", 1, echo.STATE_WORDS], ["echo_far.0", 1, hi - lo]]
            assert hi - lo == 5200 - (4500 - 20 - 3 - 127)
            home.buf["echo"][slot] = 0x7F7F7F7F
            away.buf["echo"][1 - other] = 0x7F7F7F7F                        # the free row it lands in is no zeroed one
            for pool, why in ((bare, "echo=True"), (tight, "far_room_samples")):
                with pytest.raises(ValueError, match=why):
                    pool.restore([snap])
                assert pool.open_slots == []
            [slot] = away.restore([snap.cpu().to(dev)])
            assert away.echoes()[slot] == reps[1] and away.echo_blocks(slot)[0].numel() == 0   # the state came along; the step's words did not
            where, moved_at = away, j
    assert moved_at == 2 and reps[0].total_samples == mic.shape[0]
    e, state, _, _ = echo.scan(mic, far, cfg)
    assert reps[1] == echo.report(state, 32, SR) and torch.equal(torch.cat(got, dim=1), encode_of(codec, dev, e))
    # a session without a canceller in the echo pool: its snapshot is the one of a pool without the option, byte for byte
    a, b = home.open(), bare.open()
    home.push({a: dmic[:4096]}), bare.push({b: dmic[:4096]})
    sa, sb = home.snapshot([a])[a], bare.snapshot([b])[b]
    assert sa.meta == sb.meta and torch.equal(sa.blob, sb.blob) and "echo" not in sa.meta


def test_a_ring_that_wraps_travels_in_two_runs(dev, codec):
    """a session pushed past 65536 far samples is parked where its live far samples lie on both sides of the ring's end"""
    cfg = EchoConfig(taps=64, block_samples=16)
    n = echo.FAR_RING + 800
    rng = np.random.default_rng(80)
    far = (rng.standard_normal(n) * 0.05).astype(f32)
    mic = echoed(far, echo_path(seed=81, taps=40, delay=8, gain=0.3))
    pool = codec.encode_sessions(slots=2, max_push_samples=7680, echo=True, far_room_samples=10000)
    stay, move = pool.open(echo=cfg), pool.open(echo=cfg)
    dmic, dfar = torch.from_numpy(mic).to(dev), torch.from_numpy(far).to(dev)
    cut = echo.FAR_RING - 300                                                # the samples seen; the far end is 500 ahead: 200 past the end
    at = fa = 0
    ids = {stay: [], move: []}
    while at < n:
        m = min(7680, (cut if at < cut else n) - at)
        fb = min(n, at + m + 500)
        out = pool.push({stay: dmic[at:at + m], move: dmic[at:at + m]}, far={stay: dfar[fa:fb], move: dfar[fa:fb]},
                        final=(stay, move) if at + m == n else ())
        for s in (stay, move):
            ids[s].append(out[s] if at >= cut else None)
        at, fa = at + m, fb
        if at == cut:
            snap = pool.park([move])[move]
            assert [seg[:3] for seg in snap.meta["layout"][-2:]] == [["echo_far.0", 1, 300 + 4 + 63], ["echo_far.1", 1, 200]]
            pool.buf["echo"][move] = 0x7F7F7F7F
            [move2] = pool.restore([snap])
            assert move2 == move
    assert all(torch.equal(u, v) for u, v in zip(ids[stay], ids[move]) if u is not None)
    reps = pool.echoes()
    assert reps[stay] == reps[move] and reps[stay].far_missing == 0 and reps[stay].total_samples == n


def test_a_pool_without_the_option_refuses_and_keeps_its_buffers_and_far_is_refused_before_any_launch(dev, codec):
    far, mic = line(90, n=3000)
    dmic, dfar = torch.from_numpy(mic).to(dev), torch.from_numpy(far).to(dev)
    bare = codec.encode_sessions(slots=2, max_push_samples=4096)
    with pytest.raises(ValueError, match="echo=True"):
        bare.open(echo=True)
    s = bare.open()
    with pytest.raises(ValueError, match="echo=True"):
        bare.push({s: dmic[:1000]}, far={s: dfar[:1000]})
    assert bare.buf is None and bare.sched[s].samples == 0                   # refused before anything was allocated or launched
    bare.push({s: dmic[:1000]})
    assert set(bare.buf) == {"mel", "hist", "skip", "feat", "samples", "scratch", "stft_tab", "pcm_tab"} and bare.echoes() == {}
    pool = codec.encode_sessions(slots=2, max_push_samples=4096, echo=True, far_room_samples=1500)
    assert pool.buf is None
    e, q = pool.open(echo=EchoConfig(taps=64, block_samples=16)), pool.open()
    pool.push({e: dmic[:100], q: dmic[:100]}, far={e: dfar[:100]})
    assert set(pool.buf) - set(bare.buf) == {"echo", "echo_in", "echo_res", "echo_tab"} and tuple(pool.buf["echo"].shape) == (2, echo.ROW_WORDS)
    before = pool.buf["echo"].clone()
    for far_arg, why in (({q: dfar[:10]}, "no canceller"), ({e: dfar[:10].double()}, "fp32"), ({e: dfar[:10][None]}, "1-D"),
                         ({e: dfar[:10].cpu()}, "audio on"), ({e: dfar[:1501]}, "far_room_samples"), ({6: dfar[:10]}, "not among")):
        with pytest.raises(ValueError, match=why):
            pool.push({e: dmic[100:200], q: dmic[100:200]}, far=far_arg)
        torch.cuda.synchronize()
        assert pool.sched[e].samples == 100 and pool._far[e] == 100 and torch.equal(pool.buf["echo"], before), why
    pool.push({e: dmic[100:200], q: dmic[100:200]}, far={e: dfar[100:1600]})   # exactly the room
    assert pool.echoes()[e].far_ahead == 1400
    with pytest.raises(ValueError, match="echo=True"):
        bare.restore([pool.snapshot([e])[e]])
