"""The input level rule of encode sessions on the host (utils/level.py), without a GPU: the config and its bounds, the state row, the
scan and its independence of how the samples were cut, what the defaults do to sines at four levels, the hold over silence, the clamp
on a loud onset, the report, the refusals of the C entry dmel_level_items (fake pointers, never read) and the pool's bookkeeping:
open(level=), the `level` key and segment of a snapshot.  Every comparison is bit equality."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot, dense_layout
from dmel_codec_amd.utils import level
from dmel_codec_amd.utils.level import LevelConfig

RATE, N = 24000, 240
CUTS = [[1, 239, 240, 241, 7, 1000], None, [13] * 384 + [8]]               # None: one push; a list that ends early: the rest follows


def sine(amp, n=24000, rate=RATE, hz=1000.0):
    """whole periods in every block of 240: the block peaks are identical"""
    return (amp * np.sin(2 * np.pi * hz * np.arange(n) / rate)).astype(np.float32)


def burst_clip(n=5000, seed=0):
    """noise at 0.05 with a x30 burst: it clamps"""
    x = (np.random.default_rng(seed).standard_normal(n) * 0.05).astype(np.float32)
    x[2000:2600] *= 30
    return x


def pieces_of(n, cuts):
    sizes = [n] if cuts is None else list(cuts)
    assert sum(sizes) <= n
    if sum(sizes) < n:
        sizes.append(n - sum(sizes))
    return sizes


def scan_in(x, cfg, sizes, rate=RATE):
    st, ys, pk, gn, at = None, [], [], [], 0
    for k in sizes:
        y, st, p, g = level.scan(x[at:at + k], cfg, st, rate)
        ys.append(y), pk.append(p), gn.append(g)
        at += k
    assert at == x.shape[0]
    return torch.cat(ys), st, torch.cat(pk), torch.cat(gn)


def block_peaks(y, n=N):
    return np.abs(y.numpy()[:y.shape[0] // n * n]).reshape(-1, n).max(axis=1)


# ------------------------------------------------------------------------------------------------------------ the config
def test_defaults_are_the_documented_ones():
    c = LevelConfig()
    assert (c.block_samples, c.target_peak, c.max_gain, c.min_gain, c.attack, c.release, c.gate, c.ceiling, c.initial_gain) == \
        (None, 0.5, 31.6, 0.1, 1.0, 0.02, 0.003, 1.0, 1.0)
    assert c.block(24000) == 240 == level.default_block(24000) and c.block(8000) == 80 and c.block(44100) == 441
    assert level.STATE_WORDS == 16 and level.fresh_state().tolist() == [0] * 16 and level.fresh_state().dtype == torch.int32
    assert level.as_config(None) is None and level.as_config(False) is None and level.as_config(True) == c and level.as_config(c) is c
    with pytest.raises(ValueError):
        level.as_config("on")
    other = LevelConfig(block_samples=64, target_peak=1, max_gain=4, release=0.5, gate=0, initial_gain=2)
    assert LevelConfig.from_dict(other.as_dict()) == other and other.target_peak == 1.0 and isinstance(other.target_peak, float)
    f32 = lambda v: float(np.float32(v))
    assert c.fparams(24000) == tuple(f32(v) for v in (1.0, 0.5, 0.5 / 31.6, 0.1, 31.6, 1.0, 0.02, 0.003, 1.0, 1 / 240))
    assert other.fparams(8000)[2] == 0.25 and other.fparams(8000)[9] == 1 / 64
    assert level.max_blocks(1, 240) == 1 and level.max_blocks(240, 240) == 1 and level.max_blocks(241, 240) == 2
    assert level.pass_blocks(32) == 64 and level.pass_blocks(240) == 17 and level.pass_blocks(4096) == 1 and level.pass_blocks(3000) == 1


@pytest.mark.parametrize("bad", [dict(block_samples=31), dict(block_samples=4097), dict(block_samples=64.0), dict(block_samples=True),
                                 dict(target_peak=0.0), dict(target_peak=-0.5), dict(target_peak=math.inf), dict(target_peak="0.5"),
                                 dict(max_gain=0.0), dict(max_gain=math.nan), dict(max_gain=True), dict(min_gain=0.0),
                                 dict(min_gain=math.inf), dict(min_gain=2.0), dict(max_gain=0.5), dict(attack=0.0), dict(attack=1.5),
                                 dict(attack=math.nan), dict(release=0.0), dict(release=1.0001), dict(release=-0.02),
                                 dict(gate=-1e-3), dict(gate=math.inf), dict(gate=None), dict(ceiling=0.0), dict(ceiling=math.nan),
                                 dict(initial_gain=0.0), dict(initial_gain=0.05), dict(initial_gain=32.0), dict(initial_gain=math.inf),
                                 dict(target_peak=1e-30, max_gain=1e10, initial_gain=1.0)])
def test_config_refuses(bad):
    with pytest.raises(ValueError):
        LevelConfig(**bad)


def test_config_bounds_that_are_accepted_and_rates_that_do_not_fit():
    LevelConfig(block_samples=32, attack=1.0, release=1.0, gate=0.0, min_gain=1.0, max_gain=1.0, initial_gain=1.0)
    LevelConfig(block_samples=4096, attack=1e-3, release=1e-6, ceiling=0.5, initial_gain=31.6)
    c = LevelConfig()
    with pytest.raises(ValueError, match="block"):
        c.block(2000)                                                       # 10 ms are 20 samples
    with pytest.raises(ValueError, match="block"):
        c.block(500000)
    assert LevelConfig(block_samples=4096).block(500000) == 4096
    for rate in (0, -8000, 8000.0, True):
        with pytest.raises(ValueError, match="sample_rate"):
            c.block(rate)


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("amp", [0.1, 0.9])
def test_a_sine_leaves_at_the_target_peak_from_block_2_on(amp):
    cfg, x = LevelConfig(), sine(amp)
    y, st, pk, gn = level.scan(x, cfg, None, RATE)
    p = np.abs(x[:N]).max()
    assert (pk.numpy() == p).all() and pk.shape[0] == 100                   # identical block peaks
    out = block_peaks(y)
    assert (out[2:] == np.float32(cfg.target_peak)).all(), out[:5]
    assert out[0] == p                                                      # block 0 passes with the initial gain
    rep = level.report(st, N, RATE)
    assert rep.locked and rep.envelope == float(p) and rep.gain == float(gn[-1]) and rep.clamped == 0 and rep.blocks == 100
    assert rep.peak_in == float(p) and rep.held_blocks == 0 and rep.total_samples == 24000


def test_a_quiet_sine_ends_at_the_gain_limit():
    cfg, x = LevelConfig(), sine(0.01)
    y, st, pk, gn = level.scan(x, cfg, None, RATE)
    p = np.abs(x[:N]).max()
    assert (gn.numpy() == np.float32(31.6)).all()
    assert (block_peaks(y)[2:] == np.float32(p * np.float32(31.6))).all()
    assert level.report(st, N, RATE).gain == float(np.float32(31.6))


def test_a_sine_below_the_gate_never_locks_and_leaves_unchanged():
    cfg, x = LevelConfig(), sine(1e-3)
    y, st, pk, gn = level.scan(x, cfg, None, RATE)
    assert np.array_equal(y.numpy().view(np.int32), x.view(np.int32))
    rep = level.report(st, N, RATE)
    assert not rep.locked and rep.gain == 1.0 and rep.gain_db == 0.0 and rep.blocks == 100 and (gn.numpy() == 1.0).all()
    assert rep.peak_in == float(np.abs(x).max()) == rep.peak_out


@pytest.mark.parametrize("cfg", [LevelConfig(), LevelConfig(block_samples=32, release=0.5, attack=0.5),
                                 LevelConfig(block_samples=4096, initial_gain=3.0, max_gain=8.0)])
def test_any_cut_of_the_samples_gives_the_bits_of_one_call(cfg):
    x = burst_clip()
    y, st, pk, gn = level.scan(x, cfg, None, RATE)
    if cfg == LevelConfig():
        assert int(st[level.I_CLAMPED]) == 265                              # the burst meets the ceiling
    for cuts in CUTS:
        y2, st2, pk2, gn2 = scan_in(x, cfg, pieces_of(x.shape[0], cuts))
        assert torch.equal(y2.view(torch.int32), y.view(torch.int32)) and torch.equal(st2, st), cuts
        assert torch.equal(pk2, pk) and torch.equal(gn2, gn) and int(st2[level.I_CLAMPED]) == int(st[level.I_CLAMPED])
    assert int(st[level.I_BLOCKS]) == pk.shape[0] == 5000 // cfg.block(RATE) and int(st[level.I_FILL]) == 5000 % cfg.block(RATE)


def test_no_sample_changes_nothing_and_neither_input_is_modified():
    x = burst_clip(1000)
    keep = x.copy()
    _, st, _, _ = level.scan(x, LevelConfig(), None, RATE)
    before = st.clone()
    y, st2, pk, gn = level.scan(np.zeros(0, np.float32), LevelConfig(), st, RATE)
    assert y.shape == (0,) and pk.shape == (0,) and gn.shape == (0,) and torch.equal(st2, before) and torch.equal(st, before)
    level.scan(x, LevelConfig(), st, RATE)
    assert torch.equal(st, before) and np.array_equal(x, keep)
    assert not st[11:].any()                                                # the reserved words stay 0
    with pytest.raises(ValueError):
        level.scan(x.astype(np.float64), LevelConfig())
    with pytest.raises(ValueError):
        level.scan(x, LevelConfig(), st.to(torch.int64))
    bad = st.clone()
    bad[level.I_FILL] = 240
    with pytest.raises(ValueError, match="open block"):
        level.scan(x, LevelConfig(), bad, RATE)


def test_silence_holds_the_gain():
    cfg = LevelConfig()
    x = np.concatenate([sine(0.2, 2400), np.zeros(4800, np.float32)])
    _, st1, _, g1 = level.scan(x[:2400], cfg, None, RATE)
    y, st, pk, gn = level.scan(x, cfg, None, RATE)
    rep1, rep = level.report(st1, N, RATE), level.report(st, N, RATE)
    assert rep.gain == rep1.gain == float(np.float32(0.5) / np.abs(x[:N]).max()) and rep.envelope == rep1.envelope
    assert rep.held_blocks == 20 and rep.blocks == 30 and (gn[10:] == g1[-1]).all() and not y[2400:].any()
    # without the hold (gate 0) the release pumps the gain up
    loose = level.report(level.scan(x, LevelConfig(gate=0.0), None, RATE)[1], N, RATE)
    assert loose.held_blocks == 0 and loose.gain > rep.gain


def test_a_loud_onset_passes_unclamped_at_first_and_is_clamped_behind_a_quiet_stretch():
    cfg = LevelConfig()
    x = np.concatenate([np.zeros(500, np.float32), sine(0.9, 4800)])
    y, st, _, _ = level.scan(x, cfg, None, RATE)
    rep = level.report(st, N, RATE)
    assert rep.clamped == 0 and rep.locked and rep.peak_out <= 1.0           # gain 1 until acquired
    x = np.concatenate([sine(0.01, 4800), sine(0.9, 4800)])
    y, st, _, _ = level.scan(x, cfg, None, RATE)
    rep = level.report(st, N, RATE)
    assert rep.clamped > 0 and float(np.abs(y.numpy()).max()) == 1.0 == rep.peak_out
    assert (np.abs(y.numpy()[-2400:]) <= np.float32(0.5)).all()              # and it settles


def test_report_of_a_fresh_row():
    rep = level.report(level.fresh_state(), N, RATE)
    assert rep == level.LevelReport(gain=1.0, gain_db=0.0, envelope=0.0, locked=False, peak_in=0.0, peak_in_dbfs=-math.inf, peak_out=0.0,
                                    clamped=0, held_blocks=0, blocks=0, total_samples=0, block=240, sample_rate=24000)
    assert rep.samples(3) == 720 and rep.seconds(100) == 1.0
    assert level.report(level.fresh_state(), 80, 8000, initial_gain=2.0).gain == 2.0
    assert abs(level.report(level.fresh_state(), 80, 8000, initial_gain=2.0).gain_db - 6.0206) < 1e-3


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_level_entry_refuses_before_it_launches():
    """dmel_level_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_level_items"][1]) == 13
    fake = 1 << 20
    good = LevelConfig().fparams(RATE)

    def call(n_new, first=None, N=None, fp=None, S=None, samples=fake, stride=9000, state=fake + (1 << 16), peak=fake + (1 << 17),
             gain=fake + (1 << 18), pitch=100, table=fake + (1 << 19)):
        n = len(n_new)
        first = [0] * n if first is None else first
        N = [240] * n if N is None else N
        fp = [good] * n if fp is None else fp
        rc = lib.dmel_level_items(samples, stride, n if S is None else S, (C.c_int64 * n)(*first), (C.c_int64 * n)(*n_new),
                                  (C.c_int32 * n)(*N), (C.c_float * (10 * n))(*[v for r in fp for v in r]), state, peak, gain, pitch,
                                  table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    def with_(k, v):
        return [good, good[:k] + (v,) + good[k + 1:]]

    cases = [(dict(n_new=[5, -1]), ("item 1", "new samples")),
             (dict(n_new=[5, 1 << 30]), ("item 1", "new samples")),
             (dict(n_new=[5, 5], first=[0, -1]), ("item 1", "first column")),
             (dict(n_new=[5, 5], first=[1 << 30, 0]), ("item 0", "first column")),
             (dict(n_new=[5, 5], N=[240, 31]), ("item 1", "block")),
             (dict(n_new=[5, 5], N=[4097, 240]), ("item 0", "block")),
             (dict(n_new=[240 * 100 + 1, 5]), ("item 0", "pitch")),
             (dict(n_new=[5, 32 * 100 + 1], N=[240, 32]), ("item 1", "pitch")),
             (dict(n_new=[5, 5], fp=with_(5, 1.5)), ("item 1", "attack")),
             (dict(n_new=[5, 5], fp=with_(6, 1.0001)), ("item 1", "release")),
             (dict(n_new=[5, 5], fp=with_(9, 2.0)), ("item 1", "rN")),
             (dict(n_new=[5, 5], fp=with_(0, 0.05)), ("item 1", "initial_gain")),
             (dict(n_new=[5, 5], fp=with_(0, 40.0)), ("item 1", "initial_gain"))]
    for k in range(10):
        for v in (-1.0, math.inf, math.nan) + ((0.0,) if k != 7 else ()):
            cases.append((dict(n_new=[5, 5], fp=with_(k, v)), ("item 1", f"float parameter {k}")))
    for kw, words in cases:
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for S in (0, -1, 65536):
        rc, msg = call([5], S=S)
        assert rc == -1 and "65535" in msg, (S, rc, msg)
    for kw in (dict(samples=None), dict(state=None), dict(peak=None), dict(gain=None), dict(table=None), dict(samples=fake + 2),
               dict(state=fake + 1), dict(peak=fake + 2), dict(gain=fake + 1), dict(table=fake + 3), dict(stride=-1), dict(pitch=-1)):
        assert call([5], **kw)[0] == -1, kw
    # idle items: their parameters are not looked at, and a call of idle items only launches nothing
    nan = (math.nan,) * 10
    assert call([0, 0], first=[-5, -5], N=[0, 0], fp=[nan, nan], pitch=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.lcfg))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.lcfg) == before              # a refused restore takes no slot


def test_pool_bookkeeping_of_sessions_with_a_leveller(codec):
    cfg = LevelConfig(block_samples=256, target_peak=0.25)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, level=True)
    both = codec.encode_sessions(2, max_push_samples=4096, dtmf=True, level=True)
    assert not plain_pool.level_on and pool.level_on and not pool.dtmf_on and both.dtmf_on and both.level_on and plain_pool.cap == pool.cap
    # open(level=) on a pool without rows: refused, no slot taken
    for v in (True, cfg):
        with pytest.raises(ValueError, match="level=True"):
            plain_pool.open(level=v)
    assert plain_pool.open_slots == [] and plain_pool.levels() == {}
    with pytest.raises(ValueError):
        pool.open(level="on")
    with pytest.raises(ValueError):
        pool.open(level=dict(target_peak=0.5))
    with pytest.raises(ValueError):
        codec.encode_sessions(2, level=cfg)                                 # the pool's option is a bool: configs belong to sessions
    with pytest.raises(ValueError, match="dtmf=True"):
        pool.open(dtmf=True, level=True)                                    # the options are independent
    assert pool.open_slots == []
    a, b, c = pool.open(level=True), pool.open(), pool.open(level=cfg)
    assert pool.lcfg == [LevelConfig(), None, cfg]
    v = both.open(dtmf=True, level=cfg)
    assert both.dcfg[v] is not None and both.lcfg[v] == cfg
    # nothing was pushed: reports of no sample, without buffers or a device
    reps = pool.levels()
    assert set(reps) == {a, c} and pool.buf is None
    assert reps[a] == level.report(level.fresh_state(), 240, pool.codec_rate) and reps[c].block == 256 and reps[c].total_samples == 0
    with pytest.raises(ValueError, match="leveller"):
        pool.level_blocks(b)
    # the snapshot: the key only where a leveller is on; a fresh session owns the zeroed row, so no words
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["level"] == LevelConfig().as_dict() and snaps[c].meta["level"] == cfg.as_dict() and "level" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without a leveller: the snapshot of a pool without the option
    plain_pool.drop(0)
    assert all(sn.nbytes == 0 and sn.meta["layout"] == [] for sn in snaps.values())
    sv = both.snapshot([v])[v]
    assert sv.meta["level"] == cfg.as_dict() and "dtmf" in sv.meta
    # the layout of a session that has seen samples: one tail segment ("level", 1, 16) behind the others
    meta = copy.deepcopy(snaps[c].meta)
    meta["schedule"]["samples"] = 1
    shapes = pool._park_shapes(meta)
    assert shapes[-1] == ("level", 1, 16) and shapes[:-1] == pool._park_shapes({k: x for k, x in meta.items() if k != "level"})
    assert dense_layout(shapes)[0][-1] == ["level", 1, 16, 0]
    # a pool without the option refuses the key; a level pool takes snapshots with and without it
    refused(plain_pool, snaps[c], "level=True")
    refused(plain_pool, snaps[a], "level=True")
    assert plain_pool.restore([snaps[b]]) == [0]
    other = codec.encode_sessions(4, max_push_samples=1000, level=True)
    assert other.restore([snaps[c], snaps[b], snaps[a]]) == [0, 1, 2] and other.lcfg == [cfg, None, LevelConfig(), None]
    assert set(other.levels()) == {0, 2}
    refused(other, SessionSnapshot(dict(snaps[c].meta, level=dict(snaps[c].meta["level"], release=-1.0)), snaps[c].blob), "release")
    refused(other, SessionSnapshot(dict(snaps[c].meta, level=dict(snaps[c].meta["level"], loudness=3)), snaps[c].blob), "LevelConfig")
    refused(pool, sv, "dtmf=True")                                          # the other option's rows are still needed
    other.drop(0)
    assert set(other.levels()) == {2}
    with pytest.raises(ValueError):
        other.level_blocks(0)
