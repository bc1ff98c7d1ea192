"""The DTMF rule of encode sessions on the host (utils/dtmf.py), without a GPU: the config and its bounds, the state row, the scan and
its independence of how the samples were cut, detection and rejection with the defaults on synthetic signals, the event ring, the
refusals of the C entry dmel_dtmf_items (fake pointers, never read) and the pool's bookkeeping: open(dtmf=), the `dtmf` key and
segment of a snapshot."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot, dense_layout
from dmel_codec_amd.utils import dtmf
from dmel_codec_amd.utils.dtmf import DtmfConfig

RATES = [(24000, 307), (8000, 102), (44100, 564)]


# ------------------------------------------------------------------------------------------------------------ the config
def test_defaults_are_the_documented_ones():
    c = DtmfConfig()
    assert (c.block_samples, c.min_mean_square, c.rel, c.max_col_over_row, c.max_row_over_col, c.purity, c.hits, c.misses) == \
        (None, 1e-6, 6.0, 2.51, 6.31, 0.5, 2, 2)
    for rate, n in RATES:
        assert c.block(rate) == n == dtmf.default_block(rate)
    assert dtmf.KEYS == "123A456B789C*0#D" and dtmf.ROWS_HZ == (697.0, 770.0, 852.0, 941.0) and dtmf.COLS_HZ == (1209.0, 1336.0, 1477.0, 1633.0)
    assert dtmf.as_config(None) is None and dtmf.as_config(False) is None and dtmf.as_config(True) == c and dtmf.as_config(c) is c
    with pytest.raises(ValueError):
        dtmf.as_config("on")
    other = DtmfConfig(block_samples=64, rel=3, hits=1, misses=5)
    assert DtmfConfig.from_dict(other.as_dict()) == other and other.rel == 3.0 and isinstance(other.rel, float)
    assert c.coefficients(8000)[0] == float(np.float32(2 * math.cos(2 * math.pi * 697 / 8000)))
    assert c.fparams(8000) == tuple(float(np.float32(v)) for v in (1e-6 * 102, 6.0, 2.51, 6.31, 0.5 * 102 / 2))


@pytest.mark.parametrize("bad", [dict(block_samples=31), dict(block_samples=4097), dict(block_samples=64.0), dict(block_samples=True),
                                 dict(min_mean_square=0.0), dict(min_mean_square=-1e-6), dict(min_mean_square=math.inf),
                                 dict(rel=0.0), dict(rel=math.nan), dict(rel="6"), dict(rel=True),
                                 dict(max_col_over_row=0.0), dict(max_col_over_row=math.inf), dict(max_row_over_col=-1.0),
                                 dict(max_row_over_col=math.nan), dict(purity=0.0), dict(purity=math.inf),
                                 dict(hits=0), dict(hits=(1 << 20) + 1), dict(hits=2.0), dict(hits=True),
                                 dict(misses=0), dict(misses=(1 << 20) + 1), dict(misses=None)])
def test_config_refuses(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        DtmfConfig(**bad)


def test_config_bounds_that_are_accepted_and_rates_that_do_not_fit():
    DtmfConfig(block_samples=32, hits=1, misses=1 << 20)
    DtmfConfig(block_samples=4096, hits=1 << 20, misses=1)
    c = DtmfConfig()
    with pytest.raises(ValueError, match="column"):
        c.block(3266)                                                       # 1633 Hz is not below half of it
    with pytest.raises(ValueError, match="block"):
        c.block(384000)                                                     # 12.8 ms are 4915 samples
    assert DtmfConfig(block_samples=4096).block(384000) == 4096
    for rate in (0, -8000, 8000.0, True):
        with pytest.raises(ValueError, match="sample_rate"):
            c.block(rate)


# ------------------------------------------------------------------------------------------------------------ signals
def tone(n, rate, freq, amp, phase):
    t = np.arange(n, dtype=np.float64) / rate
    return amp * np.sin(2 * np.pi * freq * t + phase)


def keyed_clip(rate, N, keys, rng, noise=True, twist_db=None):
    """every key 40 ms + 1 sample on and 40 ms + 1 sample off behind a lead-in of less than a block; tones of amplitude 0.1 with
    random phases, the column tone scaled by a twist drawn from [-6, +3] dB; white noise 15 dB under a tone"""
    on = rate * 40 // 1000 + 1
    parts = [np.zeros(int(rng.integers(0, N)))]
    for k in keys:
        tw = rng.uniform(-6.0, 3.0) if twist_db is None else twist_db
        parts.append(tone(on, rate, dtmf.ROWS_HZ[k // 4], 0.1, rng.uniform(0, 2 * np.pi))
                     + tone(on, rate, dtmf.COLS_HZ[k % 4], 0.1 * 10.0 ** (tw / 20.0), rng.uniform(0, 2 * np.pi)))
        parts.append(np.zeros(on))
    x = np.concatenate(parts)
    if noise:
        x = x + rng.standard_normal(x.shape[0]) * math.sqrt(0.1 ** 2 / 2 / 10.0 ** 1.5)
    return x.astype(np.float32)


def run(x, cfg, rate):
    state, decided, pressed = dtmf.scan(x, cfg, None, rate)
    return state, decided, pressed, dtmf.report(state, cfg.block(rate), rate)


# ------------------------------------------------------------------------------------------------------------ detection
@pytest.mark.parametrize("rate,N", RATES)
def test_defaults_read_every_key_of_twenty_random_sequences(rate, N):
    rng = np.random.default_rng(1000 + rate)
    cfg = DtmfConfig()
    for trial in range(20):
        keys = [int(k) for k in rng.permutation(16)]
        x = keyed_clip(rate, N, keys, rng)
        state, decided, pressed, rep = run(x, cfg, rate)
        want = "".join(dtmf.KEYS[k] for k in keys)
        assert rep.digits == want, (rate, trial, rep.digits, want)
        assert rep.total == 16 and rep.down is None and rep.blocks == x.shape[0] // N == decided.shape[0] and rep.samples == x.shape[0]
        on = rate * 40 // 1000 + 1
        for (i, key, start, end), k in zip(rep.events, keys):               # the event lies where the key was played
            assert key == dtmf.KEYS[k] and end is not None and start % N == 0 and end % N == 0
            assert 2 * on * i - N < start < 2 * on * i + 2 * N and start + N < end <= start + on + 2 * N, (trial, i, start, end)


@pytest.mark.parametrize("rate,N", RATES[:2])
@pytest.mark.parametrize("signal", ["noise", "tone", "buzz140", "buzz233", "silence", "twist+12", "twist-12"])
def test_defaults_give_no_event_on(signal, rate, N):
    rng = np.random.default_rng(7)
    n = 2 * rate
    if signal == "noise":
        x = rng.standard_normal(n) * 0.1
    elif signal == "tone":
        x = tone(n, rate, 770.0, 0.1, 0.3)
    elif signal.startswith("buzz"):
        f0, h = (140.0, 20) if signal == "buzz140" else (233.0, 14)
        x = sum(tone(n, rate, f0 * k, 0.1 / k, 0.1 * k) for k in range(1, h + 1))
    elif signal == "silence":
        x = np.zeros(n)
    else:
        db = 12.0 if signal == "twist+12" else -12.0
        x = tone(n, rate, 770.0, 0.1, 0.3) + tone(n, rate, 1336.0, 0.1 * 10.0 ** (db / 20.0), 1.1)
    state, decided, pressed, rep = run(x.astype(np.float32), DtmfConfig(), rate)
    assert rep.total == 0 and rep.digits == "" and rep.events == () and rep.down is None and not pressed.any(), (signal, rep)
    assert rep.blocks == n // N


def test_a_zeroed_row_is_the_fresh_state_and_no_sample_changes_nothing():
    assert dtmf.fresh_state().dtype == torch.int32 and tuple(dtmf.fresh_state().shape) == (128,) and not dtmf.fresh_state().any()
    rep = dtmf.report(dtmf.fresh_state(), 307, 24000)
    assert rep == dtmf.DtmfReport(digits="", events=(), total=0, down=None, blocks=0, samples=0, block=307, sample_rate=24000)
    x = keyed_clip(8000, 102, [5], np.random.default_rng(3))[:1000]
    state, d, p = dtmf.scan(x, DtmfConfig(), None, 8000)
    again, d0, p0 = dtmf.scan(np.zeros(0, np.float32), DtmfConfig(), state, 8000)
    assert torch.equal(again, state) and d0.numel() == 0 and p0.numel() == 0 and d.dtype == torch.uint8
    assert not state[24:32].any()                                           # the reserved words
    for bad in (state.float(), state[:100], torch.zeros(128, dtype=torch.int64)):
        with pytest.raises(ValueError):
            dtmf.scan(x, DtmfConfig(), bad, 8000)
    with pytest.raises(ValueError):
        dtmf.scan(x.astype(np.float64), DtmfConfig(), None, 8000)


def test_a_whole_last_block_leaves_a_zeroed_carry_and_a_key_held_is_reported():
    rate, N = 8000, 102
    x = (tone(10 * N, rate, 852.0, 0.1, 0.2) + tone(10 * N, rate, 1477.0, 0.1, 0.9)).astype(np.float32)
    state, decided, pressed, rep = run(x, DtmfConfig(), rate)
    assert not state[:18].any() and rep.blocks == 10 and rep.samples == 10 * N
    assert rep.down == "9" and rep.digits == "9" and rep.events == ((0, "9", 0, None),) and rep.total == 1
    assert decided.tolist() == [11] * 10 and pressed.tolist() == [0] + [11] * 9    # key 10 ("9"), stored as key + 1
    state, _, _ = dtmf.scan(x[:50], DtmfConfig(), state, rate)
    assert int(state[dtmf.I_FILL]) == 50 and state[:17].any()


# ------------------------------------------------------------------------------------------------------------ chunking
def cuts_of(n, N, rng):
    sizes, fixed, at = [], [1, N - 1, N, N + 1, 3 * N + 7, 0, 2, 2 * N, 29 * N + 3, 5], 0
    for k in fixed + [int(v) for v in rng.integers(0, 4 * N, size=64)]:
        k = min(k, n - at)
        sizes.append(k)
        at += k
    if at < n:
        sizes.append(n - at)
    return sizes


@pytest.mark.parametrize("rate,N,cfg", [(24000, 307, DtmfConfig()), (8000, 102, DtmfConfig()), (44100, 564, DtmfConfig()),
                                        (8000, 32, DtmfConfig(block_samples=32, rel=1.5, hits=1, misses=1)),
                                        (24000, 4096, DtmfConfig(block_samples=4096, hits=1))])
def test_any_cut_of_the_samples_gives_the_bits_of_one_call(rate, N, cfg):
    rng = np.random.default_rng(N)
    x = np.concatenate([keyed_clip(rate, N, [3, 8, 14], rng), keyed_clip(rate, N, [0, 0, 11], rng, noise=False)])
    if N == 4096:
        x = np.concatenate([x, tone(6 * N, rate, 941.0, 0.2, 0.0).astype(np.float32) + tone(6 * N, rate, 1209.0, 0.2, 1.0).astype(np.float32)])
    whole, d, p = dtmf.scan(x, cfg, None, rate)
    assert d.shape[0] == x.shape[0] // N
    for seed in (0, 1):
        state, ds, ps, at = None, [], [], 0
        for k in cuts_of(x.shape[0], N, np.random.default_rng(seed)):
            state, dk, pk = dtmf.scan(x[at:at + k], cfg, state, rate)
            ds.append(dk), ps.append(pk)
            at += k
        assert at == x.shape[0] and torch.equal(state, whole) and torch.equal(torch.cat(ds), d) and torch.equal(torch.cat(ps), p), (N, seed)
    assert int(whole[dtmf.I_EVENTS]) >= 1


# ------------------------------------------------------------------------------------------------------------ the ring
def test_the_ring_keeps_the_last_32_events_and_the_total():
    # 32 samples resolve rate / 32 Hz: at 4 kHz the corners of the keypad, "1" and "D", are two bins apart; the conditions that
    # need a longer block (rel, the twist limits) are set aside, so that a block decides the strongest pair
    rate, N = 4000, 32
    cfg = DtmfConfig(block_samples=N, rel=0.01, max_col_over_row=100.0, max_row_over_col=100.0, purity=0.05, hits=1, misses=1)
    keys = [0, 15] * 20
    parts = []
    for i, k in enumerate(keys):                                           # two blocks of the key, two of silence
        parts.append(tone(2 * N, rate, dtmf.ROWS_HZ[k // 4], 0.2, 0.1 * i) + tone(2 * N, rate, dtmf.COLS_HZ[k % 4], 0.2, 0.2 * i))
        parts.append(np.zeros(2 * N))
    x = np.concatenate(parts).astype(np.float32)
    state, decided, pressed, rep = run(x, cfg, rate)
    # with hits = misses = 1 an event is a maximal run of one key in `pressed`
    p = pressed.tolist()
    runs = [(b, p[b]) for b in range(len(p)) if p[b] and (b == 0 or p[b - 1] != p[b])]
    assert len(runs) == 40 and [k for _, k in runs] == [k + 1 for k in keys]
    assert rep.total == 40 and len(rep.events) == 32 and rep.digits == "".join(dtmf.KEYS[k] for k in keys[8:])
    assert [(i, b * N) for (i, _, b, _) in [(e[0], e[1], e[2] // N, e[3]) for e in rep.events]] == [(i, runs[i][0] * N) for i in range(8, 40)]
    assert all(end == start + 2 * N for _, _, start, end in rep.events)
    # the same in pieces, so that the ring wraps across calls
    st = None
    for a in range(0, x.shape[0], 1000):
        st, _, _ = dtmf.scan(x[a:a + 1000], cfg, st, rate)
    assert torch.equal(st, state)


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_dtmf_entry_refuses_before_it_launches():
    """dmel_dtmf_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_dtmf_items"][1]) == 15
    fake = 1 << 20
    cfg = DtmfConfig()
    good_c, good_f, good_i = cfg.coefficients(8000), cfg.fparams(8000), (2, 2)

    def call(n_new, first=None, N=None, ck=None, fp=None, ip=None, S=None, samples=fake, stride=9000, state=fake + (1 << 16),
             decided=fake + (1 << 17), pressed=fake + (1 << 18), pitch=100, table=fake + (1 << 19)):
        n = len(n_new)
        first = [0] * n if first is None else first
        N = [102] * n if N is None else N
        ck = [good_c] * n if ck is None else ck
        fp = [good_f] * n if fp is None else fp
        ip = [good_i] * n if ip is None else ip
        rc = lib.dmel_dtmf_items(samples, stride, n if S is None else S, (C.c_int64 * n)(*first), (C.c_int64 * n)(*n_new), (C.c_int32 * n)(*N),
                                 (C.c_float * (8 * n))(*[v for r in ck for v in r]), (C.c_float * (5 * n))(*[v for r in fp for v in r]),
                                 (C.c_int32 * (2 * n))(*[v for r in ip for v in r]), state, decided, pressed, pitch, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    def with_(row, k, v):
        return [row, row[:k] + (v,) + row[k + 1:]]

    cases = [(dict(n_new=[5, -1]), ("item 1", "new samples")),
             (dict(n_new=[5, 1 << 30]), ("item 1", "new samples")),
             (dict(n_new=[5, 5], first=[0, -1]), ("item 1", "first column")),
             (dict(n_new=[5, 5], first=[1 << 30, 0]), ("item 0", "first column")),
             (dict(n_new=[5, 5], N=[102, 31]), ("item 1", "block")),
             (dict(n_new=[5, 5], N=[4097, 102]), ("item 0", "block")),
             (dict(n_new=[102 * 100 + 1, 5]), ("item 0", "pitch")),
             (dict(n_new=[5, 32 * 100 + 1], N=[102, 32]), ("item 1", "pitch")),
             (dict(n_new=[5, 5], ck=with_(good_c, 3, math.nan)), ("item 1", "coefficient 3")),
             (dict(n_new=[5, 5], ck=with_(good_c, 7, 2.5)), ("item 1", "coefficient 7")),
             (dict(n_new=[5, 5], ip=with_(good_i, 0, 0)), ("item 1", "hits")),
             (dict(n_new=[5, 5], ip=with_(good_i, 0, (1 << 20) + 1)), ("item 1", "hits")),
             (dict(n_new=[5, 5], ip=with_(good_i, 1, 0)), ("item 1", "misses")),
             (dict(n_new=[5, 5], ip=with_(good_i, 1, (1 << 20) + 1)), ("item 1", "misses"))]
    for k in range(5):
        for v in (0.0, -1.0, math.inf, math.nan):
            cases.append((dict(n_new=[5, 5], fp=with_(good_f, k, v)), ("item 1", f"float parameter {k}")))
    for kw, words in cases:
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for S in (0, -1, 65536):
        rc, msg = call([5], S=S)
        assert rc == -1 and "65535" in msg, (S, rc, msg)
    for kw in (dict(samples=None), dict(state=None), dict(decided=None), dict(pressed=None), dict(table=None), dict(samples=fake + 2),
               dict(state=fake + 1), dict(table=fake + 3), dict(stride=-1), dict(pitch=-1)):
        assert call([5], **kw)[0] == -1, kw
    # idle items: their parameters are not looked at, and a call of idle items only launches nothing
    nan = (math.nan,) * 5
    assert call([0, 0], first=[-5, -5], N=[0, 0], ck=[(math.nan,) * 8] * 2, fp=[nan, nan], ip=[(0, 0)] * 2, pitch=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.dcfg))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.dcfg) == before              # a refused restore takes no slot


def test_pool_bookkeeping_of_sessions_with_a_dtmf_detector(codec):
    cfg = DtmfConfig(block_samples=256, hits=3)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, dtmf=True)
    both = codec.encode_sessions(2, max_push_samples=4096, voice=True, dtmf=True)
    assert not plain_pool.dtmf_on and pool.dtmf_on and not pool.voice_on and both.voice_on and both.dtmf_on and plain_pool.cap == pool.cap
    # open(dtmf=) on a pool without rows: refused, no slot taken
    for v in (True, cfg):
        with pytest.raises(ValueError, match="dtmf=True"):
            plain_pool.open(dtmf=v)
    assert plain_pool.open_slots == [] and plain_pool.dtmf() == {}
    with pytest.raises(ValueError):
        pool.open(dtmf="on")
    with pytest.raises(ValueError):
        codec.encode_sessions(2, dtmf=cfg)                                  # the pool's option is a bool: configs belong to sessions
    with pytest.raises(ValueError, match="voice=True"):
        pool.open(voice=True, dtmf=True)                                    # the options are independent
    assert pool.open_slots == []
    a, b, c = pool.open(dtmf=True), pool.open(), pool.open(dtmf=cfg)
    assert pool.dcfg == [DtmfConfig(), None, cfg]
    v = both.open(voice=True, dtmf=cfg)
    assert both.vcfg[v] is not None and both.dcfg[v] == cfg
    # nothing was pushed: reports of no sample, without buffers or a device
    reps = pool.dtmf()
    assert set(reps) == {a, c} and pool.buf is None
    assert reps[a] == dtmf.report(dtmf.fresh_state(), 307, pool.codec_rate) and reps[c].block == 256 and reps[c].samples == 0
    with pytest.raises(ValueError, match="DTMF"):
        pool.dtmf_blocks(b)
    # the snapshot: the key only where a detector is on; a fresh session owns the zeroed row, so no words
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["dtmf"] == DtmfConfig().as_dict() and snaps[c].meta["dtmf"] == cfg.as_dict() and "dtmf" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without a detector: the snapshot of a pool without the option
    plain_pool.drop(0)
    assert all(sn.nbytes == 0 and sn.meta["layout"] == [] for sn in snaps.values())
    sv = both.snapshot([v])[v]
    assert sv.meta["dtmf"] == cfg.as_dict() and "voice" in sv.meta
    # the layout of a session that has seen samples: one tail segment ("dtmf", 1, 128) behind the others
    meta = copy.deepcopy(snaps[c].meta)
    meta["schedule"]["samples"] = 1
    shapes = pool._park_shapes(meta)
    assert shapes[-1] == ("dtmf", 1, 128) and shapes[:-1] == pool._park_shapes({k: x for k, x in meta.items() if k != "dtmf"})
    assert dense_layout(shapes)[0][-1] == ["dtmf", 1, 128, 0]
    # a pool without the option refuses the key; a dtmf pool takes snapshots with and without it
    refused(plain_pool, snaps[c], "dtmf=True")
    refused(plain_pool, snaps[a], "dtmf=True")
    assert plain_pool.restore([snaps[b]]) == [0]
    other = codec.encode_sessions(4, max_push_samples=1000, dtmf=True)
    assert other.restore([snaps[c], snaps[b], snaps[a]]) == [0, 1, 2] and other.dcfg == [cfg, None, DtmfConfig(), None]
    assert set(other.dtmf()) == {0, 2}
    refused(other, SessionSnapshot(dict(snaps[c].meta, dtmf=dict(snaps[c].meta["dtmf"], rel=-1.0)), snaps[c].blob), "rel")
    refused(other, SessionSnapshot(dict(snaps[c].meta, dtmf=dict(snaps[c].meta["dtmf"], loudness=3)), snaps[c].blob), "DtmfConfig")
    refused(pool, sv, "voice=True")                                         # the other option's rows are still needed
    other.drop(0)
    assert set(other.dtmf()) == {2}
    with pytest.raises(ValueError):
        other.dtmf_blocks(0)
