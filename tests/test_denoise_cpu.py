"""The noise suppression rule on the host (dmel_codec_amd/utils/denoise.py): reconstruction, chunk invariance, silence, subnormal
squares, what the defaults do to noise, tones, a floor that jumps and a harmonic signal in noise (synthetic signals only), the report,
the refusals of the C entry, and the pool's bookkeeping.  Nothing here needs a GPU."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot, dense_layout
from dmel_codec_amd.utils import denoise
from dmel_codec_amd.utils.denoise import DenoiseConfig

RATE = 24000


def bits(t):
    return t.contiguous().view(torch.int32)


def power(a):
    return float(np.mean(np.asarray(a, dtype=np.float64) ** 2))


def db(a, b):
    return 10.0 * math.log10(power(a) / power(b))


def white(n, rms, seed):
    return np.random.default_rng(seed).standard_normal(n) * rms


def harmonic(n, start, seed=1):
    """voiced-like: 29 harmonics of a 120 Hz line with vibrato and tremolo, amplitudes 1 / k, peak 0.5, from sample `start` on"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    phase = 2 * np.pi * np.cumsum(120.0 * (1 + 0.02 * np.sin(2 * np.pi * 5 * t))) / RATE
    s = sum(np.sin(k * phase + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 30)) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t))
    s = s / np.abs(s).max() * 0.5
    s[:start] = 0.0
    return s


def scan_in(x, cfg, sizes):
    state, ys, pi, po, at = None, [], [], [], 0
    for m in sizes:
        y, state, a, b = denoise.scan(x[at:at + m], cfg, state)
        ys.append(y), pi.append(a), po.append(b)
        at += m
    assert at == x.shape[0]
    return torch.cat(ys), state, torch.cat(pi), torch.cat(po)


def wola64(x, N):
    """the rule with every gain 1 in float64: window, FFT, inverse, window, overlap-add, delayed by N"""
    H = N // 2
    w = np.sin(np.pi * (np.arange(N) + 0.5) / N)
    xp = np.concatenate([np.zeros(H), x.astype(np.float64)])
    y = np.zeros(xp.shape[0] + N)
    for k in range((x.shape[0]) // H):
        y[k * H:k * H + N] += np.fft.irfft(np.fft.rfft(xp[k * H:k * H + N] * w), N) * w
    y[:H] = 0.0                                                              # the hop in front of the stream
    return np.concatenate([np.zeros(H), y])[:x.shape[0]]                       # y is on [-H, ..): out[p] = y[p - N]


# ------------------------------------------------------------------------------------------------------------ the config
def test_defaults_are_the_documented_ones():
    c = DenoiseConfig()
    assert (c.frame_samples, c.hop, c.alpha, c.track, c.track_ratio, c.creep, c.floor_gain, c.eps, c.learn_frames) == \
        (512, 256, 0.96, 0.05, 6.0, 1.002, 0.126, 1e-20, 16)
    assert c.delay(24000) == 512 / 24000 and DenoiseConfig(frame_samples=256).delay(8000) == 0.032
    assert denoise.STATE_WORDS == 3092 and denoise.HEADER_WORDS == 16 and denoise.TABLE_WORDS == 16 and denoise.TRANSFORM_WORDS == 3072
    assert DenoiseConfig.from_dict(c.as_dict()) == c
    fp = c.fparams()
    assert len(fp) == 8 and fp[1] == float(np.float32(1.0 - 0.96)) and fp[7] == 1.0 / 512
    assert denoise.as_config(None) is None and denoise.as_config(False) is None and denoise.as_config(True) == c and denoise.as_config(c) is c
    assert denoise.max_frames(1, 512) == 1 and denoise.max_frames(256, 512) == 1 and denoise.max_frames(257, 512) == 2
    t = denoise.transform_table()
    assert t.shape == (3072,) and t.dtype == torch.float32 and float(t[1024]) == 1.0 and float(t[2048]) == 1.0 and float(t[2560]) == 0.0


@pytest.mark.parametrize("bad", [dict(frame_samples=32), dict(frame_samples=2048), dict(frame_samples=96), dict(frame_samples=512.0),
                                 dict(frame_samples=True), dict(alpha=1.0), dict(alpha=-0.1), dict(track=0.0), dict(track=1.5),
                                 dict(track_ratio=0.5), dict(creep=0.99), dict(creep=2.5), dict(floor_gain=0.0), dict(floor_gain=1.5),
                                 dict(eps=0.0), dict(eps=math.nan), dict(alpha=math.inf), dict(learn_frames=0), dict(learn_frames=5000),
                                 dict(learn_frames=2.0), dict(alpha="0.9")])
def test_config_refuses(bad):
    with pytest.raises(ValueError):
        DenoiseConfig(**bad)


def test_as_config_refuses_what_is_no_config():
    for v in ("on", 1, dict(alpha=0.5)):
        with pytest.raises(ValueError):
            denoise.as_config(v)
    with pytest.raises(ValueError):
        DenoiseConfig().delay(0)


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("N", [64, 1024])
def test_unit_gain_returns_the_input_delayed_by_a_frame(N):
    """floor_gain = 1 makes every gain 1.  The float64 evaluation of the rule reconstructs to 2e-15; the fp32 rule deviated from it
    by 1.8e-7 at most on this input (|x| up to 1.3) for N = 64 and 2.4e-7 for N = 1024: the bound is four times the larger."""
    x = (white(8 * N + 7, 0.3, N)).astype(np.float32)
    ref = wola64(x, N)
    whole = x.shape[0] // (N // 2) * (N // 2)                                 # outputs the completed frames have reached
    assert np.abs(ref[N:whole] - x[:whole - N].astype(np.float64)).max() < 2e-15 and not ref[:N].any()
    y, state, pi, po = denoise.scan(x, DenoiseConfig(frame_samples=N, floor_gain=1.0))
    y = y.numpy()
    assert not y[:N].any()
    err = float(np.abs(y[:whole] - ref[:whole]).max())
    print(f"N = {N}: largest deviation from float64 {err:.3e}")
    assert err < 9.54e-7
    assert torch.equal(bits(pi), bits(po)) and pi.shape[0] == x.shape[0] // (N // 2)      # G = 1: power_out is power_in


@pytest.mark.parametrize("cfg", [DenoiseConfig(), DenoiseConfig(frame_samples=64, learn_frames=3, alpha=0.9),
                                 DenoiseConfig(frame_samples=1024, learn_frames=2, track=0.2)])
def test_any_cut_of_the_samples_gives_the_bits_of_one_call(cfg):
    H = cfg.hop
    sizes = [1, H - 1, H, H + 1, 3 * H + 5, 1, 1, 2 * H, 7]
    x = white(sum(sizes), 0.05, H)
    x[len(x) // 2:] += 0.3 * np.sin(2 * np.pi * 0.07 * np.arange(len(x) - len(x) // 2))
    x = x.astype(np.float32)
    y, state, pi, po = denoise.scan(x, cfg)
    assert int(state[denoise.I_FRAMES]) == len(x) // H and int(state[denoise.I_FILL]) == len(x) % H
    for cut in (sizes, sizes[::-1], [len(x) - 1, 1]):
        y2, s2, pi2, po2 = scan_in(x, cfg, cut)
        assert torch.equal(bits(y2), bits(y)) and torch.equal(s2, state) and torch.equal(bits(pi2), bits(pi)) and torch.equal(bits(po2), bits(po))
    assert float(po.sum()) < float(pi.sum())


def test_no_sample_changes_nothing_and_neither_input_is_modified():
    x = white(700, 0.1, 0).astype(np.float32)
    keep = x.copy()
    y, state, _, _ = denoise.scan(x, DenoiseConfig(frame_samples=64))
    before = state.clone()
    y0, s0, a, b = denoise.scan(np.zeros(0, dtype=np.float32), DenoiseConfig(frame_samples=64), state)
    assert y0.shape == (0,) and a.shape == (0,) and b.shape == (0,) and torch.equal(s0, before) and torch.equal(state, before)
    assert np.array_equal(x, keep)
    with pytest.raises(ValueError):
        denoise.scan(x.astype(np.float64), DenoiseConfig())
    with pytest.raises(ValueError):
        denoise.scan(x, DenoiseConfig(), torch.zeros(16, dtype=torch.int32))
    bad = denoise.fresh_state()
    bad[denoise.I_FILL] = 32
    with pytest.raises(ValueError, match="open hop"):
        denoise.scan(x, DenoiseConfig(frame_samples=64), bad)


def test_digital_silence_gives_zeros_and_leaves_the_estimate_alone():
    cfg = DenoiseConfig(frame_samples=128, learn_frames=4)
    zeros = np.zeros(5 * 64 + 9, dtype=np.float32)
    y, state, pi, po = denoise.scan(zeros, cfg)
    assert not y.any() and not pi.any() and not po.any() and pi.shape[0] == 5
    fresh = denoise.fresh_state()
    fresh[denoise.I_FRAMES], fresh[denoise.I_FILL] = 5, 9                      # only the framing counters moved
    assert torch.equal(state, fresh)
    # behind noise: the estimate, the smoothed SNR, the learnt count and the sums stay; the overlap tail drains and zeros follow
    x = np.concatenate([white(64 * 9, 0.05, 2), np.zeros(64)]).astype(np.float32)     # the last frame still holds the noise's last hop
    _, s1, pi1, _ = denoise.scan(x, cfg)
    y2, s2, pi2, po2 = denoise.scan(np.zeros(64 * 6, dtype=np.float32), cfg, s1)
    keep = list(range(denoise.I_LEARNED, denoise.HEADER_WORDS)) + list(range(denoise.O_NZ, denoise.STATE_WORDS))
    assert torch.equal(s2[keep], s1[keep]) and int(s2[denoise.I_FRAMES]) == int(s1[denoise.I_FRAMES]) + 6
    assert float(pi1[-1]) > 0 and not pi2.any() and not po2.any()
    assert y2[:64 * 2].any() and not y2[64 * 2:].any() and not s2[denoise.O_RAW:denoise.O_NZ].any()


def test_squares_that_are_subnormal_give_a_finite_and_repeatable_output():
    x = white(3000, 1e-20, 3).astype(np.float32)
    a = denoise.scan(x, DenoiseConfig())
    b = denoise.scan(x, DenoiseConfig())
    assert torch.isfinite(a[0]).all() and torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])
    assert not a[2].any() and not a[0].any()                                  # every bin power is below TINY: the frames count as silent
    # just above the clamp the rule runs: finite, repeatable, and the noise estimate is a normal number
    x = white(3000, 1e-13, 3).astype(np.float32)
    a, b = denoise.scan(x, DenoiseConfig()), denoise.scan(x, DenoiseConfig())
    assert torch.isfinite(a[0]).all() and torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and float(a[2].min()) > 0
    assert denoise.report(a[1]).noise_power > 1e-30


def test_white_noise_is_attenuated_towards_the_gain_floor():
    """-40 dBFS white noise, the defaults (a floor of -18 dB): over 0.4 s behind 1.5 s the output lies at least 15 dB below the input
    and no more than the floor allows"""
    x = white(int(1.9 * RATE), 0.01, 4).astype(np.float32)
    y, state, pi, po = denoise.scan(x, DenoiseConfig())
    a, b = int(1.5 * RATE), int(1.9 * RATE)
    att = db(x[a - 512:b - 512], y[a:b].numpy())
    print(f"attenuation of white noise {att:.2f} dB")
    assert 15.0 <= att <= -20 * math.log10(0.126) + 0.01
    rep = denoise.report(state)
    assert not rep.learning and rep.learned == 16 and rep.frames == len(x) // 256 and 10.0 < rep.attenuation_db < 18.0


def test_a_tone_that_starts_abruptly_on_quiet_noise_is_kept():
    """-60 dBFS noise from the first sample, a 697 Hz tone at 0.1 peak from 0.5 s on: 1.9 s later it still has 0.9 of its RMS"""
    n = int(2.8 * RATE)
    t = np.arange(n) / RATE
    x = (white(n, 0.001, 5) + 0.1 * np.sin(2 * np.pi * 697 * t) * (t >= 0.5)).astype(np.float32)
    y = denoise.scan(x, DenoiseConfig())[0].numpy()
    a, b = int(2.4 * RATE), int(2.8 * RATE)
    kept = math.sqrt(power(y[a:b]) / power(x[a - 512:b - 512]))
    print(f"tone kept {kept:.4f}")
    assert kept >= 0.9


def test_a_noise_floor_that_jumps_by_20_db_is_learnt_again_within_3_s():
    n = int(4.5 * RATE)
    x = white(n, 0.003, 6)
    x[int(1.5 * RATE):] *= 10.0
    x = x.astype(np.float32)
    y = denoise.scan(x, DenoiseConfig())[0].numpy()
    a, b = int(4.1 * RATE), int(4.5 * RATE)                                   # the last 0.4 s of the 3 s behind the jump
    att = db(x[a - 512:b - 512], y[a:b])
    print(f"attenuation {att:.2f} dB at 2.6 .. 3.0 s behind the jump")
    assert att >= 10.0


def test_a_harmonic_signal_in_noise_at_0_db_gains_3_db_of_snr():
    """white noise from the first sample, the harmonic signal from 0.5 s on at the noise's power: against the clean signal delayed
    by N the output SNR over the last 2 s exceeds the input SNR by at least 3 dB at N = 512"""
    n = int(3.0 * RATE)
    s = harmonic(n, RATE // 2)
    noise = white(n, 1.0, 7)
    noise *= math.sqrt(power(s[RATE:]) / power(noise))
    x = (s + noise).astype(np.float32)
    y = denoise.scan(x, DenoiseConfig())[0].numpy().astype(np.float64)
    a = RATE
    ref = s[a - 512:n - 512]
    snr_in = 10 * math.log10(power(ref) / power(x[a - 512:n - 512] - ref))
    snr_out = 10 * math.log10(power(ref) / power(y[a:] - ref))
    print(f"SNR in {snr_in:.2f} dB, out {snr_out:.2f} dB")
    assert abs(snr_in) < 0.1 and snr_out >= snr_in + 3.0


# ------------------------------------------------------------------------------------------------------------ the report
def test_report_of_a_fresh_row_and_of_a_stream():
    rep = denoise.report(denoise.fresh_state())
    assert rep == denoise.DenoiseReport(frames=0, total_samples=0, learned=0, learning=True, power_in=0.0, power_out=0.0, attenuation_db=0.0,
                                        noise_power=0.0, delay_samples=512, sample_rate=24000)
    assert rep.seconds(93) == 94 * 256 / 24000
    cfg = DenoiseConfig(frame_samples=128, learn_frames=5)
    x = white(64 * 20 + 13, 0.05, 8).astype(np.float32)
    _, state, pi, po = denoise.scan(x, cfg)
    rep = denoise.report(state, 128, 8000, 5)
    assert (rep.frames, rep.total_samples, rep.learned, rep.learning, rep.delay_samples, rep.sample_rate) == (20, len(x), 5, False, 128, 8000)
    assert rep == denoise.report(state[:denoise.HEADER_WORDS], 128, 8000, 5)   # the header is all it reads
    f32 = np.float32
    acc_in = acc_out = f32(0)
    for a, b in zip(pi.numpy(), po.numpy()):
        acc_in, acc_out = f32(acc_in + a), f32(acc_out + b)
    assert rep.power_in == float(acc_in) and rep.power_out == float(acc_out)
    assert abs(rep.attenuation_db - 10 * math.log10(float(acc_in) / float(acc_out))) < 1e-12
    nz = state[denoise.O_NZ:denoise.O_NZ + 65].view(torch.float32).numpy()
    assert rep.noise_power == float(denoise._sum(nz)) and abs(rep.noise_power - float(nz.astype(np.float64).sum())) < 1e-5 * rep.noise_power
    assert denoise.report(state, 128, 8000, 64).learning


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_denoise_entry_refuses_before_it_launches():
    """dmel_denoise_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_denoise_items"][1]) == 15
    fake = 1 << 20
    good = DenoiseConfig().fparams()

    def call(n_new, first=None, N=None, learn=None, fp=None, S=None, samples=fake, stride=9000, state=fake + (1 << 16),
             pin=fake + (1 << 17), pout=fake + (1 << 18), pitch=100, transform=fake + (1 << 19), table=fake + (1 << 20)):
        n = len(n_new)
        first = [0] * n if first is None else first
        N = [512] * n if N is None else N
        learn = [16] * n if learn is None else learn
        fp = [good] * n if fp is None else fp
        rc = lib.dmel_denoise_items(samples, stride, n if S is None else S, (C.c_int64 * n)(*first), (C.c_int64 * n)(*n_new),
                                    (C.c_int32 * n)(*N), (C.c_int32 * n)(*learn), (C.c_float * (8 * n))(*[v for r in fp for v in r]),
                                    state, pin, pout, pitch, transform, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    def with_(k, v):
        return [good, good[:k] + (v,) + good[k + 1:]]

    cases = [(dict(n_new=[5, -1]), ("item 1", "new samples")),
             (dict(n_new=[5, 1 << 30]), ("item 1", "new samples")),
             (dict(n_new=[5, 5], first=[0, -1]), ("item 1", "first column")),
             (dict(n_new=[5, 5], first=[1 << 30, 0]), ("item 0", "first column")),
             (dict(n_new=[5, 5], N=[512, 32]), ("item 1", "frame")),
             (dict(n_new=[5, 5], N=[2048, 512]), ("item 0", "frame")),
             (dict(n_new=[5, 5], N=[512, 96]), ("item 1", "power of two")),
             (dict(n_new=[5, 5], N=[512, 0]), ("item 1", "frame")),
             (dict(n_new=[256 * 100 + 1, 5]), ("item 0", "pitch")),
             (dict(n_new=[5, 32 * 100 + 1], N=[512, 64]), ("item 1", "pitch")),
             (dict(n_new=[5, 5], learn=[16, 0]), ("item 1", "learn_frames")),
             (dict(n_new=[5, 5], learn=[4097, 16]), ("item 0", "learn_frames")),
             (dict(n_new=[5, 5], fp=with_(0, 1.0)), ("item 1", "alpha")),
             (dict(n_new=[5, 5], fp=with_(1, 0.0)), ("item 1", "oma")),
             (dict(n_new=[5, 5], fp=with_(2, 0.0)), ("item 1", "track")),
             (dict(n_new=[5, 5], fp=with_(2, 1.5)), ("item 1", "track")),
             (dict(n_new=[5, 5], fp=with_(3, 0.5)), ("item 1", "track_ratio")),
             (dict(n_new=[5, 5], fp=with_(4, 0.99)), ("item 1", "creep")),
             (dict(n_new=[5, 5], fp=with_(4, 2.5)), ("item 1", "creep")),
             (dict(n_new=[5, 5], fp=with_(5, 0.0)), ("item 1", "floor_gain")),
             (dict(n_new=[5, 5], fp=with_(5, 1.5)), ("item 1", "floor_gain")),
             (dict(n_new=[5, 5], fp=with_(6, 0.0)), ("item 1", "eps")),
             (dict(n_new=[5, 5], fp=with_(7, 1.0 / 256)), ("item 1", "rN")),
             (dict(n_new=[5, 5], N=[512, 256]), ("item 1", "rN"))]
    for k in range(8):
        for v in (-1.0, math.inf, math.nan):
            cases.append((dict(n_new=[5, 5], fp=with_(k, v)), ("item 1", f"float parameter {k}")))
    for kw, words in cases:
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for S in (0, -1, 65536):
        rc, msg = call([5], S=S)
        assert rc == -1 and "65535" in msg, (S, rc, msg)
    for kw in (dict(samples=None), dict(state=None), dict(pin=None), dict(pout=None), dict(transform=None), dict(table=None),
               dict(samples=fake + 2), dict(state=fake + 1), dict(pin=fake + 2), dict(pout=fake + 1), dict(transform=fake + 2),
               dict(table=fake + 3), dict(stride=-1), dict(pitch=-1)):
        assert call([5], **kw)[0] == -1, kw
    # idle items: their parameters are not looked at, and a call of idle items only launches nothing
    nan = (math.nan,) * 8
    assert call([0, 0], first=[-5, -5], N=[0, 0], learn=[0, 0], fp=[nan, nan], pitch=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.ncfg))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.ncfg) == before              # a refused restore takes no slot


def test_pool_bookkeeping_of_sessions_with_a_suppressor(codec):
    cfg = DenoiseConfig(frame_samples=256, floor_gain=0.25)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, denoise=True)
    both = codec.encode_sessions(2, max_push_samples=4096, level=True, denoise=True)
    assert not plain_pool.denoise_on and pool.denoise_on and not pool.level_on and both.level_on and both.denoise_on and plain_pool.cap == pool.cap
    # open(denoise=) on a pool without rows: refused, no slot taken
    for v in (True, cfg):
        with pytest.raises(ValueError, match="denoise=True"):
            plain_pool.open(denoise=v)
    assert plain_pool.open_slots == [] and plain_pool.denoised() == {}
    with pytest.raises(ValueError):
        pool.open(denoise="on")
    with pytest.raises(ValueError):
        pool.open(denoise=dict(alpha=0.5))
    with pytest.raises(ValueError):
        codec.encode_sessions(2, denoise=cfg)                               # the pool's option is a bool: configs belong to sessions
    with pytest.raises(ValueError, match="level=True"):
        pool.open(level=True, denoise=True)                                 # the options are independent
    assert pool.open_slots == []
    a, b, c = pool.open(denoise=True), pool.open(), pool.open(denoise=cfg)
    assert pool.ncfg == [DenoiseConfig(), None, cfg]
    v = both.open(level=True, denoise=cfg)
    assert both.lcfg[v] is not None and both.ncfg[v] == cfg
    # nothing was pushed: reports of no sample, without buffers or a device
    reps = pool.denoised()
    assert set(reps) == {a, c} and pool.buf is None
    assert reps[a] == denoise.report(denoise.fresh_state(), 512, pool.codec_rate) and reps[c].delay_samples == 256 and reps[c].total_samples == 0
    with pytest.raises(ValueError, match="suppressor"):
        pool.denoise_frames(b)
    # the snapshot: the key only where a suppressor is on; a fresh session owns the zeroed row, so no words
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["denoise"] == DenoiseConfig().as_dict() and snaps[c].meta["denoise"] == cfg.as_dict() and "denoise" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without a suppressor: the snapshot of a pool without the option
    plain_pool.drop(0)
    assert all(sn.nbytes == 0 and sn.meta["layout"] == [] for sn in snaps.values())
    sv = both.snapshot([v])[v]
    assert sv.meta["denoise"] == cfg.as_dict() and "level" in sv.meta
    # the layout of a session that has seen samples: one tail segment ("denoise", 1, 3092) behind the others
    meta = copy.deepcopy(snaps[c].meta)
    meta["schedule"]["samples"] = 1
    shapes = pool._park_shapes(meta)
    assert shapes[-1] == ("denoise", 1, 3092) and shapes[:-1] == pool._park_shapes({k: x for k, x in meta.items() if k != "denoise"})
    assert dense_layout(shapes)[0][-1] == ["denoise", 1, 3092, 0]
    # a pool without the option refuses the key; a denoising pool takes snapshots with and without it
    refused(plain_pool, snaps[c], "denoise=True")
    refused(plain_pool, snaps[a], "denoise=True")
    assert plain_pool.restore([snaps[b]]) == [0]
    other = codec.encode_sessions(4, max_push_samples=1000, denoise=True)
    assert other.restore([snaps[c], snaps[b], snaps[a]]) == [0, 1, 2] and other.ncfg == [cfg, None, DenoiseConfig(), None]
    assert set(other.denoised()) == {0, 2}
    refused(other, SessionSnapshot(dict(snaps[c].meta, denoise=dict(snaps[c].meta["denoise"], creep=0.5)), snaps[c].blob), "creep")
    refused(other, SessionSnapshot(dict(snaps[c].meta, denoise=dict(snaps[c].meta["denoise"], comfort=3)), snaps[c].blob), "DenoiseConfig")
    refused(pool, sv, "level=True")                                         # the other option's rows are still needed
    other.drop(0)
    assert set(other.denoised()) == {2}
    with pytest.raises(ValueError):
        other.denoise_frames(0)
