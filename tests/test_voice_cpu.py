"""The voice-activity and end-of-turn rule on the host (dmel_codec_amd/utils/voice.py), the part that needs no GPU: the config's
refusals, the fresh state, split invariance of scan(), the defaults on synthetic clips through the oracle's log-mel, the refusals of
the C entry dmel_voice_items (fake pointers, never read) and the pool's bookkeeping: open(voice=), the `voice` key and segment of a
snapshot, and both refusals."""
import copy
import ctypes as C
import dataclasses
import io
import math

import pytest
import torch

from dmel_codec_amd.models.stream_park import SessionSnapshot, dense_layout
from dmel_codec_amd.utils import voice
from dmel_codec_amd.utils.voice import VoiceConfig
from oracle import ref_cpu


# ------------------------------------------------------------------------------------------------------------ the config
def test_defaults_are_the_documented_ones():
    c = VoiceConfig()
    assert dataclasses.astuple(c) == (1.5, -10.0, 0.1, 0.02, 0.002, None, 4, 3, 47)
    assert c.fparams() == (1.5, -10.0, 0.1, 0.02, 0.002) and c.iparams(80) == (0, 80, 4, 3, 47)
    assert VoiceConfig(bands=(3, 9), min_bands=6).iparams(100) == (3, 9, 6, 3, 47)
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.threshold = 2.0
    assert VoiceConfig.from_dict(c.as_dict()) == c
    d = VoiceConfig(bands=(2, 70), rise=1).as_dict()
    assert d["bands"] == [2, 70] and VoiceConfig.from_dict(d) == VoiceConfig(bands=(2, 70), rise=1.0)
    assert voice.as_config(None) is None and voice.as_config(False) is None and voice.as_config(True) == c and voice.as_config(c) is c
    with pytest.raises(ValueError):
        voice.as_config("yes")


@pytest.mark.parametrize("bad", [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=math.inf), dict(threshold=math.nan),
                                 dict(min_level=math.nan), dict(min_level=-math.inf), dict(min_level="low"), dict(fall=0.0),
                                 dict(fall=1.5), dict(rise=0.0), dict(rise=1.0001), dict(rise=math.nan), dict(rise_speech=-0.1),
                                 dict(rise_speech=1.5), dict(rise_speech=True), dict(bands=(5, 5)), dict(bands=(-1, 4)),
                                 dict(bands=(0, 129)), dict(bands=(1.0, 4)), dict(bands=(1, 2, 3)), dict(bands=7), dict(min_bands=0),
                                 dict(min_bands=2.0), dict(attack_frames=0), dict(attack_frames=2 ** 20 + 1), dict(release_frames=0),
                                 dict(release_frames=2 ** 20 + 1), dict(release_frames=True)])
def test_config_refuses(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        VoiceConfig(**bad)


def test_config_refuses_what_does_not_fit_the_transform():
    VoiceConfig(rise=1.0, fall=1.0, rise_speech=0.0, attack_frames=2 ** 20, release_frames=2 ** 20, min_bands=80).window(80)
    with pytest.raises(ValueError, match="min_bands"):
        VoiceConfig(min_bands=81).window(80)
    with pytest.raises(ValueError, match="bands"):
        VoiceConfig(bands=(10, 81)).window(80)
    with pytest.raises(ValueError, match="min_bands"):
        VoiceConfig(bands=(10, 13)).window(80)                              # the default 4 bands of a window of 3
    assert VoiceConfig(bands=(10, 14)).window(80) == (10, 14)
    for n in (0, 129, 80.0, True):
        with pytest.raises(ValueError, match="n_mels"):
            VoiceConfig().window(n)
    with pytest.raises(ValueError):
        voice.scan(torch.zeros(80, 3, dtype=torch.float64), VoiceConfig())
    with pytest.raises(ValueError):
        voice.scan(torch.zeros(80, 3), VoiceConfig(), state=torch.zeros(80 + 7, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------ the state
def test_a_zeroed_row_is_the_fresh_state():
    cfg = VoiceConfig()
    z = voice.fresh_state(7)
    assert z.dtype == torch.int32 and tuple(z.shape) == (15,) and not z.any()
    st, flags, counts = voice.scan(torch.zeros(7, 0), VoiceConfig(min_bands=1))       # no frame: nothing is initialised yet
    assert torch.equal(st, z) and flags.numel() == 0 and counts.numel() == 0
    rep = voice.report(z, hop=256, sample_rate=24000)
    assert (rep.speaking, rep.frames, rep.speech_start, rep.speech_end, rep.starts, rep.active_frames) == (False, 0, None, None, 0, 0)
    assert rep.silence_frames == 0 and not rep.end_of_turn
    # the first frame initialises the floors with itself (clamped at min_level) and start = end = -1; no band exceeds its own level
    col = torch.tensor([[-11.5], [-10.0], [-9.999], [0.0], [3.0], [-20.0], [1e-3]])
    st, flags, counts = voice.scan(col, VoiceConfig(min_bands=1))
    assert torch.equal(st[:7].view(torch.float32), torch.tensor([-10.0, -10.0, -9.999, 0.0, 3.0, -10.0, 1e-3]))
    assert st[7:].tolist() == [0, 0, 1, -1, -1, 0, 0, 0] and flags.tolist() == [0] and counts.tolist() == [0]
    assert z.tolist() == [0] * 15                                           # the state handed in is not modified
    # the second frame: the floor falls by `fall`, rises by `rise`; a band under min_level never exceeds
    st2, flags, counts = voice.scan(torch.tensor([[5.0], [-9.0], [-9.999], [-1.0], [6.0], [5.0], [1e-3]]), VoiceConfig(min_bands=1), st)
    f32 = torch.float32
    a, r = torch.tensor(0.1, dtype=f32), torch.tensor(0.02, dtype=f32)
    t = lambda v: torch.tensor(v, dtype=f32)
    expect = torch.stack([t(-10.0) + r * (t(5.0) - t(-10.0)), t(-10.0) + r * (t(-9.0) - t(-10.0)), t(-9.999), t(0.0) + a * (t(-1.0) - t(0.0)),
                          t(3.0) + r * (t(6.0) - t(3.0)), t(-10.0) + r * (t(5.0) - t(-10.0)), t(1e-3)])
    assert torch.equal(st2[:7].view(f32), expect)
    assert counts.tolist() == [3] and flags.tolist() == [1] and st2[7:].tolist() == [0, 1, 2, -1, -1, 0, 1, 0]
    # attack 3: the third active frame in a row switches to speech, dated at the first of the three
    loud = torch.tensor([[5.0], [-9.0], [-9.999], [-1.0], [6.0], [5.0], [1e-3]]).repeat(1, 2)
    st3, flags, _ = voice.scan(loud, VoiceConfig(min_bands=1), st2)
    assert flags.tolist() == [1, 3] and st3[7:].tolist() == [1, 0, 4, 1, -1, 1, 3, 0]
    rep = voice.report(st3, hop=256, sample_rate=24000)
    assert rep.speaking and rep.speech_start == 1 and rep.speech_end is None and rep.silence_frames == 0 and not rep.end_of_turn
    assert rep.samples(rep.speech_start) == 256 and rep.seconds(3) == 3 * 256 / 24000
    # release 2: two quiet frames end the turn, dated at the first quiet one
    st4, flags, _ = voice.scan(torch.full((7, 3), -11.5), VoiceConfig(min_bands=1, release_frames=2), st3)
    assert flags.tolist() == [2, 0, 0] and st4[7:].tolist() == [0, 0, 7, 1, 4, 1, 3, 0]
    rep = voice.report(st4)
    assert not rep.speaking and rep.end_of_turn and rep.speech_end == 4 and rep.silence_frames == 3 and rep.frames == 7


def random_mel(n_mels, frames, seed):
    """log-mel in the codec's range with bursts in some bands and columns at the clamp value"""
    g = torch.Generator().manual_seed(seed)
    mel = torch.randn(n_mels, frames, generator=g) * 0.3 - 6.0
    for a in range(10, frames, 37):
        mel[torch.randperm(n_mels, generator=g)[:max(1, 2 * n_mels // 3)], a:a + 9] += 4.0 + torch.rand(1, generator=g)
    mel[:, 50:53] = math.log(1e-5)
    return mel.clamp_(min=math.log(1e-5)).contiguous()


@pytest.mark.parametrize("n_mels", [7, 80, 100, 128])
def test_any_split_of_the_frames_gives_the_bits_of_one_call(n_mels):
    mel = random_mel(n_mels, 130, n_mels)
    for cfg in (VoiceConfig(release_frames=10), VoiceConfig(bands=(1, n_mels - 1), min_bands=2, attack_frames=1, release_frames=5, rise_speech=0.0)):
        whole, flags, counts = voice.scan(mel, cfg)
        assert int(whole[n_mels + voice.I_STARTS]) >= 2 and flags.max() == 3 and flags.min() == 0          # the state machine moved
        for pieces in ((1, 63, 2, 64), (7,) * 18 + (4,)):
            assert sum(pieces) == 130
            st, fl, ct, at = None, [], [], 0
            for n in pieces:
                st, f, c = voice.scan(mel[:, at:at + n].contiguous(), cfg, st)
                fl.append(f), ct.append(c)
                at += n
            assert torch.equal(st, whole) and torch.equal(torch.cat(fl), flags) and torch.equal(torch.cat(ct), counts), pieces


# ------------------------------------------------------------------------------------------------------------ the defaults on synthetic clips
SR, N_FFT, HOP = 24000, 1024, 256


def clip(noise_dbfs, burst):
    """4 s at 24 kHz: white noise at noise_dbfs (None: digital silence), a 20-harmonic burst of 150 Hz over [0.75, 1.5) s on top"""
    torch.manual_seed(0)
    n = 4 * SR
    x = torch.zeros(n) if noise_dbfs is None else torch.randn(n) * 10.0 ** (noise_dbfs / 20.0)
    if burst:
        t = torch.arange(n, dtype=torch.float64) / SR
        b = sum(torch.sin(2 * math.pi * 150 * k * t) / k for k in range(1, 21)) * 0.1
        on = (t >= 0.75) & (t < 1.5)
        x = x + torch.where(on, b, torch.zeros_like(b)).float()
    return x


@pytest.mark.parametrize("n_mels", [80, 100])
@pytest.mark.parametrize("noise", [-60, -40, -30, None])
def test_defaults_find_a_harmonic_burst_over_noise(noise, n_mels):
    cfg = VoiceConfig()
    mel = ref_cpu.stft_logmel(clip(noise, True)[None], SR, N_FFT, N_FFT, HOP, n_mels, 0.0, 12000.0)[0].contiguous()
    st, flags, counts = voice.scan(mel, cfg)
    rep = voice.report(st, HOP, SR)
    print(f"noise {noise} dBFS, {n_mels} bands: start {rep.speech_start}, end {rep.speech_end}, starts {rep.starts}, "
          f"count in the burst {int(counts[75:135].min())} .. {int(counts[75:135].max())}, outside at most "
          f"{int(torch.cat([counts[:66], counts[146:]]).max())}")
    assert rep.frames == mel.shape[1] == 4 * SR // HOP
    assert rep.starts == 1 and not rep.speaking and rep.end_of_turn
    # 4 = n_fft / hop: the frames that straddle an edge of the burst (0.75 s is frame 70.3, 1.5 s frame 140.6)
    assert abs(rep.speech_start - 70) <= 4 and abs(rep.speech_end - 141) <= 4
    # away from the straddling frames the band count stays under min_bands
    assert int(torch.cat([counts[:66], counts[146:]]).max()) <= 2 < cfg.min_bands
    assert rep.silence_frames == rep.frames - rep.speech_end
    # the same clip without the burst: nothing starts
    quiet = ref_cpu.stft_logmel(clip(noise, False)[None], SR, N_FFT, N_FFT, HOP, n_mels, 0.0, 12000.0)[0].contiguous()
    st, flags, counts = voice.scan(quiet, cfg)
    rep = voice.report(st, HOP, SR)
    assert rep.starts == 0 and not rep.speaking and not rep.end_of_turn and rep.speech_start is None and int(flags.max()) <= 1


# ------------------------------------------------------------------------------------------------------------ the C entry
def test_voice_entry_refuses_before_it_launches():
    """dmel_voice_items checks its host tables before anything touches the device: the "device" pointers here are never read"""
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    assert len(_lib.PROTOTYPES["dmel_voice_items"][1]) == 14
    fake = 1 << 20
    good_f, good_i = (1.5, -10.0, 0.1, 0.02, 0.002), (0, 80, 4, 3, 47)

    def call(frames, fp=None, ip=None, n_mels=80, S=None, mel=fake, state=fake + (1 << 16), pitch=200, table=fake + (1 << 18), strides=(80 * 200, 200)):
        n = len(frames)
        fp = [good_f] * n if fp is None else fp
        ip = [good_i] * n if ip is None else ip
        rc = lib.dmel_voice_items(mel, strides[0], strides[1], n_mels, n if S is None else S, (C.c_int64 * n)(*frames),
                                  (C.c_float * (5 * n))(*[v for r in fp for v in r]), (C.c_int32 * (5 * n))(*[v for r in ip for v in r]),
                                  state, None, None, pitch, table, None)
        return rc, lib.dmel_last_error().decode(errors="replace")

    def f_with(k, v):
        return [good_f, good_f[:k] + (v,) + good_f[k + 1:]]

    def i_with(k, v):
        return [good_i, good_i[:k] + (v,) + good_i[k + 1:]]

    for kw, words in ((dict(frames=[5, -1]), ("item 1", "frames")),
                      (dict(frames=[5, 1 << 31]), ("item 1", "frames")),
                      (dict(frames=[201, 5]), ("item 0", "pitch")),
                      (dict(frames=[5, 5], fp=f_with(0, 0.0)), ("item 1", "threshold")),
                      (dict(frames=[5, 5], fp=f_with(0, math.inf)), ("item 1", "finite")),
                      (dict(frames=[5, 5], fp=f_with(1, math.nan)), ("item 1", "finite")),
                      (dict(frames=[5, 5], fp=f_with(2, 0.0)), ("item 1", "fall")),
                      (dict(frames=[5, 5], fp=f_with(2, 1.5)), ("item 1", "fall")),
                      (dict(frames=[5, 5], fp=f_with(3, 0.0)), ("item 1", "rise")),
                      (dict(frames=[5, 5], fp=f_with(4, -0.5)), ("item 1", "rise_speech")),
                      (dict(frames=[5, 5], fp=f_with(4, 1.5)), ("item 1", "rise_speech")),
                      (dict(frames=[5, 5], ip=i_with(0, -1)), ("item 1", "bands")),
                      (dict(frames=[5, 5], ip=i_with(0, 80)), ("item 1", "bands")),
                      (dict(frames=[5, 5], ip=i_with(1, 81)), ("item 1", "bands")),
                      (dict(frames=[5, 5], ip=i_with(2, 0)), ("item 1", "min_bands")),
                      (dict(frames=[5, 5], ip=i_with(2, 81)), ("item 1", "min_bands")),
                      (dict(frames=[5, 5], ip=i_with(3, 0)), ("item 1", "attack_frames")),
                      (dict(frames=[5, 5], ip=i_with(4, (1 << 20) + 1)), ("item 1", "release_frames"))):
        rc, msg = call(**kw)
        assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
    for S in (0, -1, 65536):
        rc, msg = call([5], S=S)
        assert rc == -1 and "65535" in msg, (S, rc, msg)
    for n_mels in (0, 129):
        rc, msg = call([5], n_mels=n_mels)
        assert rc == -1 and "mel bands" in msg, (n_mels, rc, msg)
    for kw in (dict(mel=None), dict(state=None), dict(table=None), dict(mel=fake + 2), dict(state=fake + 1), dict(table=fake + 3),
               dict(strides=(-1, 200)), dict(strides=(16000, -200))):
        assert call([5], **kw)[0] == -1, kw
    # idle items: their parameters are not looked at, and a call of idle items only launches nothing
    nan = (math.nan,) * 5
    assert call([0, 0], fp=[nan, nan], ip=[(9, 9, 9, 0, 0)] * 2, pitch=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the pool
@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, residual_channels=70, vocoder=None)


def refused(pool, snap, match=None):
    before = (pool.open_slots, copy.deepcopy(pool.origin), list(pool.vcfg))
    with pytest.raises(ValueError, match=match):
        pool.restore([snap])
    assert (pool.open_slots, pool.origin, pool.vcfg) == before              # a refused restore takes no slot


def test_pool_bookkeeping_of_sessions_with_detection(codec):
    cfg = VoiceConfig(bands=(4, 60), min_bands=3, release_frames=20)
    plain_pool = codec.encode_sessions(2, max_push_samples=4096)
    pool = codec.encode_sessions(3, max_push_samples=4096, voice=True)
    assert not plain_pool.voice_on and pool.voice_on and plain_pool.cap == pool.cap
    # open(voice=) on a pool built without: refused, no slot taken
    for v in (True, cfg):
        with pytest.raises(ValueError, match="voice=True"):
            plain_pool.open(voice=v)
    assert plain_pool.open_slots == [] and plain_pool.voice() == {}
    with pytest.raises(ValueError, match="min_bands"):
        pool.open(voice=VoiceConfig(bands=(70, 80), min_bands=11))
    with pytest.raises(ValueError, match="bands"):
        pool.open(voice=VoiceConfig(bands=(70, 81)))
    with pytest.raises(ValueError):
        pool.open(voice="on")
    with pytest.raises(ValueError):
        codec.encode_sessions(2, voice=cfg)                                 # the pool's option is a bool: configs belong to sessions
    assert pool.open_slots == []
    a, b, c = pool.open(voice=True), pool.open(), pool.open(voice=cfg)
    assert pool.vcfg == [VoiceConfig(), None, cfg]
    # nothing was pushed: reports of no frames, without buffers or a device
    reps = pool.voice()
    assert set(reps) == {a, c} and pool.buf is None
    assert all(r == voice.report(voice.fresh_state(80), pool.geo.hop, pool.codec_rate) and r.frames == 0 for r in reps.values())
    assert reps[a].hop == 256 and reps[a].sample_rate == pool.codec_rate
    with pytest.raises(ValueError, match="voice"):
        pool.voice_frames(b)
    # the snapshot: the key only where detection is on; a fresh session owns the zeroed row, so no words
    snaps = pool.snapshot([a, b, c])
    assert snaps[a].meta["voice"] == VoiceConfig().as_dict() and snaps[c].meta["voice"] == cfg.as_dict() and "voice" not in snaps[b].meta
    assert snaps[b].meta == plain_pool.snapshot([plain_pool.open()])[0].meta  # without detection: the snapshot of a pool without the option
    plain_pool.drop(0)
    assert all(sn.nbytes == 0 and sn.meta["layout"] == [] for sn in snaps.values())
    buf = io.BytesIO()
    torch.save(snaps[c].cpu().as_dict(), buf)
    buf.seek(0)
    back = SessionSnapshot.from_dict(torch.load(buf, weights_only=True))
    assert back.meta == snaps[c].meta
    # the layout of a session that has seen frames: one tail segment ("voice", 1, n_mels + 8) behind the others
    meta = copy.deepcopy(snaps[c].meta)
    meta["schedule"]["frames"] = 1
    shapes = pool._park_shapes(meta)
    assert shapes[-1] == ("voice", 1, 88) and shapes[:-1] == pool._park_shapes({k: v for k, v in meta.items() if k != "voice"})
    assert dense_layout(shapes)[0][-1] == ["voice", 1, 88, 0]
    # a pool without the option refuses the key; a voice pool takes snapshots with and without it
    refused(plain_pool, back, "voice=True")
    refused(plain_pool, snaps[a], "voice=True")
    assert plain_pool.restore([snaps[b]]) == [0]
    other = codec.encode_sessions(4, max_push_samples=1000, voice=True)
    assert other.restore([back, snaps[b], snaps[a]]) == [0, 1, 2] and other.vcfg == [cfg, None, VoiceConfig(), None]
    assert set(other.voice()) == {0, 2}
    # a config that is none, or does not fit the transform
    bad = SessionSnapshot(dict(back.meta, voice=dict(back.meta["voice"], threshold=-1.0)), back.blob)
    refused(other, bad, "threshold")
    refused(other, SessionSnapshot(dict(back.meta, voice=dict(back.meta["voice"], loudness=3)), back.blob), "VoiceConfig")
    refused(other, SessionSnapshot(dict(back.meta, voice=dict(back.meta["voice"], bands=[4, 81])), back.blob), "bands")
    # drop forgets the detector with the session
    other.drop(0)
    assert set(other.voice()) == {2}
    with pytest.raises(ValueError):
        other.voice_frames(0)
