"""dmel_voice_items on the GPU against the host rule (dmel_codec_amd/utils/voice.py: scan), bit for bit: floors (compared as int32),
the eight integers, flags and counts.  Five slots, one of them idle in every launch and the others idle in some; band counts on
both sides of the 64-lane split; 0, 1, 2, 63, 64, 65 and 130 frames per launch (one chunk of the kernel's LDS tile holds 64 frames);
an output pitch above the frames; one clip scanned in one launch and in the pieces 1, 63, 2, 64.  Idle rows and the bytes behind a
row's frames carry sentinels."""
import ctypes as C
import math

import pytest
import torch

from dmel_codec_amd.utils import voice
from dmel_codec_amd.utils.voice import VoiceConfig
from test_voice_cpu import random_mel

pytestmark = pytest.mark.gpu

S, IDLE, FRAMES = 5, 2, 200
# frames of slot s in launch j; slots 0 and 1 scan the same clip with the same config: in one launch, and in the pieces 1, 63, 2, 64
SCRIPT = {0: [130, 0, 65, 0], 1: [1, 63, 2, 64], 3: [63, 64, 1, 2], 4: [65, 2, 0, 130]}
SENTINEL_WORD, SENTINEL_BYTE = 0x7FC00123, 0xEE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def configs(n_mels):
    wide = (1, n_mels - 1)
    narrow = (2, 5)
    return {0: VoiceConfig(bands=wide, min_bands=1, release_frames=6), 1: VoiceConfig(bands=wide, min_bands=1, release_frames=6),
            3: VoiceConfig(bands=narrow, min_bands=narrow[1] - narrow[0], attack_frames=2, release_frames=3, threshold=1.0, rise_speech=0.0),
            4: VoiceConfig(min_bands=min(4, n_mels), attack_frames=1, release_frames=1, fall=1.0, rise=0.5, min_level=-9.5)}


def clips(n_mels):
    a = random_mel(n_mels, FRAMES, 1000 + n_mels)
    b = random_mel(n_mels, FRAMES, 2000 + n_mels)
    b[2:5, 20:30] += 5.0                                                    # every band of slot 3's window at once
    b[2:5, 70:72] += 5.0
    c = random_mel(n_mels, FRAMES, 3000 + n_mels)
    c[:, 64] = math.log(1e-5)                                               # columns at the clamp value on both sides of a chunk edge
    c[:, 66:68] = math.log(1e-5)
    return {0: a, 1: a, 3: b.contiguous(), 4: c.contiguous()}


@pytest.mark.parametrize("n_mels", [7, 64, 65, 80, 100, 128])
def test_kernel_equals_the_host_scan_bit_for_bit(dev, n_mels):
    cfg, clip = configs(n_mels), clips(n_mels)
    W = n_mels + voice.STATE_INTS
    state = torch.zeros(S, W, dtype=torch.int32, device=dev)
    state[IDLE] = SENTINEL_WORD
    ref = {s: voice.fresh_state(n_mels) for s in SCRIPT}
    at = {s: 0 for s in SCRIPT}
    got = {s: ([], []) for s in SCRIPT}
    expect = {s: ([], []) for s in SCRIPT}
    table = torch.empty(voice.TABLE_WORDS * S, dtype=torch.int32, device=dev)
    seen_counts = set()
    for j in range(4):
        n = [SCRIPT[s][j] if s in SCRIPT else 0 for s in range(S)]
        seen_counts |= set(n)
        tmax = max(n)
        pitch = tmax + 3
        base = torch.full((S, n_mels, tmax + 5), float("nan"))              # NaN behind every slot's frames and in the idle rows:
        for s in SCRIPT:                                                    # a frame read from there would poison a floor
            base[s, :, :n[s]] = clip[s][:, at[s]:at[s] + n[s]]
        mel = base.to(dev)[:, :, :tmax]                                     # a view: the band stride is not the frame count
        flags = torch.full((S, pitch), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
        counts = torch.full((S, pitch), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
        voice.voice_items(mel, n, [cfg.get(s) for s in range(S)], state, flags, counts, table=table)
        host_state, host_flags, host_counts = state.cpu(), flags.cpu(), counts.cpu()
        for s in SCRIPT:
            ref[s], f, c = voice.scan(clip[s][:, at[s]:at[s] + n[s]].contiguous(), cfg[s], ref[s])
            at[s] += n[s]
            assert torch.equal(host_state[s], ref[s]), (n_mels, j, s, host_state[s][n_mels:].tolist(), ref[s][n_mels:].tolist())
            assert torch.equal(host_flags[s, :n[s]], f) and torch.equal(host_counts[s, :n[s]], c), (n_mels, j, s)
            assert (host_flags[s, n[s]:] == SENTINEL_BYTE).all() and (host_counts[s, n[s]:] == SENTINEL_BYTE).all(), (n_mels, j, s)
            got[s][0].append(host_flags[s, :n[s]]), got[s][1].append(host_counts[s, :n[s]])
            expect[s][0].append(f), expect[s][1].append(c)
        assert (host_state[IDLE] == SENTINEL_WORD).all() and (host_flags[IDLE] == SENTINEL_BYTE).all() and (host_counts[IDLE] == SENTINEL_BYTE).all()
    assert {0, 1, 2, 63, 64, 65, 130} <= seen_counts
    # 130 frames in one launch and in the pieces 1, 63, 2, 64: one state, one sequence of flags and counts
    one, _, _ = voice.scan(clip[0][:, :130].contiguous(), cfg[0])
    assert torch.equal(ref[1], one) and torch.equal(torch.cat(got[1][0]), got[0][0][0]) and torch.equal(torch.cat(got[1][1]), got[0][1][0])
    # the cases are no trivial ones: every slot's state machine went to speech and back at least once
    for s in SCRIPT:
        ints = ref[s][n_mels:].tolist()
        assert ints[voice.I_STARTS] >= 1 and ints[voice.I_END] >= 0 and ints[voice.I_SEEN] == at[s], (n_mels, s, ints)
        assert set(torch.cat(expect[s][0]).tolist()) >= {0, 3}, (n_mels, s)


def test_outputs_are_optional_and_an_all_idle_call_launches_nothing(dev):
    from dmel_codec_amd import _lib
    n_mels = 80
    mel = random_mel(n_mels, 70, 5).to(dev)[None].contiguous()
    cfg = VoiceConfig()
    want, want_flags, _ = voice.scan(mel[0].cpu(), cfg)
    state = torch.zeros(1, n_mels + 8, dtype=torch.int32, device=dev)
    voice.voice_items(mel, [70], [cfg], state)                              # neither flags nor counts
    assert torch.equal(state[0].cpu(), want)
    state.zero_()
    flags = torch.zeros(1, 70, dtype=torch.uint8, device=dev)
    voice.voice_items(mel, [70], [cfg], state, flags=flags)                 # flags alone, pitch == frames
    assert torch.equal(state[0].cpu(), want) and torch.equal(flags[0].cpu(), want_flags)
    _lib.prof_enable(True)
    try:
        _lib.prof_reset()
        voice.voice_items(mel, [0], [None], state, flags=flags)
        assert _lib.prof_read("voice")["launches"] == 0
        voice.voice_items(mel, [3], [cfg], state, flags=flags)
        torch.cuda.synchronize()
        assert _lib.prof_read("voice")["launches"] == 1
    finally:
        _lib.prof_enable(False)


def test_refusals_name_their_item_and_launch_nothing(dev):
    from dmel_codec_amd import _lib
    lib = _lib.lib()
    n_mels, n = 80, 10
    mel = random_mel(n_mels, n, 6).to(dev)[None].repeat(3, 1, 1).contiguous()
    state = torch.full((3, n_mels + 8), 77, dtype=torch.int32, device=dev)
    out = torch.full((3, n), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    table = torch.empty(voice.TABLE_WORDS * 3, dtype=torch.int32, device=dev)
    good_f, good_i = VoiceConfig().fparams(), VoiceConfig().iparams(n_mels)

    def call(frames, fp, ip, pitch=n, n_mels=n_mels, S=3, state_ptr=None):
        rc = lib.dmel_voice_items(mel.data_ptr(), mel.stride(0), mel.stride(1), n_mels, S, (C.c_int64 * 3)(*frames),
                                  (C.c_float * 15)(*[v for r in fp for v in r]), (C.c_int32 * 15)(*[v for r in ip for v in r]),
                                  state.data_ptr() if state_ptr is None else state_ptr, out.data_ptr(), out.data_ptr(), pitch,
                                  table.data_ptr(), _lib.stream_ptr())
        return rc, lib.dmel_last_error().decode(errors="replace")

    F3, I3 = [good_f] * 3, [good_i] * 3
    with torch.cuda.device(dev):
        for kw, words in ((dict(frames=[n, n, -1], fp=F3, ip=I3), ("item 2", "frames")),
                          (dict(frames=[n, n + 1, n], fp=F3, ip=I3), ("item 1", "pitch")),
                          (dict(frames=[n, n, n], fp=[good_f, (0.0,) + good_f[1:], good_f], ip=I3), ("item 1", "threshold")),
                          (dict(frames=[n, n, n], fp=[good_f, good_f, good_f[:3] + (math.nan,) + good_f[4:]], ip=I3), ("item 2", "finite")),
                          (dict(frames=[n, n, n], fp=[good_f[:2] + (1.5,) + good_f[3:], good_f, good_f], ip=I3), ("item 0", "fall")),
                          (dict(frames=[n, n, n], fp=F3, ip=[good_i, (0, n_mels + 1) + good_i[2:], good_i]), ("item 1", "bands")),
                          (dict(frames=[n, n, n], fp=F3, ip=[good_i, good_i, good_i[:2] + (81,) + good_i[3:]]), ("item 2", "min_bands")),
                          (dict(frames=[n, n, n], fp=F3, ip=[good_i[:3] + (0,) + good_i[4:], good_i, good_i]), ("item 0", "attack_frames")),
                          (dict(frames=[n, n, n], fp=F3, ip=[good_i, good_i[:4] + (0,), good_i]), ("item 1", "release_frames")),
                          (dict(frames=[n, n, n], fp=F3, ip=I3, S=0), ("65535",)),
                          (dict(frames=[n, n, n], fp=F3, ip=I3, n_mels=129), ("mel bands",)),
                          (dict(frames=[n, n, n], fp=F3, ip=I3, state_ptr=state.data_ptr() + 2), ("aligned",))):
            rc, msg = call(**kw)
            assert rc == -1 and all(w in msg for w in words), (kw, rc, msg)
        torch.cuda.synchronize()
    assert (state.cpu() == 77).all() and (out.cpu() == SENTINEL_BYTE).all()     # nothing was launched
    with pytest.raises(ValueError, match="config"):
        voice.voice_items(mel, [n, n, n], [VoiceConfig(), None, VoiceConfig()], torch.zeros_like(state))
    with pytest.raises(ValueError, match="exceed"):
        voice.voice_items(mel, [n + 1, 0, 0], [VoiceConfig(), None, None], torch.zeros_like(state))
    with pytest.raises(ValueError, match="min_bands"):
        voice.voice_items(mel[:, :3].contiguous(), [n, 0, 0], [VoiceConfig(), None, None], torch.zeros(3, 11, dtype=torch.int32, device=dev))
