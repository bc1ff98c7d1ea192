"""Interleaved channels without a GPU: the restatement of the channel rule (tests/channels_ref.py) against values pinned by hand,
against numpy.mean(axis=0) of the channel-first array (librosa's to_mono) and against the fp64 mean rounded once; the Python-side
refusals of utils/pcm.py and of both pools, with their state unchanged; the refusals of dmel_pcm_convert_items_ch (it refuses before it
launches, so the "device" pointers of those calls are never followed); and the new symbol's place in the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import channels_ref as cref
import g711_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_words(values):
    return [int(np.float32(v).view(np.uint32)) for v in values]


# ------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_the_hand_values():
    """c = 3 frames whose sum is 5, 7, 1.25: 5 / 3 = 1.6666666..., nearest fp32 0x3FD55555, while 5 * fl(1 / 3) = 5 * 0x3EAAAAAB rounds
    to 0x3FD55556 -- division and reciprocal-multiply differ in the last bit (the same for 7 / 3 and 1.25 / 3)"""
    x = torch.tensor([[1.0, 2.0, 2.0], [1.0, 2.0, 4.0], [0.25, 0.5, 0.5], [3.0, 3.0, 3.0], [-1.0, 0.0, 1.0]])
    got = cref.downmix(x, "f32")
    assert f32_words(got.numpy()) == [0x3FD55555, 0x40155555, 0x3ED55555, 0x40400000, 0x00000000]
    recip = (x[:, 0] + x[:, 1] + x[:, 2]).numpy() * (np.float32(1) / np.float32(3))
    assert f32_words(recip)[:3] == [0x3FD55556, 0x40155556, 0x3ED55556]               # what the rule is NOT
    # the sum is left to right: (2^24 + 1) + 1 loses both ones, 1 + 1 + 2^24 keeps them
    order = torch.tensor([[2.0 ** 24, 1.0, 1.0], [1.0, 1.0, 2.0 ** 24]])
    assert cref.downmix(order, "f32").tolist() == [float(np.float32(2.0 ** 24) / np.float32(3)), float(np.float32(2.0 ** 24 + 2) / np.float32(3))]
    stereo = torch.tensor([[1.0, 2.0], [-0.0, -0.0], [2.0 ** -149, 0.0], [2.0 ** -149, 2.0 ** -149], [3.0 * 2.0 ** -149, 0.0]])
    got = cref.downmix(stereo, "f32")
    assert f32_words(got.numpy()) == [0x3FC00000, 0x80000000, 0x00000000, 0x00000001, 0x00000002]    # denormals: ties to even
    # s16 and the laws: each channel by its format's rule first
    s = torch.tensor([[-32768, 32767], [1, 2], [-1, 0]], dtype=torch.int16)
    assert cref.downmix(s, "s16").tolist() == [-0.5 / 32768, 1.5 / 32768, -0.5 / 32768]
    assert cref.downmix(s, "s16", channel=1).tolist() == [32767 / 32768, 2 / 32768, 0.0]
    u = torch.tensor([[0x00, 0x80, 0xFF], [0x7F, 0xFF, 0x80]], dtype=torch.uint8)       # -32124, 32124, 0 / 0, 0, 32124
    assert cref.downmix(u, "ulaw").tolist() == [0.0, float(np.float32(32124 / 32768) / np.float32(3))]
    assert cref.downmix(u, "ulaw", channel=0).tolist() == [-32124 / 32768, 0.0]
    a = torch.tensor([[0x55, 0xD5], [0x2A, 0xD5]], dtype=torch.uint8)                   # -8, 8 / -32256, 8
    assert cref.downmix(a, "alaw").tolist() == [0.0, -16124 / 32768]
    # pick and fan-out move words: -0.0, a denormal and a NaN's payload survive
    odd = torch.tensor([0x80000000 - 2 ** 32, 0x00000001, 0x7FC12345, 0x3F800000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    two = torch.stack([odd, odd.flip(0)], dim=1)
    assert torch.equal(cref.words(cref.downmix(two, "f32", channel=0)), cref.words(odd))
    assert torch.equal(cref.words(cref.downmix(two, "f32", channel=1)), cref.words(odd.flip(0)))
    fan = cref.fan_out(odd, 3, "f32")
    assert fan.shape == (4, 3) and fan.is_contiguous() and all(torch.equal(cref.words(fan[:, j]), cref.words(odd)) for j in range(3))
    y = torch.tensor([0.5 / 32768, 1.5 / 32768, 2.0, float("nan"), -1.0])
    assert cref.fan_out(y, 2, "s16").tolist() == [[0, 0], [2, 2], [32767, 32767], [0, 0], [-32768, -32768]]
    assert cref.fan_out(y, 2, "ulaw").tolist() == [[0xFF] * 2, [0xFF] * 2, [0x80] * 2, [0xFF] * 2, [0x00] * 2]
    assert cref.fan_out(y, 8, "alaw")[2].tolist() == [0xAA] * 8


@pytest.mark.parametrize("c", [2, 3, 5, 6, 7, 8])
def test_restatement_is_numpy_mean_over_the_channel_first_array(c):
    """librosa.to_mono is numpy.mean(y, axis=0) of the (c, n) float32 array: the restatement equals it bit for bit for every c, and the
    shorter forms do not all -- at least the reciprocal-multiply differs for c = 3, 5, 6, 7"""
    y = np.random.default_rng(c).standard_normal((c, 20000)).astype(np.float32)
    x = torch.from_numpy(np.ascontiguousarray(y.T))                                     # interleaved (n, c)
    got = cref.downmix(x, "f32").numpy()
    assert np.array_equal(got.view(np.uint32), np.mean(y, axis=0).view(np.uint32))
    acc = y[0].copy()
    for j in range(1, c):
        acc = acc + y[j]
    recip = acc * np.float32(1.0 / c)
    assert np.array_equal(recip, got) == (c in (2, 8))                                  # exact only where 1 / c is a power of two


@pytest.mark.parametrize("fmt", ["s16", "ulaw", "alaw"])
@pytest.mark.parametrize("c", [2, 3, 5, 8])
def test_integer_formats_give_the_fp64_mean_rounded_once(fmt, c):
    """the channel values (16 bits) and their sum (at most 16 + 3 bits) are exact in fp32: the only rounding is the division's"""
    g = torch.Generator().manual_seed(c)
    if fmt == "s16":
        x = torch.randint(-32768, 32768, (20000, c), generator=g).to(torch.int16)
        x[0], x[1] = -32768, 32767
        v = x.double() / 32768
    else:
        x = torch.randint(0, 256, (20000, c), generator=g).to(torch.uint8)
        v = torch.from_numpy(ref.decode(x.numpy(), fmt).astype(np.float64)) / 32768
    want = (v.sum(dim=1) / c).float()                                                   # fp64: the sum is exact, one rounding to fp32
    assert torch.equal(cref.downmix(x, fmt), want)


# ------------------------------------------------------------------------------------ utils/pcm.py and the pools
def test_convert_items_and_helpers_refuse_before_any_device_call():
    from dmel_codec_amd.utils import pcm
    f, f2, f3 = torch.zeros(4), torch.zeros(4, 2), torch.zeros(4, 3)
    s2, u2 = torch.zeros(4, 2, dtype=torch.int16), torch.zeros(4, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="channel counts 9 -> 1"):
        pcm.convert_items([torch.zeros(4, 9)], [f], src_channels=[9])
    with pytest.raises(ValueError, match="channel counts 1 -> 0"):
        pcm.convert_items([f], [f], dst_channels=[0])
    with pytest.raises(ValueError, match="item 1: 2 -> 3 channels is not served"):
        pcm.convert_items([f, f2], [f, f3], src_channels=[1, 2], dst_channels=[None, 3])
    with pytest.raises(ValueError, match="channel 2 of a source with 2"):
        pcm.convert_items([f2], [f], src_channels=[2], src_pick=[2])
    with pytest.raises(ValueError, match="channel 0 of a source with 1"):
        pcm.convert_items([f], [f], src_pick=[0])
    with pytest.raises(ValueError, match="src_channels names 2 pieces"):
        pcm.convert_items([f2], [f], src_channels=[2, 2])
    with pytest.raises(ValueError, match="torch.uint8"):                                # channels do not name the law either
        pcm.convert_items([u2], [f], src_channels=[2])
    with pytest.raises(RuntimeError, match="GPU"):                                      # well-formed: refused last, for the device
        pcm.convert_items([f2], [f], src_channels=[2])
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.convert_items([f], [s2], dst_channels=[2])
    with pytest.raises(RuntimeError, match="GPU"):                                      # everything that was valid stays valid
        pcm.convert_items([f], [f])
    # downmix
    for bad in (f, torch.zeros(2, 2, 2, 2)):
        with pytest.raises(ValueError, match="interleaved frames"):
            pcm.downmix(bad)
    with pytest.raises(ValueError, match="9 channels"):
        pcm.downmix(torch.zeros(4, 9))
    with pytest.raises(ValueError, match="torch.uint8"):
        pcm.downmix(u2)
    with pytest.raises(ValueError, match="'alaw'"):
        pcm.downmix(s2, "alaw")
    with pytest.raises(ValueError, match="unknown sample format"):
        pcm.downmix(u2, "u8")
    with pytest.raises(ValueError, match="channel=2"):
        pcm.downmix(f2, channel=2)
    with pytest.raises(ValueError, match="channel=0"):
        pcm.downmix(torch.zeros(4, 1), channel=0)
    with pytest.raises(ValueError, match="samples are"):
        pcm.downmix(torch.zeros(4, 2, dtype=torch.float64))
    for ok in (dict(x=f2), dict(x=s2, channel=1), dict(x=u2, sample_format="ulaw"), dict(x=torch.zeros(3, 4, 2))):
        with pytest.raises(RuntimeError, match="GPU"):
            pcm.downmix(**ok)
    # fan_out
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="channels="):
            pcm.fan_out(f, bad)
    with pytest.raises(ValueError, match="unknown sample format"):
        pcm.fan_out(f, 2, "u8")
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.fan_out(f, 2, "s16")
    assert pcm.FORMATS == {"f32": (0, torch.float32), "s16": (1, torch.int16), "ulaw": (8, torch.uint8), "alaw": (9, torch.uint8)}
    assert pcm.MAX_CHANNELS == 8


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=None)


def test_encode_pool_refusals_need_no_device(codec):
    pool = codec.encode_sessions(slots=3, max_push_samples=4000, sample_rates=(8000,))
    for kw, msg in ((dict(channels=0), "channels=0"), (dict(channels=9), "channels=9"), (dict(channels=2.0), "channels=2.0"),
                    (dict(channels=2, channel=2), "channel=2"), (dict(channels=2, channel=-1), "channel=-1"),
                    (dict(channel=0), "channel=0"), (dict(channels=2, sample_format="u8"), "unknown sample format"),
                    (dict(channels=2, sample_rate=44100), "44100 Hz")):
        with pytest.raises(ValueError, match=msg):
            pool.open(**kw)
    assert pool.open_slots == []                                                        # a refused open takes no slot
    st = pool.open(sample_rate=8000, sample_format="s16", channels=2)
    pk = pool.open(sample_format="ulaw", channels=2, channel=1)
    mono = pool.open()
    assert [pool.ch[s] for s in (st, pk, mono)] == [2, 2, 1] and [pool.pick[s] for s in (st, pk, mono)] == [-1, 1, -1]
    s2, u2 = torch.zeros(100, 2, dtype=torch.int16), torch.zeros(100, 2, dtype=torch.uint8)
    refused = [({st: torch.zeros(100, dtype=torch.int16)}, "channels=2"),               # 1-D to a stereo slot
               ({st: torch.zeros(1, 100, dtype=torch.int16)}, "channels=2"),            # (1, n) to a stereo slot
               ({st: torch.zeros(100, 3, dtype=torch.int16)}, "channels=2"),            # another channel count
               ({st: torch.zeros(2, 100, dtype=torch.int16)}, "channels=2"),            # planar
               ({st: torch.zeros(100, 4, dtype=torch.int16)[:, :2]}, "channels=2"),     # not contiguous
               ({mono: torch.zeros(100, 2)}, "expected mono audio"),                    # frames to a mono slot
               ({st: torch.zeros(100, 2)}, "sample_format='s16'"),                      # the dtype still has to match
               ({pk: s2}, "sample_format='ulaw'"),
               ({st: torch.zeros(4001, 2, dtype=torch.int16)}, "max_push_samples"),     # frames, not samples, are bounded
               ({st: s2, pk: u2, mono: torch.zeros(100, 2)}, "expected mono audio")]
    for push, msg in refused:
        with pytest.raises(ValueError, match=msg):
            pool.push(push)
    assert all(pool.sched[s].samples == 0 for s in (st, pk, mono)) and pool.allocated_bytes() == 0
    with pytest.raises(RuntimeError, match="GPU"):                                      # matching pushes on the CPU are refused last
        pool.push({st: torch.zeros(4000, 2, dtype=torch.int16), pk: u2, mono: torch.zeros(100)})
    assert all(pool.sched[s].samples == 0 for s in (st, pk, mono)) and pool.allocated_bytes() == 0
    pool.sched[st] = None                                                               # what a final push leaves behind
    assert pool.open(channels=3) == st and (pool.ch[st], pool.pick[st], pool.fmt[st]) == (3, -1, "f32")
    pool.sched[st] = None
    assert pool.open() == st and (pool.ch[st], pool.pick[st]) == (1, -1)                # a reopened slot takes the new session's count
    assert pool.allocated_bytes() == codec.encode_sessions(slots=3, max_push_samples=4000, sample_rates=(8000,)).allocated_bytes()


def test_decode_pool_refusals_need_no_device(codec):
    pool = codec.decode_sessions(2, max_push_tokens=8, return_audios=False)
    with pytest.raises(ValueError, match="return_audios=False"):
        pool.open(channels=2)
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError, match="channels="):
            pool.open(channels=bad)
    with pytest.raises(TypeError):
        pool.open(channels=2, channel=0)                                                # a reply has nothing to pick from
    assert pool.open_slots == [] and pool.open() == 0 and pool.ch[0] == 1 and pool.fmt[0] == "f32"


def test_pool_constructors_take_no_channel_argument(codec):
    with pytest.raises(TypeError):
        codec.encode_sessions(slots=1, channels=2)
    with pytest.raises(TypeError):
        codec.decode_sessions(1, return_audios=False, channels=2)


# ------------------------------------------------------------------------------------ the C entry
def test_c_entry_refuses_before_it_launches():
    """host memory stands in for the device: a refused call reads the tables and never follows a pointer"""
    from dmel_codec_amd import _lib
    L = _lib.lib()
    f = torch.zeros(64, dtype=torch.float32)
    s = torch.full((64,), 7, dtype=torch.int16)
    u = torch.full((64,), 9, dtype=torch.uint8)
    table = torch.zeros(8, dtype=torch.int64)
    F32, S16, ULAW, ALAW = 0, 1, 8, 9
    I32 = lambda v: None if v is None else (C.c_int32 * len(v))(*v)

    def call(src, sf, dst, df, n, sc=None, dc=None, pick=None, old=False):
        k = len(src)
        P = C.c_void_p * k
        if old:
            rc = L.dmel_pcm_convert_items(P(*src), I32(sf), P(*dst), I32(df), (C.c_int64 * k)(*n), k, table.data_ptr(), None)
        else:
            rc = L.dmel_pcm_convert_items_ch(P(*src), I32(sf), I32(sc), I32(pick), P(*dst), I32(df), I32(dc), (C.c_int64 * k)(*n), k,
                                             table.data_ptr(), None)
        return rc, L.dmel_last_error().decode(errors="replace")

    fp, sp, up = f.data_ptr(), s.data_ptr(), u.data_ptr()
    # item 0 is a valid stereo item in every case; item 1 is the one refused
    base = dict(src=[sp, fp], sf=[S16, F32], dst=[fp + 128, sp + 64], df=[F32, S16], n=[4, 4])
    cases = {"src_ch 0": dict(sc=[2, 0]), "src_ch 9": dict(sc=[2, 9]), "src_ch -1": dict(sc=[2, -1]),
             "dst_ch 0": dict(sc=[2, 1], dc=[1, 0]), "dst_ch 9": dict(sc=[2, 1], dc=[1, 9]),
             "2 -> 2": dict(sc=[2, 2], dc=[1, 2]), "3 -> 8": dict(sc=[2, 3], dc=[1, 8]),
             "pick 2 of 2": dict(sc=[2, 2], pick=[0, 2]), "pick -2": dict(sc=[2, 2], pick=[1, -2]),
             "pick with a mono source": dict(sc=[2, 1], pick=[-1, 0]), "pick 0 into a fan-out": dict(sc=[2, 1], dc=[1, 2], pick=[-1, 0]),
             "stereo s16 -> mono s16": dict(sc=[2, 2], src=[sp, sp], sf=[S16, S16]),
             "stereo ulaw -> mono alaw": dict(sc=[2, 2], src=[sp, up], sf=[S16, ULAW], dst=[fp + 128, up + 32], df=[F32, ALAW]),
             "mono f32 -> code 2, stereo": dict(sc=[2, 1], dc=[1, 2], df=[F32, 2]),
             "n * c reaches 2^40": dict(sc=[2, 1], dc=[1, 8], n=[4, 1 << 37]),
             "NULL stereo src": dict(sc=[2, 2], src=[sp, 0], sf=[S16, S16], dst=[fp + 128, fp], df=[F32, F32]),
             "odd stereo s16 dst": dict(sc=[2, 1], dc=[1, 2], dst=[fp + 128, sp + 65])}
    for name, kw in cases.items():
        rc, msg = call(**{**base, **kw})
        assert rc == -1 and "item 1" in msg and msg.startswith("pcm_convert_items"), (name, rc, msg)
    assert "not a conversion" in call(**{**base, **cases["stereo s16 -> mono s16"]})[1]
    assert "channels is not served" in call(**{**base, **cases["2 -> 2"]})[1]
    assert "1 .. 8" in call(**{**base, **cases["src_ch 9"]})[1] and "pick" in call(**{**base, **cases["pick 2 of 2"]})[1]
    rc, msg = call([0, up], [ULAW, ALAW], [fp, 0], [F32, F32], [0, 0], sc=[8, 2], pick=[7, -1])        # every item idle: DMEL_OK
    assert rc == 0, msg
    rc, msg = call([0, 0], [F32, F32], [up + 1, sp], [ULAW, S16], [0, 0], dc=[3, 8])
    assert rc == 0, msg
    # NULL channel tables: the old entry's verdict on the old cases, refusals and their messages included
    old = {"ulaw -> alaw": ([up, up], [ULAW, ULAW], [fp, up + 32], [F32, ALAW], [4, 4]),
           "s16 -> s16": ([up, sp], [ULAW, S16], [fp, sp + 32], [F32, S16], [4, 4]),
           "ulaw -> s16": ([up, up], [ULAW, ULAW], [fp, sp], [F32, S16], [4, 4]),
           "code 2": ([up, fp], [ULAW, F32], [fp, up + 32], [F32, 2], [4, 4]),
           "code 264": ([up, up], [ULAW, 264], [fp, fp + 128], [F32, F32], [4, 4]),
           "negative n": ([up, up], [ULAW, ULAW], [fp, fp + 128], [F32, F32], [4, -1]),
           "n = 2^40": ([up, up], [ULAW, ULAW], [fp, fp + 128], [F32, F32], [4, 1 << 40]),
           "NULL law src": ([up, 0], [ULAW, ALAW], [fp, fp + 128], [F32, F32], [4, 4]),
           "f32 off by 2": ([up, fp + 2], [ULAW, F32], [fp, up + 32], [F32, ALAW], [4, 4]),
           "idle": ([0, up], [ULAW, ALAW], [fp, 0], [F32, F32], [0, 0]),
           "idle, odd law pointers": ([fp, 0], [F32, F32], [up + 1, up + 3], [ULAW, ALAW], [0, 0])}
    for name, args in old.items():
        want = call(*args, old=True)
        assert call(*args) == want and call(*args, sc=[1, 1], dc=[1, 1], pick=[-1, -1]) == want, name
        assert want[0] == (0 if name.startswith("idle") else -1), (name, want)
    assert bool((f == 0).all()) and bool((s == 7).all()) and bool((u == 9).all()) and bool((table == 0).all())


def test_the_symbol_is_declared_exported_and_bound():
    from dmel_codec_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmel_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dmel_pcm_convert_items_ch\s*\(", src) and re.search(r"#define\s+DMEL_MAX_CHANNELS\s+8\b", src)
    L = _lib.lib()
    assert hasattr(L, "dmel_pcm_convert_items_ch") and hasattr(L, "dmel_pcm_convert_items")
    assert len(_lib.PROTOTYPES["dmel_pcm_convert_items_ch"][1]) == 11 and len(_lib.PROTOTYPES["dmel_pcm_convert_items"][1]) == 8
    assert L.dmel_abi_version() == 2
