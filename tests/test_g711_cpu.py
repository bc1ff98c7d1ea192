"""G.711 sessions without a GPU: the numpy restatement of the companding rule (tests/g711_ref.py) against CPython's audioop, against
values pinned by hand and against the round-trip property; the Python-side refusals of utils/pcm.py and of the pools that need no
device; the refusals of dmel_pcm_convert_items (it refuses before it launches, so the "device" pointers of those calls are never
followed); and the resampler's schedule at the two telephony pairs, 8000 <-> 24000 Hz."""
import ctypes as C

import numpy as np
import pytest
import torch

import g711_ref as ref
from dmel_codec_amd.models.stream_schedule import ResampleSchedule, resample_max_outputs

ALL_S16 = np.arange(-32768, 32768, dtype=np.int32)
ALL_CODES = np.arange(256, dtype=np.int32)


# ------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("law", ref.LAWS)
def test_restatement_equals_audioop(law):
    """all 65536 s16 values through both encoders, all 256 codes through both decoders"""
    audioop = pytest.importorskip("audioop")
    enc, dec = {"ulaw": (audioop.lin2ulaw, audioop.ulaw2lin), "alaw": (audioop.lin2alaw, audioop.alaw2lin)}[law]
    want = np.frombuffer(enc(ALL_S16.astype("<i2").tobytes(), 2), dtype=np.uint8)
    assert want.shape == (65536,) and np.array_equal(ref.encode(ALL_S16, law), want)
    back = np.frombuffer(dec(ALL_CODES.astype(np.uint8).tobytes(), 2), dtype="<i2")
    assert back.shape == (256,) and np.array_equal(ref.decode(ALL_CODES, law), back)


@pytest.mark.parametrize("law", ref.LAWS)
def test_restatement_equals_the_hand_values(law):
    for x, code in ref.HAND_ENCODE[law]:
        assert int(ref.encode([x], law)[0]) == code, (law, x, hex(code))
    for code, x in ref.HAND_DECODE[law]:
        assert int(ref.decode([code], law)[0]) == x, (law, hex(code), x)
    special = torch.tensor([float("nan"), 0.0, -0.0, 1e-40, float("inf"), float("-inf"), 1.0, -1.0, 2.0, -2.0])
    full = {"ulaw": (0x80, 0x00), "alaw": (0xAA, 0x2A)}[law]
    assert ref.f32_to_law(special, law).tolist() == [ref.NEUTRAL[law]] * 4 + [full[0], full[1]] * 3
    assert ref.law_to_f32(torch.tensor([c for c, _ in ref.HAND_DECODE[law]], dtype=torch.uint8), law).tolist() == \
        [x / 32768 for _, x in ref.HAND_DECODE[law]]


def test_round_trip_holds_for_every_code_but_negative_zero():
    again = ref.encode(ref.decode(ALL_CODES, "alaw"), "alaw")
    assert np.array_equal(again, ALL_CODES)                                             # 256 of 256
    again = ref.encode(ref.decode(ALL_CODES, "ulaw"), "ulaw")
    differ = np.nonzero(again != ALL_CODES)[0].tolist()
    assert differ == [0x7F] and int(ref.decode([0x7F], "ulaw")[0]) == 0 and int(again[0x7F]) == 0xFF     # 255 of 256
    for law in ref.LAWS:                                                                # decode is monotone in the folded code
        assert len(set(ref.decode(ALL_CODES, law).tolist())) == (255 if law == "ulaw" else 256)
        edges = ref.segment_edges(law)
        assert len(edges) == 15 and 0 in edges                                          # 8 segments on either side of zero


# ------------------------------------------------------------------------------------ utils/pcm.py and the pools
def test_formats_and_helpers_refuse_before_any_device_call():
    from dmel_codec_amd.utils import pcm
    assert pcm.FORMATS == {"f32": (0, torch.float32), "s16": (1, torch.int16), "ulaw": (8, torch.uint8), "alaw": (9, torch.uint8)}
    u8, f = torch.zeros(4, dtype=torch.uint8), torch.zeros(4)
    with pytest.raises(ValueError, match="torch.uint8"):                                # the dtype alone does not say which law
        pcm.convert_items([u8], [f])
    with pytest.raises(ValueError, match="torch.uint8"):
        pcm.convert_items([f], [u8])
    with pytest.raises(ValueError, match="torch.uint8"):
        pcm.convert_items([f, u8], [u8, f], src_formats=[None, "ulaw"], dst_formats=[None, None])      # item 0's destination
    with pytest.raises(ValueError, match="unknown sample format"):
        pcm.convert_items([u8], [f], src_formats=["u8"])
    with pytest.raises(ValueError, match="'ulaw'"):                                     # a name that does not fit the dtype
        pcm.convert_items([f], [f], src_formats=["ulaw"])
    with pytest.raises(ValueError, match="names 2 pieces"):
        pcm.convert_items([u8], [f], src_formats=["ulaw", "ulaw"])
    with pytest.raises(RuntimeError, match="GPU"):                                      # named: refused last, loudly, for the device
        pcm.convert_items([u8], [f], src_formats=["alaw"])
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.from_g711(u8, "ulaw")
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.to_g711(f, "alaw")
    with pytest.raises(ValueError, match="unknown sample format"):
        pcm.check_format("u8")


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=None)


def test_encode_pool_refusals_need_no_device(codec):
    pool = codec.encode_sessions(slots=3, max_push_samples=4000, sample_rates=(8000,))
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="u8")
    assert pool.open_slots == []
    u, a, f = pool.open(sample_rate=8000, sample_format="ulaw"), pool.open(sample_rate=8000, sample_format="alaw"), pool.open()
    assert [pool.fmt[s] for s in (u, a, f)] == ["ulaw", "alaw", "f32"] and pool.rate[u] == 8000
    codes = torch.zeros(100, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sample_format='ulaw'"):
        pool.push({u: torch.zeros(100)})                                                # a float push to a law slot
    with pytest.raises(ValueError, match="sample_format='alaw'"):
        pool.push({a: torch.zeros(100, dtype=torch.int16)})                             # an s16 push to a law slot
    with pytest.raises(ValueError, match="sample_format='f32'"):
        pool.push({f: codes})                                                           # and codes to a float slot
    with pytest.raises(ValueError, match="sample_format='alaw'"):
        pool.push({u: codes, a: codes.to(torch.int8)})
    assert all(pool.sched[s].samples == 0 for s in (u, a, f)) and pool.allocated_bytes() == 0
    with pytest.raises(RuntimeError, match="GPU"):                                      # a matching push on the CPU is refused last
        pool.push({u: codes, a: codes})
    assert pool.sched[u].samples == 0 and pool.allocated_bytes() == 0
    pool.sched[u] = None                                                                # what a final push leaves behind
    assert pool.open(sample_format="alaw") == u and pool.fmt[u] == "alaw"               # a reopened slot takes the new session's law


def test_decode_pool_refusals_need_no_device(codec):
    pool = codec.decode_sessions(2, max_push_tokens=8, return_audios=False)
    for law in ref.LAWS:
        with pytest.raises(ValueError, match="return_audios=False"):
            pool.open(sample_format=law)
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="u8")
    assert pool.open_slots == [] and pool.open() == 0 and pool.fmt[0] == "f32"


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

    def call(src, sf, dst, df, n):
        k = len(src)
        rc = L.dmel_pcm_convert_items((C.c_void_p * k)(*src), (C.c_int32 * k)(*sf), (C.c_void_p * k)(*dst), (C.c_int32 * k)(*df),
                                      (C.c_int64 * k)(*n), k, table.data_ptr(), None)
        return rc, L.dmel_last_error().decode(errors="replace")

    fp, sp, up = f.data_ptr(), s.data_ptr(), u.data_ptr()
    # item 0 is a valid law item in every case; item 1 is the one refused
    cases = {"ulaw -> alaw": ([up, up], [ULAW, ULAW], [fp, up + 32], [F32, ALAW], [4, 4]),
             "alaw -> alaw": ([up, up], [ULAW, ALAW], [fp, up + 32], [F32, ALAW], [4, 4]),
             "ulaw -> s16": ([up, up], [ULAW, ULAW], [fp, sp], [F32, S16], [4, 4]),
             "s16 -> alaw": ([up, sp], [ULAW, S16], [fp, up + 32], [F32, ALAW], [4, 4]),
             "code 2": ([up, fp], [ULAW, F32], [fp, up + 32], [F32, 2], [4, 4]),
             "code 7": ([up, up], [ULAW, 7], [fp, fp + 128], [F32, F32], [4, 4]),
             "code 10": ([up, fp], [ULAW, F32], [fp, up + 32], [F32, 10], [4, 4]),
             "code 264": ([up, up], [ULAW, 264], [fp, fp + 128], [F32, F32], [4, 4]),   # 8 + 256: must not alias ULAW in the table word
             "NULL law src": ([up, 0], [ULAW, ALAW], [fp, fp + 128], [F32, F32], [4, 4]),
             "NULL law dst": ([up, fp], [ULAW, F32], [fp, 0], [F32, ULAW], [4, 4]),
             "f32 off by 2": ([up, fp + 2], [ULAW, F32], [fp, up + 32], [F32, ALAW], [4, 4])}
    for name, args in cases.items():
        rc, msg = call(*args)
        assert rc == -1 and "item 1" in msg, (name, rc, msg)
    for name in ("ulaw -> alaw", "ulaw -> s16", "s16 -> alaw"):
        assert "not a conversion" in call(*cases[name])[1], name
    rc, msg = call([0, up], [ULAW, ALAW], [fp, 0], [F32, F32], [0, 0])                  # every item idle: DMEL_OK, nothing launched
    assert rc == 0, msg
    rc, msg = call([fp, 0], [F32, F32], [up + 1, up + 3], [ULAW, ALAW], [0, 0])          # odd law pointers are no offence, idle or not
    assert rc == 0, msg
    assert bool((f == 0).all()) and bool((s == 7).all()) and bool((u == 9).all())


# ------------------------------------------------------------------------------------ 8 kHz
@pytest.mark.parametrize("orig,new,up,down,width", [(8000, 24000, 3, 1, 7), (24000, 8000, 1, 3, 19)])
def test_telephony_rate_pairs_schedule(orig, new, up, down, width):
    """Brute force, as tests/test_sessions_resample_cpu.py does for the sound cards' pairs: from every phase, one push of n samples,
    final or not, never releases more than resample_max_outputs; the walk's pieces add up to the whole clip's output count."""
    ref_s = ResampleSchedule(orig, new)
    assert (ref_s.up, ref_s.down, ref_s.width, ref_s.kw) == (up, down, width, 2 * width + down)
    worst = {}
    for n in (0, 1, width, down, 160, 255, 777):
        bound = resample_max_outputs(orig, new, n)
        assert resample_max_outputs(orig, new, max(n - 1, 0)) <= bound
        for final in (False, True):
            for k in list(range(0, 2 * down + 2 * width + 1)) + [None]:
                sc = ResampleSchedule(orig, new)
                if k is not None:
                    sc.step(k)
                a, b = sc.step(n, final).outputs
                assert b - a <= bound, (n, final, k, b - a, bound)
                worst[n] = max(worst.get(n, 0), b - a)
    for n in (1, 160):
        assert worst[n] == resample_max_outputs(orig, new, n)
    for total in (1, 159, 160, 1001):                                                   # 20 ms packets of 160 samples, and ragged ones
        sc, out, pos = ResampleSchedule(orig, new), 0, 0
        for n in [160, 0, 1, 37] * 10:
            n = min(n, total - pos)
            pos += n
            a, b = sc.step(n, pos == total).outputs
            assert a == out
            out = b
            if pos == total:
                break
        assert out == sc.total_outputs(total) == -(-total * up // down)
