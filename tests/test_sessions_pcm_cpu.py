"""16-bit PCM sessions without a GPU: the rounding oracle of the GPU tests against a hand-written list, the refusals of the pools and of
utils/pcm.py that need no device, and the refusals of dmel_pcm_convert_items (it refuses before it launches, so the "device" pointers
of those calls are never followed)."""
import ctypes as C

import pytest
import torch

from test_gpu_pcm_convert import oracle_to_f32, oracle_to_s16


def test_oracle_rounds_halves_to_even_and_clamps():
    hand = {0.5: 0, -0.5: 0, 1.5: 2, 2.5: 2, -1.5: -2, 32767.5: 32767}
    y = torch.tensor([v / 32768 for v in hand], dtype=torch.float32)
    assert oracle_to_s16(y).tolist() == list(hand.values())
    assert oracle_to_s16(torch.tensor([float("nan"), float("inf"), float("-inf"), 1.0, -1.0])).tolist() == [0, 32767, -32768, 32767, -32768]
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    assert torch.equal(oracle_to_s16(oracle_to_f32(x)), x)                              # s16 -> f32 -> s16 is the identity


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=None)


def test_encode_pool_refusals_need_no_device(codec):
    pool = codec.encode_sessions(slots=3, max_push_samples=4000)
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="u8")
    assert pool.open_slots == []                                                        # the refused open took no slot
    a, b = pool.open(sample_format="s16"), pool.open()
    assert pool.fmt[a] == "s16" and pool.fmt[b] == "f32"
    with pytest.raises(ValueError, match="sample_format='s16'"):
        pool.push({a: torch.zeros(100)})                                                # a float push to an s16 slot
    with pytest.raises(ValueError, match="sample_format='f32'"):
        pool.push({b: torch.zeros(100, dtype=torch.int16)})                             # and the reverse
    with pytest.raises(ValueError, match="sample_format='s16'"):
        pool.push({b: torch.zeros(100), a: torch.zeros(100, dtype=torch.float64)})
    # nothing above changed any state or touched a device; a matching push on the CPU is refused last, loudly, as before
    assert pool.sched[a].samples == 0 and pool.sched[b].samples == 0 and pool.allocated_bytes() == 0
    with pytest.raises(RuntimeError, match="GPU"):
        pool.push({a: torch.zeros(100, dtype=torch.int16)})
    assert pool.sched[a].samples == 0 and pool.allocated_bytes() == 0
    pool.sched[a] = None                                                                # what a final push leaves behind
    assert pool.open() == a and pool.fmt[a] == "f32"                                    # a reopened slot takes the new session's format


def test_decode_pool_refusals_need_no_device(codec):
    pool = codec.decode_sessions(2, max_push_tokens=8, return_audios=False)
    with pytest.raises(ValueError, match="unknown sample format"):
        pool.open(sample_format="s24")
    with pytest.raises(ValueError, match="return_audios=False"):
        pool.open(sample_format="s16")
    assert pool.open_slots == [] and pool.open() == 0 and pool.fmt[0] == "f32"


def test_pcm_helpers_refuse_before_any_device_call():
    from dmel_codec_amd.utils import pcm
    assert pcm.FORMATS["f32"] == (0, torch.float32) and pcm.FORMATS["s16"] == (1, torch.int16)
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.from_pcm16(torch.zeros(10, dtype=torch.int16))
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.to_pcm16(torch.zeros(2, 10))
    with pytest.raises(RuntimeError, match="GPU"):
        pcm.convert_items([torch.zeros(4)], [torch.zeros(4, dtype=torch.int16)])
    with pytest.raises(ValueError, match="as many destinations"):
        pcm.convert_items([], [])
    with pytest.raises(ValueError, match="as many destinations"):
        pcm.convert_items([torch.zeros(4)], [])


def test_c_entry_refuses_before_it_launches():
    """host memory stands in for the device: a refused call reads the tables and never follows a pointer"""
    from dmel_codec_amd import _lib
    L = _lib.lib()
    f = torch.zeros(64, dtype=torch.float32)
    s = torch.full((64,), 7, dtype=torch.int16)
    table = torch.zeros(8, dtype=torch.int64)

    def call(src, sf, dst, df, n, B=None):
        k = len(src)
        rc = L.dmel_pcm_convert_items((C.c_void_p * k)(*src), (C.c_int32 * k)(*sf), (C.c_void_p * k)(*dst), (C.c_int32 * k)(*df),
                                      (C.c_int64 * k)(*n), k if B is None else B, table.data_ptr(), None)
        return rc, L.dmel_last_error().decode(errors="replace")

    fp, sp = f.data_ptr(), s.data_ptr()
    for name, args in {"s16 -> s16": ([fp, sp], [0, 1], [sp, sp], [1, 1], [4, 4]),
                       "format 2": ([fp, fp], [0, 2], [sp, sp], [1, 1], [4, 4]),
                       "format -1": ([fp, fp], [0, 0], [sp, sp], [1, -1], [4, 4]),
                       "negative n": ([fp, fp], [0, 0], [sp, sp], [1, 1], [4, -1]),
                       "NULL src": ([fp, 0], [0, 0], [sp, sp], [1, 1], [4, 4]),
                       "NULL dst": ([fp, fp], [0, 0], [sp, 0], [1, 1], [4, 4]),
                       "odd s16": ([fp, sp + 1], [0, 1], [sp, fp], [1, 0], [4, 4]),
                       "f32 off by 2": ([fp, fp], [0, 0], [sp, fp + 2], [1, 0], [4, 4])}.items():
        rc, msg = call(*args)
        assert rc == -1 and "item 1" in msg, (name, rc, msg)
    for B in (0, -1, 65536):
        rc, msg = call([fp], [0], [sp], [1], [4], B=B)
        assert rc == -1 and "65535" in msg, (B, rc, msg)
    assert L.dmel_pcm_convert_items(None, None, None, None, None, 1, table.data_ptr(), None) == -1
    rc, msg = call([0, fp], [0, 1], [sp, 0], [1, 0], [0, 0])                            # every item idle: DMEL_OK, nothing launched
    assert rc == 0, msg
    assert bool((f == 0).all()) and bool((s == 7).all())
