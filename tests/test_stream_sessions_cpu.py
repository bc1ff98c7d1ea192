"""Encode sessions, the parts that need no GPU: the row tables of a pool of schedules (models/stream_schedule.py: session_rows), the
open / push / close bookkeeping of EncodeSessions (every refusal happens before the first device call), and the bindings of the two
per-item C-ABI entries."""
import ctypes as C
import os
import re

import pytest
import torch

from dmel_codec_amd.models.stream_schedule import EncodeGeometry, EncodeSchedule, session_rows

HOP, NFFT = 256, 1024
DILS = tuple(2 ** (i % 4) for i in range(20))
GEO = EncodeGeometry(hop=HOP, n_fft=NFFT, dilations=DILS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_session_rows_follow_the_per_slot_schedules():
    """Four slots, three of them live with different starts, push sizes and ends: in every step the table's row of a slot is that slot's
    own EncodeSchedule walk, shifted by the slot's origin; slots without a step are rows of zeros."""
    S, W = 4, len(DILS) + 1
    walks = {0: [7680, 0, 7680, 100, 7680, 7680, 3000, 7680, 7680, 7680, 7680, 500],
             2: [None, None, 5000, 7680, 1, 7680, 7680, 7680, None, 7680, 7680, 7680],
             3: [None, 12345, 7680, None, 7680, 40, None, None, None, None, None, None]}
    ends = {0: 11, 2: 11, 3: 5}
    pool = {s: EncodeSchedule(GEO) for s in walks}
    alone = {s: EncodeSchedule(GEO) for s in walks}          # the same walks, one stream at a time
    origins = [0] * S
    for i in range(12):
        steps = {}
        for s, w in walks.items():
            if w[i] is not None:
                steps[s] = pool[s].step(w[i], final=(i == ends[s]))
        # re-base a slot the way the pool does: no column in front of the last level's window is read again
        for s, st in steps.items():
            origins[s] = max(0, min(st.prev[-1] - 8, st.quant_window[0]))
        prev, nxt, org = session_rows(S, steps, origins)
        assert len(prev) == len(nxt) == S * W and len(org) == S
        for s in range(S):
            rp, rn = prev[s * W:(s + 1) * W], nxt[s * W:(s + 1) * W]
            if s in steps:
                want = alone[s].step(walks[s][i], final=(i == ends[s]))
                assert want == steps[s]
                assert rp == [p - origins[s] for p in want.prev] and rn == [p - origins[s] for p in want.next]
                assert org[s] == origins[s] and min(rp) >= 0
                # the frontier rules dmel_wavenet_stream_step_items checks per row
                for l, d in enumerate(DILS):
                    assert rp[l + 1] <= rp[l] and rp[l + 1] <= rn[l + 1]
                    assert rn[l + 1] == rn[0] if want.final else (rn[l + 1] == rp[l + 1] or rn[l + 1] + d <= rn[l])
                    assert org[s] == 0 or rn[l + 1] == rp[l + 1] or rp[l + 1] >= d
            else:
                assert rp == rn == [0] * W and org[s] == 0
    assert origins[0] > 0 and origins[2] > 0          # the walks are long enough to re-base
    with pytest.raises(ValueError):
        session_rows(S, {}, origins)
    with pytest.raises(ValueError, match="out of range"):
        session_rows(S, {4: EncodeSchedule(GEO).step(100)}, [0] * 5)
    with pytest.raises(ValueError, match="origin"):
        session_rows(S, {1: EncodeSchedule(GEO).step(100)}, [0, 5, 0, 0])


@pytest.fixture(scope="module")
def codec():
    from dmel_codec_amd.configs import build_codec
    return build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=1, vocoder=None)


def test_open_push_close_bookkeeping_needs_no_device(codec):
    pool = codec.encode_sessions(slots=2, max_push_samples=4000)
    assert pool.allocated_bytes() == 0 and pool.open_slots == []
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1) and pool.open_slots == [0, 1]
    with pytest.raises(RuntimeError, match="slots are taken"):
        pool.open()
    with pytest.raises(ValueError, match="exceeds max_push_samples"):
        pool.push({a: torch.zeros(4001)})
    with pytest.raises(ValueError, match="out of range"):
        pool.push({2: torch.zeros(10)})
    with pytest.raises(ValueError, match="not among the pushed slots"):
        pool.push({a: torch.zeros(10)}, final=(b,))
    with pytest.raises(ValueError, match="reflect pad"):
        pool.push({a: torch.zeros(300)}, final=(a,))              # a stream that ends below the reflect pad has no encode()
    with pytest.raises(ValueError, match="mono"):
        pool.push({a: torch.zeros(2, 10)})
    with pytest.raises(ValueError, match="at least one"):
        pool.push({})
    # nothing above changed any state: no samples counted, no buffer allocated; a CPU tensor is refused last, loudly
    assert pool.sched[a].samples == 0 and pool.allocated_bytes() == 0
    with pytest.raises(RuntimeError, match="GPU"):
        pool.push({a: torch.zeros(4000)})
    assert pool.sched[a].samples == 0
    # a slot that was never opened, or is closed again, takes no push
    fresh = codec.encode_sessions(slots=3)
    with pytest.raises(RuntimeError, match="not open"):
        fresh.push({1: torch.zeros(10)})
    with pytest.raises(RuntimeError, match="not open"):
        fresh.close(1)
    s = fresh.open()
    fresh.sched[s] = None                                        # what a final push leaves behind
    with pytest.raises(RuntimeError, match="not open"):
        fresh.push({s: torch.zeros(10)})
    assert fresh.open() == s                                     # and the slot is free again


def test_capacity_is_fixed_by_the_push_size(codec):
    small, big = codec.encode_sessions(2, max_push_samples=2560), codec.encode_sessions(2, max_push_samples=25600)
    # A slot holds the columns from the quantiser's left context of its next token to its newest frame.  With `ready` encoder features,
    # 4 * tokens >= ready - 21 and the window starts 4 * 5 columns in front of that: 41 columns behind `ready`, itself encoder_context
    # behind the newest frame.  A push adds at most its frames + 1, the end of the signal 3 more.  The capacity is at least twice that,
    # in whole 32-column units.
    ctx = small.geo.encoder_context + 41
    assert small.capacity % 32 == 0 and small.capacity >= 2 * (ctx + 10 + 1 + 3)
    assert big.capacity - small.capacity >= 2 * 90 - 32
    assert small.width == NFFT + 2560


def test_construction_refuses_what_the_kernel_does_not_take(codec):
    from dmel_codec_amd.configs import build_codec
    with pytest.raises(NotImplementedError, match="codec's own rate"):
        codec.encode_sessions(2, sample_rate=48000)
    assert codec.encode_sessions(2, sample_rate=int(codec.encode_mel_transform.sample_rate)).S == 2
    with pytest.raises(ValueError):
        codec.encode_sessions(0)
    wide = build_codec(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, vocoder=None)
    wide.encoder.residual_channels = 96                          # what the eligibility check reads
    with pytest.raises(NotImplementedError, match="outside"):
        wide.encode_sessions(2)
    bf = build_codec(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, vocoder=None)
    bf.encoder.set_precision("bf16")
    with pytest.raises(NotImplementedError, match="fp32"):
        bf.encode_sessions(2)


def test_the_two_item_entries_are_declared_and_bound():
    from dmel_codec_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dmel_hip.h")).read()
    for name, nargs in (("dmel_wavenet_stream_step_items", 15), ("dmel_stft_window_items_f32", 15)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/dmel_hip.h"
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == len(params) == nargs
    # the host tables are int64 pointers, as the header has them
    _, args = _lib.PROTOTYPES["dmel_wavenet_stream_step_items"]
    assert args[9] is _lib.i64p and args[10] is _lib.i64p and args[13] is _lib.i64p
    _, args = _lib.PROTOTYPES["dmel_stft_window_items_f32"]
    assert [args[i] for i in (4, 5, 10, 11, 12)] == [_lib.i64p] * 5
