"""What EncodeSessions and DecodeSessions share as pools of slots (models/stream_park.py: ParkingPool), the part that needs no GPU:
the snapshot format pinned to literal values, the wire options (rate, sample format, channels) refused with one message from both
doors -- open() and restore() --, and refused calls that leave the pool as it was."""
import copy

import pytest

from test_stream_park_cpu import codec, edited  # noqa: F401  (the stand-in codec of the park tests)


def encode_pool(codec):
    return codec.encode_sessions(3, max_push_samples=4096, sample_rates=[48000, 8000])


def decode_pool(codec):
    return codec.decode_sessions(3, max_push_tokens=16, early_emit=True, crossfade_samples=4, output_sample_rates=[48000])


OPEN_RATE = {"encode": "sample_rate", "decode": "output_sample_rate"}
POOLS = {"encode": encode_pool, "decode": decode_pool}
LISTS = {"encode": ("origin", "s0", "tail", "rate", "fmt", "ch", "pick", "_fresh"),
         "decode": ("origin", "rate", "fmt", "ch", "fade", "has_tail", "tok_origin", "n_noise", "_fresh")}


def state_of(pool, kind):
    return pool.open_slots, [list(getattr(pool, name)) for name in LISTS[kind]], [pool.rs.is_open(s) for s in range(pool.S)]


# ------------------------------------------------------------------------------------------------------------ the pinned format
def test_encode_snapshot_format_is_pinned(codec):
    pool = encode_pool(codec)
    pool.open()
    s = pool.open(sample_rate=48000, sample_format="s16", channels=2, channel=1)
    for n in (4096, 1000, 0, 4096):
        pool.sched[s].step(n)
    pool.s0[s], pool.tail[s] = 8000, 700
    meta = pool._park_meta(s)
    assert meta == {
        'version': 1, 'kind': 'encode',
        'geometry': {'hop': 256, 'n_fft': 1024, 'dilations': [1, 2], 'downsample_factor': [2, 2], 'dw_kernel': 7},
        'G': 8, 'C': 70, 'L': 2, 'n_mels': 80, 'codec_rate': 24000, 'rate': 48000, 'sample_format': 's16', 'channels': 2, 'channel': 1,
        'lookahead': None, 'fade': 0, 'has_tail': False, 's0': 8000, 'tail': 700,
        'schedule': {'samples': 9192, 'frames': 34, 'levels': [34, 33, 31], 'tokens': 3, 'finished': False},
        'resampler': {'pair': [48000, 24000], 's0': 0, 'fill': 0, 'sched': {'samples': 0, 'emitted': 0, 'finished': False}},
        'window': [0, 34]}
    assert pool._park_shapes(meta) == [('mel', 80, 34), ('hist.0', 560, 34), ('hist.1', 560, 34), ('hist.2', 560, 34), ('skip', 560, 34),
                                       ('feat', 560, 34), ('samples', 1, 700), ('resampler', 1, 0)]


def test_decode_snapshot_format_is_pinned(codec):
    pool = decode_pool(codec)
    pool.open()
    s = pool.open(output_sample_rate=48000, sample_format="ulaw", channels=2, lookahead_frames=8, crossfade_samples=4)
    for n in (16, 3, 0, 16):
        pool.sched[s].step(n)
    pool.tok_origin[s], pool.n_noise[s], pool.has_tail[s] = 27, 16, True
    meta = pool._park_meta(s)
    assert meta == {
        'version': 1, 'kind': 'decode', 'geometry': {'factor': 4, 'dilations': [1], 'voc_halo': 25, 'quant_halo_tokens': 4},
        'G': 8, 'C': 560, 'L': 1, 'cond_channels': 560, 'n_mels': 80, 'up': 8, 'return_audios': True, 'voc_rate': 24000, 'rate': 48000,
        'sample_format': 'ulaw', 'channels': 2, 'channel': None, 'lookahead': 8, 'fade': 4, 'has_tail': True, 'tok_origin': 27,
        'n_noise': 16,
        'schedule': {'lookahead': 8, 'fade_frames': 1, 'emitted': 132,
                     'exact': {'tokens': 35, 'z_valid': 124, 'levels': [124, 123], 'emitted': 98, 'tok_origin': 27, 'finished': False}},
        'resampler': {'pair': [24000, 48000], 's0': 0, 'fill': 0, 'sched': {'samples': 0, 'emitted': 0, 'finished': False}},
        'window': [72, 124]}
    assert pool._park_shapes(meta) == [('hist.0', 560, 52), ('hist.1', 560, 52), ('skip', 560, 52), ('cond', 560, 52), ('mel', 80, 52),
                                       ('tokens', 8, 8), ('noise', 560, 16), ('fade_tail', 1, 4), ('resampler', 1, 0)]


# ------------------------------------------------------------------------------------------------------------ one message, two doors
def refusals(kind):
    rates = "(24000, 8000, 48000)" if kind == "encode" else "(24000, 48000)"
    option = "sample_rates" if kind == "encode" else "output_sample_rates"
    return [(dict(rate=16000), f"a session at 16000 Hz: the pool was built for {rates} Hz (declare the rate in {option}=)"),
            (dict(sample_format="s24"), "unknown sample format 's24': expected one of ['alaw', 'f32', 's16', 'ulaw']"),
            (dict(channels=9), "channels=9: expected an int in 1 .. 8")]


@pytest.mark.parametrize("kind", ["encode", "decode"])
def test_wire_options_are_refused_alike_by_open_and_by_restore(codec, kind):
    pool = POOLS[kind](codec)
    first = pool.open()
    snap = pool.snapshot([first])[first]
    before, scheds = copy.deepcopy(state_of(pool, kind)), list(pool.sched)
    for change, text in refusals(kind):
        opts = {OPEN_RATE[kind] if k == "rate" else k: v for k, v in change.items()}
        with pytest.raises(ValueError) as at_open:
            pool.open(**opts)
        with pytest.raises(ValueError) as at_restore:
            pool.restore([edited(snap, **change)])
        assert str(at_open.value) == text and str(at_restore.value) == text
        assert type(at_open.value) is ValueError and type(at_restore.value) is ValueError
        assert state_of(pool, kind) == before
        assert all(x is y for x, y in zip(pool.sched, scheds))             # the very schedules, not equal ones


@pytest.mark.parametrize("kind", ["encode", "decode"])
def test_refused_calls_leave_the_lowest_free_slot_free(codec, kind):
    pool = POOLS[kind](codec)
    a, b, c = pool.open(), pool.open(), pool.open()
    assert (a, b, c) == (0, 1, 2)
    with pytest.raises(RuntimeError) as full:
        pool.open()
    assert str(full.value) == "all 3 slots are taken"
    snap = pool.snapshot([c])[c]
    pool.drop(b)
    pool.drop(a)
    for change, _ in refusals(kind):
        with pytest.raises(ValueError):
            pool.open(**{OPEN_RATE[kind] if k == "rate" else k: v for k, v in change.items()})
        with pytest.raises(ValueError):
            pool.restore([edited(snap, **change)])
    with pytest.raises(ValueError):
        pool.restore([snap, edited(snap, channels=9)])                      # one bad snapshot among good ones: none is restored
    assert pool.open_slots == [c]
    assert pool.open() == a
    assert pool.restore([snap]) == [b]
    with pytest.raises(RuntimeError, match="free"):
        pool.restore([snap])
    assert pool.open_slots == [a, b, c]
