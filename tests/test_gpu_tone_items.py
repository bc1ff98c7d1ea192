"""dmel_tone_items on the GPU (csrc/small_ops.hip) against the host rule (dmel_codec_amd/utils/tones.py: render) and against plain
copies, bit for bit: every destination lies in one arena of guard words, and the whole arena is compared with the one built on the
host -- the parts' bits where parts are, the guards everywhere else."""
import numpy as np
import pytest
import torch

from dmel_codec_amd import _lib
from dmel_codec_amd.utils import tones

pytestmark = pytest.mark.gpu

GUARD = 0x7fc0dead
RATES = [8000, 24000, 44100]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def launch(specs, rate, dev, seed=0, gap=8):
    """specs: ("tone", program, dst offset) | ("copy", n, dst offset, source offset); offsets in floats off a 16-byte boundary.
    gap: guard words between two destinations (0: the destinations follow each other, as the parts of a spliced piece do)
    -> (the arena after the launch, the arena the host expects), int32 on the CPU"""
    g = np.random.default_rng(seed)
    want, at = [], 0
    for spec in specs:
        n = tones.length(spec[1]) if spec[0] == "tone" else spec[1]
        if gap or not want:
            at = (at + 8 + 3) // 4 * 4 + spec[2]                             # a 16-byte boundary behind the guards, then the offset
        want.append((at, tones.render(spec[1], rate).view(np.int32) if spec[0] == "tone"
                     else g.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)))       # any bits: NaNs and denormals too
        at += n
    total = at + 16
    host = np.full(total, GUARD, dtype=np.int64).astype(np.int32)
    for a, w in want:
        host[a:a + len(w)] = w
    arena = torch.full((total,), GUARD, dtype=torch.int32, device=dev)
    assert arena.data_ptr() % 16 == 0
    fl = arena.view(torch.float32)
    parts, keep = [], []
    for spec, (a, w) in zip(specs, want):
        if spec[0] == "tone":
            parts.append((fl[a:a + len(w)], tones.check_program(spec[1], rate)))
        else:
            src = torch.zeros(len(w) + 8, dtype=torch.int32, device=dev)
            src[spec[3]:spec[3] + len(w)] = torch.from_numpy(w)
            keep.append(src)
            parts.append((fl[a:a + len(w)], src.view(torch.float32)[spec[3]:spec[3] + len(w)]))
            assert len(w) == 0 or (parts[-1][1].data_ptr() % 16, parts[-1][0].data_ptr() % 16) == (4 * spec[3], 4 * (a % 4))
    tones.tone_items(parts, rate)
    torch.cuda.synchronize()
    return arena.cpu().numpy(), host


def seg(on, ramp, off, dual, k=0):
    rows, cols = (697, 770, 852, 941), (1209, 1336, 1477, 1633)
    return (rows[k % 4], cols[(k // 4) % 4] if dual else 0, 0.31, 0.39 if dual else 0.0, on, off, ramp)


@pytest.mark.parametrize("rate", RATES)
def test_tone_parts_equal_render(dev, rate):
    specs, k = [], 0
    for on in (1, 1023, 1024, 1025, 5000):
        for ramp in (0, 1, 24):
            for off in (0, 7):
                if ramp <= on // 2:
                    specs.append(("tone", [seg(on, ramp, off, k % 2 == 0, k)], k % 4))
                    k += 1
    for ramp, on in ((1, 2), (24, 48), (4096, 8192)):                        # on == 2 * ramp: the two ramps meet
        for off in (0, 7):
            specs.append(("tone", [seg(on, ramp, off, k % 2 == 1, k)], k % 4))
            k += 1
    # 64 segments in one part, of every kind, and a program whose segments straddle tiles
    specs.append(("tone", [seg((1, 2, 48, 300, 1025)[j % 5], (0, 1, 24, 24, 0)[j % 5], (0, 7, 3)[j % 3], j % 2 == 0, j) for j in range(64)], 3))
    specs.append(("tone", [seg(1000, 24, 24, True, 5), seg(2000, 0, 0, False, 6), seg(96, 48, 1, True, 7)], 1))
    assert len(specs) >= 30
    got, want = launch(specs, rate, dev)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} words differ, the first at {bad[0]}: {got[bad[0]]:#x} != {want[bad[0]]:#x}"


def test_copy_parts_at_every_offset_on_both_sides(dev):
    specs = [("copy", n, d, s) for n in (0, 1, 3, 4, 5, 1024, 1029) for d in range(4) for s in range(4)]
    got, want = launch(specs, 24000, dev, seed=1)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} words differ, the first at {bad[0]}"
    assert (want != GUARD).sum() >= 16 * (1 + 3 + 4 + 5 + 1024 + 1029) - 8   # the parts are there (a random word may be the guard's)


@pytest.mark.parametrize("rate, first", [(8000, 0), (24000, 1), (44100, 3)])
def test_forty_parts_that_follow_each_other(dev, rate, first):
    """spliced pieces: speech | tone | speech | tone ... with consecutive destinations, no guard between them"""
    keys = tones.dtmf_program("159D", rate, 20, 10)
    beep = tones.tone_program(1000, 30, rate, ramp_ms=3)
    specs = [("copy", 2, first, 2)]
    for j in range(13):
        specs += [("copy", (5, 1029, 0, 1, 1024, 3)[j % 6], 0, j % 4), ("tone", keys if j % 2 else beep, 0), ("copy", (4, 0, 777)[j % 3], 0, (j + 1) % 4)]
    assert len(specs) == 40
    got, want = launch(specs, rate, dev, seed=2, gap=0)
    assert np.array_equal(got, want)
    assert np.all(got[:8 + first] == np.int32(GUARD)) and np.all(got[-16:] == np.int32(GUARD))


def test_parts_that_share_segments_at_one_offset(dev):
    """the table holds one prefix sum per segment: parts may name the same segments where each begins at the same sample of both
    -- the same range twice, and a range with the same first segment -- and then every part is its own rendering"""
    import ctypes as C
    rate = 24000
    program = tones.check_program([seg(1000, 24, 24, True, 5), seg(2000, 0, 5, False, 6), seg(96, 48, 1, True, 7)], rate)
    ramps, ramp_off = tones.ramp_arena([s[6] for s in program], dev)
    words = tones.segment_words(program, ramp_off)
    counts = (3, 3, 1, 2)                                                    # segments [0, 3), [0, 3), [0, 1), [0, 2)
    lens = [tones.length(program[:c]) for c in counts]
    out = torch.full((sum(lens) + 4 * 8 + 8,), GUARD, dtype=torch.int32, device=dev)
    want, at, dst = out.cpu().numpy().copy(), 8, []
    for n, c in zip(lens, counts):
        want[at:at + n] = tones.render(program[:c], rate).view(np.int32)
        dst.append(out.data_ptr() + 4 * at)
        at += n + 8
    sine = torch.tensor(tones.sine_table(rate)).to(dev)
    table = torch.empty(tones.table_words(4, 3), dtype=torch.int64, device=dev)
    P = C.c_void_p * 4
    _lib.check(_lib.lib().dmel_tone_items(P(*dst), P(None, None, None, None), (C.c_int64 * 4)(*lens), (C.c_int32 * 4)(0, 0, 0, 0),
                                          (C.c_int32 * 4)(*counts), 4, (C.c_int32 * len(words))(*words), 3, sine.data_ptr(), rate,
                                          ramps.data_ptr(), int(ramps.numel()), table.data_ptr(), _lib.stream_ptr()), "tone_items")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_the_tones_family_counts_launches(dev):
    fl = torch.zeros(64, dtype=torch.float32, device=dev)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        tones.tone_items([(fl[:0], fl[:0]), (fl[4:4], fl[9:9])], 24000)      # every part empty: nothing is launched
        torch.cuda.synchronize()
        assert _lib.prof_read("tones")["launches"] == 0
        tones.tone_items([(fl[:5], fl[32:37]), (fl[5:8], tones.tone_program(440, 0.125, 24000, ramp_ms=0)), (fl[8:8], fl[8:8])], 24000)
        torch.cuda.synchronize()
        assert _lib.prof_read("tones")["launches"] == 1
    finally:
        _lib.prof_enable(False)
        _lib.prof_reset()
    assert torch.equal(fl[5:8].cpu(), torch.from_numpy(tones.render(tones.tone_program(440, 0.125, 24000, ramp_ms=0), 24000)))


def test_wrapper_refuses(dev):
    fl = torch.zeros(64, dtype=torch.float32, device=dev)
    beep = tones.tone_program(440, 0.125, 24000, ramp_ms=0)                  # three samples
    with pytest.raises(ValueError, match="no part"):
        tones.tone_items([], 24000)
    with pytest.raises(ValueError, match="program of 3 samples"):
        tones.tone_items([(fl[:4], beep)], 24000)
    with pytest.raises(ValueError, match="source"):
        tones.tone_items([(fl[:4], fl[8:11])], 24000)
    with pytest.raises(ValueError, match="dst"):
        tones.tone_items([(fl[:8:2], fl[8:12])], 24000)
    with pytest.raises(ValueError, match="table"):
        tones.tone_items([(fl[:3], beep)], 24000, table=torch.empty(10, dtype=torch.int64, device=dev))
    assert torch.count_nonzero(fl) == 0
