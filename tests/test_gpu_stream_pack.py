"""dmel_stream_pack_items through the C ABI (csrc/small_ops.hip): R independent 2-D copies of 4-byte words in one launch, the gather
and the scatter behind snapshot / restore of live sessions.  Every comparison is torch.equal on int32 views against torch slice
copies; the buffers are filled with distinct words -- NaN bit patterns with payloads and negative ids among them -- and every word
outside the windows must be what it was."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, PITCHES = (1, 5), (96, 99)
SPECIAL = [0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC12345, 0xFF800000, 0x7F800000, 0x80000000, 0xFFFFFFFF, 0x00000001, 0x807FFFFF]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def words(n, seed, dev):
    """n distinct-looking int32 words: random bits, every tenth word one of the NaN / infinity / denormal / negative-id patterns"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    sp = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in SPECIAL], dtype=torch.int64).to(torch.int32)
    w[::10] = sp[torch.arange(w[::10].numel()) % len(SPECIAL)]
    return w.to(dev)


def pack(items, dev, clobber=True):
    """items: [(src tensor view | None, dst tensor view | None, rows, cols, src pitch, dst pitch)] -> (return code, message).  The
    addresses are those of the views' first words; the host tables are overwritten right after the call."""
    from dmel_codec_amd import _lib
    R = len(items)
    P, I64 = C.c_void_p * R, C.c_int64 * R
    src = P(*[None if it[0] is None else it[0].data_ptr() for it in items])
    dst = P(*[None if it[1] is None else it[1].data_ptr() for it in items])
    cols = [I64(*[it[i] for it in items]) for i in range(2, 6)]
    table = torch.empty(8 * R, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().dmel_stream_pack_items(src, dst, *cols, R, table.data_ptr(), _lib.stream_ptr())
    msg = _lib.lib().dmel_last_error().decode(errors="replace") if rc else ""
    if clobber:
        for i in range(R):
            src[i] = dst[i] = 0xDEAD0
            for c in cols:
                c[i] = -1
    torch.cuda.synchronize()
    return rc, msg


def launches(fn):
    from dmel_codec_amd import _lib
    _lib.prof_reset(); _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        n = _lib.prof_read("stream_pack")["launches"]
    finally:
        _lib.prof_enable(False); _lib.prof_reset()
    return n, out


def window(buf, base, rows, cols, pitch):
    """the (rows, cols) window of the flat buffer that starts at word `base`, rows `pitch` words apart"""
    return torch.as_strided(buf, (rows, cols), (pitch, 1), base)


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("offset", [0, 1])
def test_pack_then_unpack_equals_slice_copies_and_touches_nothing_else(dev, pitch, offset):
    """every (rows, cols) of the list as ONE launch of descriptors: state rows of `pitch` words -> a dense blob -> rows of pitch 131.
    offset: words between a 16-byte boundary and the first word of every window and of the blob."""
    cases = [(r, c) for r in ROWS for c in (0, 1, 3, 4, 33, 96, pitch)]
    # a state buffer per case, 256-byte aligned by the allocator; windows start `offset` words in (+ 4 per case: every lane phase)
    states = [words(6 * pitch + 8, 100 * pitch + i, dev) for i in range(len(cases))]
    starts = [offset + 4 * (i % 3) for i in range(len(cases))]
    dense = [r * c for r, c in cases]
    at = [offset + sum(dense[:i]) for i in range(len(cases))]              # dense, back to back: most segments start unaligned
    blob = words(offset + sum(dense) + 5, 7 + pitch, dev)
    blob0, states0 = blob.clone(), [s.clone() for s in states]
    items = [(window(s, b, r, max(c, 1), pitch)[:, :c], blob[a:], r, c, pitch, c)
             for s, b, a, (r, c) in zip(states, starts, at, cases)]
    n, (rc, msg) = launches(lambda: pack(items, dev))
    assert rc == 0 and n == 1, (rc, msg, n)
    want = blob0.clone()
    for s, b, a, (r, c) in zip(states0, starts, at, cases):
        want[a:a + r * c] = window(s, b, r, c, pitch).reshape(-1)
    assert torch.equal(blob, want)                                          # the segments AND every word outside them
    assert all(torch.equal(s, s0) for s, s0 in zip(states, states0))        # a source is only read
    # ---- unpack: the same entry, roles swapped, into rows of another pitch
    outs = [words(6 * 131 + 8, 900 + i, dev) for i in range(len(cases))]
    outs0 = [o.clone() for o in outs]
    ostart = [(offset + i) % 5 for i in range(len(cases))]
    items = [(blob[a:], window(o, b, r, max(c, 1), 131)[:, :c], r, c, c, 131) for o, b, a, (r, c) in zip(outs, ostart, at, cases)]
    n, (rc, msg) = launches(lambda: pack(items, dev))
    assert rc == 0 and n == 1, (rc, msg, n)
    for o, o0, b, s0, sb, (r, c) in zip(outs, outs0, ostart, states0, starts, cases):
        w = o0.clone()
        window(w, b, r, c, 131).copy_(window(s0, sb, r, c, pitch))
        assert torch.equal(o, w), (r, c, pitch, offset)
    assert torch.equal(blob, want)


def test_both_paths_move_the_same_bits_and_floats_are_never_formed(dev):
    """one payload through the 16-byte path (aligned bases, pitches that are multiples of 4) and through the word path (one word off):
    NaN payloads, signalling NaNs, infinities, denormals and int32 ids all come out bit for bit, as float32 tensors as well"""
    rows, cols, pitch = 5, 4 * 64 + 4 * 50 + 3, 460                       # two column tiles, whole vectors and a tail of 3 words
    src = words(rows * pitch + 8, 1, dev)
    outs = {}
    for name, (so, do, dp) in {"vector": (0, 0, 464), "word": (1, 0, 464), "word_dst": (0, 3, 464), "word_pitch": (0, 0, 461)}.items():
        a = src.clone() if so == 0 else torch.cat([src[:1], src])          # the same payload, one word further
        out = torch.full((rows * dp + 8,), -5, dtype=torch.int32, device=dev)
        rc, msg = pack([(a[so:], out[do:], rows, cols, pitch, dp)], dev)
        assert rc == 0, msg
        got = window(out, do, rows, cols, dp)
        assert torch.equal(got, window(src, 0, rows, cols, pitch)), name
        untouched = out.clone()
        window(untouched, do, rows, cols, dp).fill_(-5)
        assert bool((untouched == -5).all()), name
        outs[name] = got.clone()
    assert all(torch.equal(outs["vector"], o) for o in outs.values())
    # the same call on float32 storage: the NaN payloads are still those words
    f = src.view(torch.float32)
    out = torch.zeros(rows * cols, dtype=torch.float32, device=dev)
    rc, msg = pack([(f, out, rows, cols, pitch, cols)], dev)
    assert rc == 0, msg
    assert torch.equal(out.view(torch.int32).view(rows, cols), window(src, 0, rows, cols, pitch))
    assert bool(torch.isnan(out).any())


def test_more_rows_than_a_tile_and_descriptors_of_every_size_in_one_grid(dev):
    """row tiles (8 rows) and column tiles (256 words) that end inside a descriptor, idle descriptors between live ones"""
    shapes = [(9, 257), (0, 5), (1, 1), (17, 110), (3, 0), (8, 256), (70, 399), (0, 0)]
    srcs = [words(max(r, 1) * 400 + 4, 50 + i, dev) for i, (r, c) in enumerate(shapes)]
    dsts = [torch.full((max(r, 1) * 404 + 4,), 7, dtype=torch.int32, device=dev) for r, c in shapes]
    items = [(s, d, r, c, 400, 404) for s, d, (r, c) in zip(srcs, dsts, shapes)]
    n, (rc, msg) = launches(lambda: pack(items, dev))
    assert rc == 0 and n == 1, (rc, msg, n)
    for s, d, (r, c) in zip(srcs, dsts, shapes):
        w = torch.full_like(d, 7)
        window(w, 0, r, c, 404).copy_(window(s, 0, r, c, 400))
        assert torch.equal(d, w), (r, c)


def test_all_idle_launches_nothing_and_refusals_leave_the_buffers_alone(dev):
    a, b = words(1000, 3, dev), words(1000, 4, dev)
    a0, b0 = a.clone(), b.clone()
    n, (rc, msg) = launches(lambda: pack([(None, None, 0, 9, 0, 0), (a, b, 4, 0, 1, 1), (None, b, 0, 0, -7, -7)], dev))
    assert rc == 0 and n == 0, (rc, msg, n)
    good = (a, b, 5, 33, 96, 33)
    for items, word in (([good, (a, b[500:], 2, 40, 39, 40)], "row 1"), ([good, (a, b[500:], 2, 40, 40, 39)], "row 1"),
                        ([(a, None, 1, 4, 4, 4), good], "row 0"), ([good, (a, b[500:], -1, 4, 4, 4)], "row 1")):
        n, (rc, msg) = launches(lambda: pack(items, dev))
        assert rc == -1 and n == 0 and word in msg, (rc, msg, n)
    assert torch.equal(a, a0) and torch.equal(b, b0)
