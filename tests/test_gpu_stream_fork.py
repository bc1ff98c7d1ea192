"""dmel_stream_fork_items through the C ABI (csrc/small_ops.hip): the columns [lo, hi) of every channel of a source item copied to
another item of the same hist / skip / cond / mel buffers, one launch for all rows.  Every comparison is torch.equal against a torch
slice copy; the buffers are filled with distinct values and every element outside the windows must be what it was."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

L, N, CH, CCOND, COUT = 2, 6, 5, 3, 2                  # three sources (items 0 .. 2) and three shadows (items 3 .. 5)
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def buffers(cap, dev, seed):
    """hist, skip, cond, mel: every element distinct from its neighbours in the other items (a sentinel ramp plus noise)"""
    g = torch.Generator().manual_seed(seed)
    shapes = [(L + 1, N, CH, cap), (N, CH, cap), (N, CCOND, cap), (N, COUT, cap)]
    return [(torch.randn(s, generator=g) - 777.0 * (i + 1)).to(dev) for i, s in enumerate(shapes)]


def fork(bufs, cap, rows, n_items=N):
    """rows: [(src, dst, lo, hi)] -> (return code, message); the host tables are overwritten right after the call"""
    from dmel_codec_amd import _lib
    hist, skip, cond, mel = bufs
    R = len(rows)
    I64 = C.c_int64 * R
    cols = [I64(*[r[i] for r in rows]) for i in range(4)]
    table = torch.empty(5 * R, dtype=torch.int32, device=hist.device)
    with torch.cuda.device(hist.device):
        rc = _lib.lib().dmel_stream_fork_items(hist.data_ptr(), skip.data_ptr(), cond.data_ptr(), mel.data_ptr(), L, n_items, CH, CCOND, COUT,
                                               cap, R, *cols, table.data_ptr(), _lib.stream_ptr())
    msg = _lib.lib().dmel_last_error().decode(errors="replace") if rc else ""
    for c in cols:
        for i in range(R):
            c[i] = -1
    torch.cuda.synchronize()
    return rc, msg


def expected(bufs, rows):
    want = [t.clone() for t in bufs]
    for src, dst, lo, hi in rows:
        want[0][:, dst, :, lo:hi] = bufs[0][:, src, :, lo:hi]
        for w, t in zip(want[1:], bufs[1:]):
            w[dst, :, lo:hi] = t[src, :, lo:hi]
    return want


# every window of the list, three rows at a time: sources 0 .. 2 into shadows 3 .. 5 (so that with cap = 99 rows of both parities of
# alignment meet every window), once more with the shadows in another order
def window_sets(cap):
    wins = [(0, 0), (0, 1), (3, 4), (3, 36), (4, 96), (1, 98), (0, cap)]
    wins = [w for w in wins if w[1] <= cap]
    for shift in range(3):
        for a in range(0, len(wins), 3):
            trio = (wins + wins)[a:a + 3]
            yield [(i, 3 + (i + shift) % 3, lo, hi) for i, (lo, hi) in enumerate(trio)]


@pytest.mark.parametrize("cap", [96, 99])
def test_fork_equals_slice_copy_and_touches_nothing_else(dev, cap):
    seen = set()
    for n, rows in enumerate(window_sets(cap)):
        bufs = buffers(cap, dev, 10 * cap + n)
        want = expected(bufs, rows)
        rc, msg = fork(bufs, cap, rows)
        assert rc == 0, msg
        for name, got, w in zip(("hist", "skip", "cond", "mel"), bufs, want):
            assert torch.equal(got, w), f"{name} differs for rows {rows}"        # the windows AND every element outside them
        seen |= {(lo, hi) for _, _, lo, hi in rows}
    assert {(0, 0), (0, 1), (3, 4), (3, 36), (4, 96), (0, cap)} <= seen and ((1, 98) in seen) == (cap >= 98)


def test_one_source_forked_twice_and_all_rows_idle(dev):
    cap = 99
    bufs = buffers(cap, dev, 5)
    rows = [(1, 3, 4, 40), (1, 4, 0, 99)]
    want = expected(bufs, rows)
    rc, msg = fork(bufs, cap, rows)
    assert rc == 0, msg
    assert all(torch.equal(a, b) for a, b in zip(bufs, want))
    before = [t.clone() for t in bufs]
    rc, msg = fork(bufs, cap, [(0, 3, 7, 7), (1, 4, 0, 0)])
    assert rc == 0, msg
    assert all(torch.equal(a, b) for a, b in zip(bufs, before))


def test_refusals_leave_every_buffer_alone(dev):
    cap = 96
    bufs = buffers(cap, dev, 9)
    before = [t.clone() for t in bufs]
    good = (0, 3, 4, 40)

    def refused(rows, *words):
        rc, msg = fork(bufs, cap, rows)
        assert rc == EINVAL, (rc, msg)
        for w in words:
            assert w in msg, msg
        assert all(torch.equal(a, b) for a, b in zip(bufs, before))

    refused([good, (2, 2, 0, 8)], "row 1", "itself")                      # src == dst
    refused([good, (3, 4, 0, 8)], "row 0", "source")                      # a dst that is another row's src
    refused([good, (1, 3, 0, 8)], "row 1", "destination")                 # a dst that is another row's dst
    refused([(1, 4, 0, 8), (0, 1, 0, 8)], "row 1", "source")
    refused([good, (1, 4, -1, 8)], "row 1", "window")                     # windows outside [0, cap]
    refused([good, (1, 4, 0, cap + 1)], "row 1", "window")
    refused([good, (1, 4, 9, 8)], "row 1", "window")
    refused([good, (1, N, 0, 8)], "row 1", "outside")                     # items outside [0, N)
    refused([good, (-1, 4, 0, 8)], "row 1", "outside")
    rc, msg = fork(bufs, cap, [good])
    assert rc == 0, msg
    assert all(torch.equal(a, b) for a, b in zip(bufs, expected(before, [good])))
