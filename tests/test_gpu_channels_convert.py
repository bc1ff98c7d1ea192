"""The interleaved-channel directions of dmel_pcm_convert_items_ch through the C ABI, with guarded buffers.  Every comparison is an
equality of bits against the restatement of the channel rule (tests/channels_ref.py), which tests/test_channels_cpu.py holds to values
pinned by hand, to numpy.mean over the channel-first array and to the fp64 mean rounded once."""
import ctypes as C

import pytest
import torch

import channels_ref as cref
import g711_ref as ref
from test_gpu_g711_convert import CODE, DTYPE, SENT, Guarded, code_master, float_master, words
from test_gpu_pcm_convert import oracle_to_f32, oracle_to_s16, pcm_master

pytestmark = pytest.mark.gpu

FORMATS = ("f32", "s16", "ulaw", "alaw")
F32, S16, ULAW, ALAW = 0, 1, 8, 9
N_MAX = 5000
FLT_MAX = 3.4028234663852886e38


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def call(srcs, dsts, n, sc=None, dc=None, pick=None, sf=None, df=None, old=False):
    """srcs / dsts: Guarded buffers or raw addresses; n: frames per item -> (return code, last error)"""
    from dmel_codec_amd import _lib
    ptr = lambda g: g.t.data_ptr() if isinstance(g, Guarded) else g
    code = lambda g: CODE[g.fmt] if isinstance(g, Guarded) else F32
    k = len(srcs)
    I32 = lambda v: None if v is None else (C.c_int32 * k)(*v)
    sf = [code(g) for g in srcs] if sf is None else sf
    df = [code(g) for g in dsts] if df is None else df
    dev = next(g for g in list(srcs) + list(dsts) if isinstance(g, Guarded)).t.device
    table = torch.empty(4 * k, dtype=torch.int64, device=dev)
    P = C.c_void_p * k
    with torch.cuda.device(dev):
        if old:
            rc = _lib.lib().dmel_pcm_convert_items(P(*[ptr(g) for g in srcs]), I32(sf), P(*[ptr(g) for g in dsts]), I32(df),
                                                   (C.c_int64 * k)(*n), k, table.data_ptr(), _lib.stream_ptr())
        else:
            rc = _lib.lib().dmel_pcm_convert_items_ch(P(*[ptr(g) for g in srcs]), I32(sf), I32(sc), I32(pick), P(*[ptr(g) for g in dsts]),
                                                      I32(df), I32(dc), (C.c_int64 * k)(*n), k, table.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, _lib.lib().dmel_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------ the masters and the restatement of every kind
def mean_master(c: int) -> torch.Tensor:
    """(N_MAX, c) finite fp32 frames: a seeded normal, and frames near FLT_MAX / c whose sum comes close to FLT_MAX without passing it
    -- the sum's rounding, not its overflow, is under test"""
    x = torch.randn(N_MAX, c, generator=torch.Generator().manual_seed(100 + c))
    big = FLT_MAX / c
    j = torch.arange(c, dtype=torch.float32)
    rows = torch.stack([torch.full((c,), big * 0.99), torch.full((c,), -big * 0.99), big * (0.9 + 0.09 * j / c),
                        big * 0.98 * (1 - 2 * (j % 2)), big * 0.5 + j, -big * (0.99 - 0.01 * j / c)]).float()
    for at in (0, 250, 2042, 2049, N_MAX - 6):                    # in the first whole 8, in another wave, around the tile edge, in the tail
        x[at:at + 6] = rows
    assert bool(torch.isfinite(x).all())
    return x


def master(fmt: str, c: int, mean: bool) -> torch.Tensor:
    """(N_MAX, c) source frames of format `fmt` (c = 1: (N_MAX,))"""
    if fmt == "f32":
        m = mean_master(c) if mean else float_master("ulaw", N_MAX * c)[:N_MAX * c].view(N_MAX, c)      # NaN, inf, -0.0, denormals
    elif fmt == "s16":
        m = pcm_master(N_MAX * c).view(N_MAX, c)
    else:
        m = code_master(N_MAX * c).view(N_MAX, c)
    return m[:, 0].contiguous() if c == 1 and not mean else m


# kind: (src format, src channels, pick (-1: mean), dst format, dst channels)
DOWN = [(f, c, k, "f32", 1) for f in FORMATS for c in (2, 3, 8) for k in range(-1, c)] + [(f, 5, -1, "f32", 1) for f in FORMATS]
FAN = [("f32", 1, -1, f, c) for f in FORMATS for c in (2, 3, 8)]
MONO = [("f32", 1, -1, "s16", 1), ("s16", 1, -1, "f32", 1), ("f32", 1, -1, "f32", 1), ("ulaw", 1, -1, "f32", 1), ("alaw", 1, -1, "f32", 1),
        ("f32", 1, -1, "ulaw", 1), ("f32", 1, -1, "alaw", 1)]
_cache = {}


def source_and_want(kind):
    """the kind's source master and the restatement of its whole conversion, computed once; a prefix of frames converts to the prefix"""
    if kind not in _cache:
        sf, sc, k, df, dc = kind
        if sc > 1:
            m = master(sf, sc, k < 0)
            want = cref.downmix(m, sf, None if k < 0 else k)
        elif dc > 1:
            m = master("f32", 1, False)
            want = cref.fan_out(m, dc, df)
        else:
            m = master(sf, 1, False)
            if df in ref.LAWS:
                want = ref.f32_to_law(m, df)
            elif sf in ref.LAWS:
                want = ref.law_to_f32(m, sf)
            else:
                want = oracle_to_s16(m) if df == "s16" else (oracle_to_f32(m) if sf == "s16" else m)
        assert want.dtype == DTYPE[df] and want.shape[0] == N_MAX
        _cache[kind] = (m, want)
    return _cache[kind]


def buffers(kind, n, off, dev):
    sf, sc, k, df, dc = kind
    m, _ = source_and_want(kind)
    return (Guarded(n * sc, sf, dev, off[0], fill=m[:n].reshape(-1)), Guarded(n * dc, df, dev, off[1]))


def check(kind, n, src, dst, tag):
    _, want = source_and_want(kind)
    got = dst.t.cpu()
    assert got.dtype == DTYPE[kind[3]] and torch.equal(words(got), words(want[:n].reshape(-1))), (kind, n, tag)
    assert dst.guards_intact() and src.untouched(), (kind, n, tag)
    return got


def run(kinds, lengths, offsets, dev):
    items = [(kind, n, off) + buffers(kind, n, off, dev) for kind in kinds for n in lengths for off in offsets]
    rc, msg = call([s for *_, s, _ in items], [d for *_, d in items], [n for _, n, *_ in items], sc=[k[1] for k, *_ in items],
                   dc=[k[4] for k, *_ in items], pick=[k[2] for k, *_ in items])
    assert rc == 0, msg
    return {(kind, n, off): check(kind, n, s, d, off) for kind, n, off, s, d in items}


# ------------------------------------------------------------------------------------ each direction
@pytest.mark.parametrize("c", [2, 3, 5, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_downmix_mean_and_every_pick_equal_the_restatement(dev, fmt, c):
    kinds = [k for k in DOWN if k[0] == fmt and k[1] == c]
    assert len(kinds) == (1 if c == 5 else c + 1)                                       # the mean, and every pick index
    got = run(kinds, [4099], [(0, 0), (1, 3)], dev)
    if fmt == "f32":                                                                    # finite in, finite out, close to FLT_MAX
        y = got[((fmt, c, -1, "f32", 1), 4099, (0, 0))]
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0.9 * FLT_MAX / c
    else:                                                                               # the fp64 mean rounded once
        m, _ = source_and_want((fmt, c, -1, "f32", 1))
        assert torch.equal(got[((fmt, c, -1, "f32", 1), 4099, (1, 3))], (cref.to_f32(m[:4099], fmt).double().sum(1) / c).float())


@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fan_out_equals_the_restatement(dev, fmt, c):
    got = run([("f32", 1, -1, fmt, c)], [4099], [(0, 0), (3, 1)], dev)
    for y in got.values():
        y = y.view(4099, c)
        assert all(torch.equal(words(y[:, j]), words(y[:, 0])) for j in range(1, c))    # converted once, stored c times


def test_f32_pick_and_fan_out_move_the_words(dev):
    """-0.0, denormals, inf and NaNs -- a signalling one and a negative one with a payload among them -- pass through a pick and a
    fan-out as the words they are"""
    special = torch.tensor([-0.0, 0.0, 2.0 ** -149, -(2.0 ** -149), 1e-40, -1e-40, 2.0 ** -126, float("inf"), float("-inf"), float("nan"),
                            1.0, -1.0, FLT_MAX, -FLT_MAX, 1.0 - 2.0 ** -24, 3.0])
    nans = torch.tensor([0x7FA00001, 0xFFC12345 - 2 ** 32], dtype=torch.int32)          # any arithmetic would quiet the first
    special = torch.cat([special[:2], nans.view(torch.float32), special[2:]])           # 18 words; x[632:634] are the two: in 637's tail
    x = special.repeat(36)[:640].contiguous()                                           # 640 frames: wide groups and a tail of none
    assert torch.equal(words(x)[632:634], nans)
    for n in (640, 637):
        for off in ((0, 0), (1, 1)):
            for c in (2, 3):
                frames = torch.stack([x.roll(j) for j in range(c)], dim=1)[:n].contiguous()
                for k in range(c):
                    src, dst = Guarded(n * c, "f32", dev, off[0], fill=frames.reshape(-1)), Guarded(n, "f32", dev, off[1])
                    rc, msg = call([src], [dst], [n], sc=[c], pick=[k])
                    assert rc == 0, msg
                    got = dst.t.cpu()
                    assert torch.equal(words(got), words(frames[:, k].contiguous())) and dst.guards_intact() and src.untouched()
                    assert bool((words(got) == -2 ** 31).any()) and bool((words(got) == 1).any())        # -0.0 and 2^-149 are there
                    assert bool((words(got) == 0x7FA00001).any()) and bool((words(got) == 0xFFC12345 - 2 ** 32).any())
                src, dst = Guarded(n, "f32", dev, off[0], fill=x[:n]), Guarded(n * c, "f32", dev, off[1])
                rc, msg = call([src], [dst], [n], dc=[c])
                assert rc == 0, msg
                got = dst.t.cpu().view(n, c)
                assert all(torch.equal(words(got[:, j].contiguous()), words(x[:n])) for j in range(c)) and dst.guards_intact()


# ------------------------------------------------------------------------------------ everything in one launch
LENGTHS = [0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 5000]


def offsets_of(kind):
    """(src, dst) offsets in elements behind a 16-byte boundary: aligned (a stereo item's wide path), odd elements on both sides, and
    -- for the kinds with a wide path -- 8 BYTES on the channel side, which a stereo item must not take for alignment"""
    sf, sc, _, df, dc = kind
    out = [(0, 0), (1, 3)]
    if sc == 2:
        out.append((8 // DTYPE[sf].itemsize, 0))
    if dc == 2:
        out.append((0, 8 // DTYPE[df].itemsize))
    return out


def test_ragged_items_of_every_kind_and_alignment_in_one_launch(dev):
    """every frame count x (downmix-mean and every pick of 4 formats x c in 2, 3, 8; the mean of c = 5; fan-out into 4 formats x c in 2,
    3, 8; the seven mono directions) x alignments, as ONE launch: every output equals the restatement, has the same bits on the wide
    path as off it, and the same bits as the item sent alone and unaligned; sentinels around every buffer are unchanged"""
    kinds = DOWN + FAN + MONO
    assert len(kinds) == 4 * (3 + 4 + 9 + 1) + 12 + 7
    items = [(kind, n, off) + buffers(kind, n, off, dev) for kind in kinds for n in LENGTHS for off in offsets_of(kind)]
    wide = [(s, d) for kind, n, off, s, d in items if n >= 8 and off == (0, 0) and 2 in (kind[1], kind[4])]
    assert wide and all(s.t.data_ptr() % 16 == 0 and d.t.data_ptr() % 16 == 0 for s, d in wide)
    assert any(s.t.data_ptr() % 16 == 8 for kind, n, off, s, d in items if n and kind[1] == 2)        # 8 bytes off: not the wide path
    rc, msg = call([s for *_, s, _ in items], [d for *_, d in items], [n for _, n, *_ in items], sc=[k[1] for k, *_ in items],
                   dc=[k[4] for k, *_ in items], pick=[k[2] for k, *_ in items])
    assert rc == 0, msg
    aligned = {}
    for kind, n, off, s, d in items:
        got = check(kind, n, s, d, off)
        if off == (0, 0):
            aligned[(kind, n)] = got
        else:
            assert torch.equal(words(got), words(aligned[(kind, n)])), (kind, n, off)
    for kind in kinds:                                                                  # and each item alone, off the wide path
        for n in LENGTHS:
            s, d = buffers(kind, n, (1, 3), dev)
            rc, msg = call([s], [d], [n], sc=[kind[1]], dc=[kind[4]], pick=[kind[2]])
            assert rc == 0, msg
            assert torch.equal(words(check(kind, n, s, d, "alone")), words(aligned[(kind, n)])), (kind, n)


# ------------------------------------------------------------------------------------ idle items, the old entry, refusals
def test_idle_launch_writes_nothing(dev):
    src = [Guarded(200, "s16", dev, fill=torch.ones(200, dtype=torch.int16)), Guarded(100, "f32", dev, fill=torch.ones(100))]
    dst = [Guarded(100, "f32", dev), Guarded(300, "ulaw", dev)]
    rc, msg = call(src, dst, [0, 0], sc=[2, 1], dc=[1, 3])
    assert rc == 0 and all(d.untouched() for d in dst), msg
    rc, msg = call([0, src[1]], [dst[0], 0], [0, 0], sc=[2, 1], dc=[1, 3], pick=[1, -1], sf=[S16, F32], df=[F32, ULAW])
    assert rc == 0 and all(d.untouched() for d in dst), msg                             # an idle item's pointers are not looked at
    rc, msg = call(src, dst, [0, 5], sc=[2, 1], dc=[1, 3])                              # an idle item next to a live one
    assert rc == 0 and dst[0].untouched() and dst[1].guards_intact(), msg
    assert torch.equal(dst[1].t[:15].cpu(), torch.full((15,), 0x80, dtype=torch.uint8))
    assert bool((dst[1].t[15:] == SENT[torch.uint8]).all())


def test_old_entry_equals_the_new_one_with_null_tables(dev):
    """a mono launch of all seven directions, ragged, aligned and not: the old entry, the new one with NULL tables and the new one
    with tables of ones write the same bits"""
    outs = []
    for mode in ("old", "null", "ones"):
        items = [(kind, n) + buffers(kind, n, off, dev) for kind in MONO for n in (0, 9, 2049, 5000) for off in ((0, 0), (1, 3))]
        k = len(items)
        ones = dict(sc=[1] * k, dc=[1] * k, pick=[-1] * k) if mode == "ones" else {}
        rc, msg = call([s for *_, s, _ in items], [d for *_, d in items], [n for _, n, *_ in items], old=mode == "old", **ones)
        assert rc == 0, msg
        outs.append([check(kind, n, s, d, mode) for kind, n, s, d in items])
    for a, b, c in zip(*outs):
        assert torch.equal(words(a), words(b)) and torch.equal(words(a), words(c))


def test_refusals_launch_nothing(dev):
    f = Guarded(64, "f32", dev, fill=torch.zeros(64))
    s = Guarded(64, "s16", dev, fill=torch.zeros(64, dtype=torch.int16))
    u = Guarded(64, "ulaw", dev, fill=torch.full((64,), 0xFF, dtype=torch.uint8))
    df, df2, ds, du = Guarded(64, "f32", dev), Guarded(64, "f32", dev), Guarded(64, "s16", dev), Guarded(64, "alaw", dev)
    # item 0 of every case is a valid stereo s16 -> f32 item of 8 frames
    cases = {"src_ch 0": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 0]),
             "src_ch 9": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 9]),
             "dst_ch 9": dict(srcs=[s, f], dsts=[df, ds], sc=[2, 1], dc=[1, 9]),
             "2 -> 2": dict(srcs=[s, f], dsts=[df, ds], sc=[2, 2], dc=[1, 2]),
             "pick 2 of 2": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 2], pick=[1, 2]),
             "pick -2": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 2], pick=[1, -2]),
             "pick of a mono source": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 1], pick=[-1, 0]),
             "stereo s16 -> mono s16": dict(srcs=[s, s], dsts=[df, ds], sc=[2, 2]),
             "stereo ulaw -> mono alaw": dict(srcs=[s, u], dsts=[df, du], sc=[2, 2]),
             "stereo s16 -> mono ulaw": dict(srcs=[s, s], dsts=[df, du], sc=[2, 2]),
             "NULL stereo src": dict(srcs=[s, 0], dsts=[df, df2], sc=[2, 2], sf=[S16, S16], df=[F32, F32]),
             "NULL fan-out dst": dict(srcs=[s, f], dsts=[df, 0], sc=[2, 1], dc=[1, 2], sf=[S16, F32], df=[F32, S16]),
             "odd stereo s16 src": dict(srcs=[s, s.t.data_ptr() + 1], dsts=[df, df2], sc=[2, 2], sf=[S16, S16], df=[F32, F32]),
             "f32 fan-out dst off by 2": dict(srcs=[s, f], dsts=[df, df2.t.data_ptr() + 2], sc=[2, 1], dc=[1, 2], sf=[S16, F32], df=[F32, F32]),
             "negative n": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 2], n=[8, -1]),
             "n * c reaches 2^40": dict(srcs=[s, u], dsts=[df, df2], sc=[2, 8], n=[8, 1 << 37])}
    for name, kw in cases.items():
        rc, msg = call(**{"n": [8, 8], **kw})
        assert rc == -1 and "item 1" in msg, (name, rc, msg)
        assert all(d.untouched() for d in (df, df2, ds, du)), name
    rc, msg = call([s], [df], [8], sc=[2])                                              # and the valid item alone converts
    assert rc == 0 and torch.equal(df.t[:8].cpu(), torch.zeros(8)) and df.guards_intact(), msg
    assert bool((df.t[8:] == SENT[torch.float32]).all())
