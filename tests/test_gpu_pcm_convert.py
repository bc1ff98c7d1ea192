"""dmel_pcm_convert_items through the C ABI, with guarded buffers.  Every comparison is torch.equal (or equality of the words).

The rounding oracle is torch on the CPU:

    clamp(round(nan_to_num(y, nan=0) * 32768), -32768, 32767).to(int16)

torch.round rounds halves to even; the oracle itself is checked against a hand-written list (no GPU needed)."""
import ctypes as C

import pytest
import torch

GUARD = 64                      # elements in front of and behind every view: 128 bytes of int16, 256 of fp32 -- both multiples of 16
SENT = {torch.int16: -12345, torch.float32: -777.0}
F32, S16 = 0, 1                 # DMEL_SAMPLE_F32, DMEL_SAMPLE_S16
CODE = {torch.float32: F32, torch.int16: S16}


def oracle_to_s16(y: torch.Tensor) -> torch.Tensor:
    y = y.detach().cpu().float()
    return torch.clamp(torch.round(torch.nan_to_num(y, nan=0.0) * 32768), -32768, 32767).to(torch.int16)


def oracle_to_f32(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().float() / 32768


def test_oracle_rounds_halves_to_even_and_clamps():
    hand = [(0.5, 0), (-0.5, 0), (1.5, 2), (2.5, 2), (-1.5, -2), (-2.5, -2), (3.5, 4), (32767.5, 32767), (32766.5, 32766),
            (-32768.5, -32768), (-32767.5, -32768), (40000.0, 32767), (-40000.0, -32768), (0.49, 0), (0.51, 1)]
    y = torch.tensor([v / 32768 for v, _ in hand], dtype=torch.float32)
    assert torch.equal(y * 32768, torch.tensor([v for v, _ in hand]))                   # every input is exact in fp32
    assert oracle_to_s16(y).tolist() == [w for _, w in hand]
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 1e-40, 1.0, -1.0])
    assert oracle_to_s16(special).tolist() == [0, 32767, -32768, 0, 0, 32767, -32768]
    assert oracle_to_f32(torch.tensor([-32768, 32767, 1], dtype=torch.int16)).tolist() == [-1.0, 1.0 - 2.0 ** -15, 2.0 ** -15]


def special_floats() -> torch.Tensor:
    """every tie k + 0.5 for k in -4 .. 4 and near +-32767, +-1.0, +-(1 - 2^-16), values past full scale, +-inf, NaN, -0.0, denormals"""
    ties = [k + 0.5 for k in range(-4, 5)] + [32765.5, 32766.5, 32767.5, 32768.5, -32766.5, -32767.5, -32768.5, -32769.5]
    vals = [t / 32768 for t in ties] + [1.0, -1.0, 1.0 - 2.0 ** -16, -(1.0 - 2.0 ** -16), 1.5, -2.0, float("inf"), float("-inf"),
                                        float("nan"), -0.0, 0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126]
    return torch.tensor(vals, dtype=torch.float32)


def float_master(n: int) -> torch.Tensor:
    sp = special_floats()
    u = torch.rand(n - sp.numel(), generator=torch.Generator().manual_seed(7)) * 2.4 - 1.2
    return torch.cat([sp, u])


def pcm_master(n: int) -> torch.Tensor:
    x = torch.randint(-32768, 32768, (n,), generator=torch.Generator().manual_seed(8)).to(torch.int16)
    x[:4] = torch.tensor([-32768, 32767, 0, -1], dtype=torch.int16)
    return x


def words(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Guarded:
    """n elements at `offset` elements behind a 16-byte boundary, sentinels on both sides"""

    def __init__(self, n, dtype, dev, offset=0, fill=None):
        self.base = torch.full((GUARD + offset + n + GUARD,), SENT[dtype], dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.base[self.lo:self.hi]
        if fill is not None:
            self.t.copy_(fill)
        self.before = self.base.clone()
        assert (self.base.data_ptr() + GUARD * self.base.element_size()) % 16 == 0
        assert n == 0 or (self.t.data_ptr() % 16 == 0) == (offset * self.base.element_size() % 16 == 0)

    def guards_intact(self) -> bool:
        return bool(torch.equal(words(self.base[:self.lo]), words(self.before[:self.lo])) and
                    torch.equal(words(self.base[self.hi:]), words(self.before[self.hi:])))

    def untouched(self) -> bool:
        return bool(torch.equal(words(self.base), words(self.before)))


def call(srcs, dsts, n=None, sf=None, df=None, B=None):
    """srcs / dsts: Guarded buffers or raw addresses -> (return code, last error)"""
    from dmel_codec_amd import _lib
    ptr = lambda g: g.t.data_ptr() if isinstance(g, Guarded) else g
    code = lambda g: CODE[g.t.dtype] if isinstance(g, Guarded) else F32
    k = len(srcs)
    n = [g.t.shape[0] for g in srcs] if n is None else n
    sf = [code(g) for g in srcs] if sf is None else sf
    df = [code(g) for g in dsts] if df is None else df
    dev = next(g for g in list(srcs) + list(dsts) if isinstance(g, Guarded)).t.device
    table = torch.empty(4 * max(k, 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().dmel_pcm_convert_items((C.c_void_p * k)(*[ptr(g) for g in srcs]), (C.c_int32 * k)(*sf),
                                               (C.c_void_p * k)(*[ptr(g) for g in dsts]), (C.c_int32 * k)(*df), (C.c_int64 * k)(*n),
                                               k if B is None else B, table.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, _lib.lib().dmel_last_error().decode(errors="replace")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 0), (1, 3)])
def test_f32_to_s16_equals_the_oracle(dev, offsets):
    y = float_master(special_floats().numel() + 5000)
    src, dst = Guarded(y.numel(), torch.float32, dev, offsets[0], fill=y), Guarded(y.numel(), torch.int16, dev, offsets[1])
    rc, msg = call([src], [dst])
    assert rc == 0, msg
    want = oracle_to_s16(y)
    assert want.min() == -32768 and want.max() == 32767
    assert torch.equal(dst.t.cpu(), want) and dst.guards_intact() and src.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 0), (1, 3)])
def test_s16_to_f32_all_values(dev, offsets):
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    src, dst = Guarded(65536, torch.int16, dev, offsets[0], fill=x), Guarded(65536, torch.float32, dev, offsets[1])
    rc, msg = call([src], [dst])
    assert rc == 0, msg
    got = dst.t.cpu()
    assert torch.equal(got, x.float() / 32768) and got[0] == -1.0 and dst.guards_intact() and src.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 0), (1, 3)])
def test_f32_to_f32_is_a_copy_of_the_words(dev, offsets):
    y = float_master(3000)
    nans = torch.tensor([0x7FA00001, 0xFFC12345 - 2 ** 32], dtype=torch.int32)     # a signalling NaN, a negative NaN with a payload
    words(y)[1000:1002] = nans                                                     # any arithmetic on the way would quiet the first
    words(y)[2998:] = nans
    src, dst = Guarded(3000, torch.float32, dev, offsets[0], fill=y), Guarded(3000, torch.float32, dev, offsets[1])
    rc, msg = call([src], [dst])
    assert rc == 0, msg
    finite = torch.isfinite(y)
    assert torch.equal(words(y)[[1000, 1001, 2998, 2999]], nans.repeat(2))         # the input holds them as the words they are
    assert torch.equal(dst.t.cpu()[finite], y[finite]) and torch.equal(words(dst.t.cpu()), words(y))
    assert dst.guards_intact() and src.untouched()


LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 5000]
DIRECTIONS = [(torch.float32, torch.int16), (torch.int16, torch.float32), (torch.float32, torch.float32)]
OFFSETS = [(0, 0), (1, 3), (0, 3), (1, 0)]          # (src, dst) in elements: only (0, 0) takes the 16-byte path


@pytest.mark.gpu
def test_ragged_items_mixed_directions_and_alignments_in_one_launch(dev):
    """every length x direction x alignment as ONE launch of 108 items: outputs equal the oracle, an element has the same bits in
    the aligned and in every unaligned item, sentinels around every destination and every source are unchanged"""
    masters = {torch.float32: float_master(5000), torch.int16: pcm_master(5000)}
    srcs, dsts, key = [], [], []
    for n in LENGTHS:
        for sd, dd in DIRECTIONS:
            for so, do in OFFSETS:
                srcs.append(Guarded(n, sd, dev, so, fill=masters[sd][:n]))
                dsts.append(Guarded(n, dd, dev, do))
                key.append((n, sd, dd, (so, do)))
    assert any(g.t.data_ptr() % 16 for g in dsts) and any(g.t.shape[0] and g.t.data_ptr() % 16 == 0 for g in dsts)
    rc, msg = call(srcs, dsts)
    assert rc == 0, msg
    aligned = {}
    for (n, sd, dd, off), s, d in zip(key, srcs, dsts):
        m = masters[sd][:n]
        want = oracle_to_s16(m) if dd == torch.int16 else (oracle_to_f32(m) if sd == torch.int16 else m)
        got = d.t.cpu()
        assert got.dtype == dd and torch.equal(words(got), words(want)), (n, sd, dd, off)
        assert d.guards_intact() and s.untouched(), (n, sd, dd, off)
        if off == (0, 0):
            aligned[(n, sd, dd)] = got
        else:
            assert torch.equal(words(got), words(aligned[(n, sd, dd)])), (n, sd, dd, off)


@pytest.mark.gpu
def test_idle_launch_writes_nothing(dev):
    dst = [Guarded(100, torch.int16, dev), Guarded(100, torch.float32, dev)]
    src = [Guarded(100, torch.float32, dev, fill=torch.ones(100)), Guarded(100, torch.int16, dev, fill=torch.ones(100, dtype=torch.int16))]
    rc, msg = call(src, dst, n=[0, 0])
    assert rc == 0 and all(d.untouched() for d in dst), msg
    rc, msg = call([0, src[1]], [dst[0], 0], n=[0, 0], sf=[F32, S16], df=[S16, F32])      # an idle item's pointers are not looked at
    assert rc == 0 and all(d.untouched() for d in dst), msg
    rc, msg = call(src, dst, n=[0, 5])                                                    # an idle item next to a live one
    assert rc == 0 and dst[0].untouched() and dst[1].guards_intact() and torch.equal(dst[1].t[:5].cpu(), torch.full((5,), 2.0 ** -15))
    assert bool((dst[1].t[5:] == SENT[torch.float32]).all())


@pytest.mark.gpu
def test_refusals_launch_nothing(dev):
    f = Guarded(64, torch.float32, dev, fill=torch.zeros(64))
    s = Guarded(64, torch.int16, dev, fill=torch.zeros(64, dtype=torch.int16))
    df, ds, ds2 = Guarded(64, torch.float32, dev), Guarded(64, torch.int16, dev), Guarded(64, torch.int16, dev)
    ok = (f, ds)                                                                          # item 0 of every case is a valid item
    cases = {"s16 -> s16": dict(srcs=[f, s], dsts=[ds, ds2]),
             "format 2": dict(srcs=[f, f], dsts=[ds, ds2], df=[S16, 2]),
             "format -1": dict(srcs=[f, f], dsts=[ds, ds2], sf=[F32, -1], df=[S16, S16]),
             "negative n": dict(srcs=[f, f], dsts=[ds, ds2], n=[64, -1]),
             "NULL src": dict(srcs=[f, 0], dsts=[ds, ds2], n=[64, 8], sf=[F32, F32], df=[S16, S16]),
             "NULL dst": dict(srcs=[f, f], dsts=[ds, 0], n=[64, 8], sf=[F32, F32], df=[S16, S16]),
             "odd s16 src": dict(srcs=[f, s.t.data_ptr() + 1], dsts=[ds, df], n=[64, 8], sf=[F32, S16], df=[S16, F32]),
             "odd s16 dst": dict(srcs=[f, f], dsts=[ds, ds2.t.data_ptr() + 1], n=[64, 8], sf=[F32, F32], df=[S16, S16]),
             "f32 src off by 2": dict(srcs=[f, f.t.data_ptr() + 2], dsts=[ds, ds2], n=[64, 8], sf=[F32, F32], df=[S16, S16])}
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc == -1 and "item 1" in msg, (name, rc, msg)
        assert all(d.untouched() for d in (df, ds, ds2)), name
    for B in (0, -1, 65536):
        rc, msg = call([ok[0]], [ok[1]], B=B)
        assert rc == -1 and "65535" in msg and ds.untouched(), (B, rc, msg)
    rc, msg = call([ok[0]], [ok[1]])                                                      # and the valid item alone converts
    assert rc == 0 and torch.equal(ds.t.cpu(), torch.zeros(64, dtype=torch.int16)), msg
