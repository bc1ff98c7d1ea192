"""The G.711 directions of dmel_pcm_convert_items through the C ABI, with guarded buffers.  Every comparison is an equality of bits
against the numpy restatement of the companding rule (tests/g711_ref.py), which tests/test_g711_cpu.py holds to audioop and to values
pinned by hand."""
import ctypes as C

import pytest
import torch

import g711_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements in front of and behind every view: 64 bytes of codes, 128 of int16, 256 of fp32 -- multiples of 16
SENT = {torch.uint8: 0xA5, torch.int16: -12345, torch.float32: -777.0}
F32, S16, ULAW, ALAW = 0, 1, 8, 9
CODE = {"f32": F32, "s16": S16, "ulaw": ULAW, "alaw": ALAW}
DTYPE = {"f32": torch.float32, "s16": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def words(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Guarded:
    """n samples of format `fmt` at `offset` elements behind a 16-byte boundary, sentinels on both sides"""

    def __init__(self, n, fmt, dev, offset=0, fill=None):
        dtype = DTYPE[fmt]
        self.fmt = fmt
        self.base = torch.full((GUARD + offset + n + GUARD,), SENT[dtype], dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.base[self.lo:self.hi]
        if fill is not None:
            self.t.copy_(fill)
        self.before = self.base.clone()
        assert (self.base.data_ptr() + GUARD * self.base.element_size()) % 16 == 0

    def guards_intact(self) -> bool:
        return bool(torch.equal(words(self.base[:self.lo]), words(self.before[:self.lo])) and
                    torch.equal(words(self.base[self.hi:]), words(self.before[self.hi:])))

    def untouched(self) -> bool:
        return bool(torch.equal(words(self.base), words(self.before)))


def call(srcs, dsts, n=None, sf=None, df=None):
    """srcs / dsts: Guarded buffers or raw addresses -> (return code, last error)"""
    from dmel_codec_amd import _lib
    ptr = lambda g: g.t.data_ptr() if isinstance(g, Guarded) else g
    code = lambda g: CODE[g.fmt] if isinstance(g, Guarded) else F32
    k = len(srcs)
    n = [g.t.shape[0] for g in srcs] if n is None else n
    sf = [code(g) for g in srcs] if sf is None else sf
    df = [code(g) for g in dsts] if df is None else df
    dev = next(g for g in list(srcs) + list(dsts) if isinstance(g, Guarded)).t.device
    table = torch.empty(4 * k, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().dmel_pcm_convert_items((C.c_void_p * k)(*[ptr(g) for g in srcs]), (C.c_int32 * k)(*sf),
                                               (C.c_void_p * k)(*[ptr(g) for g in dsts]), (C.c_int32 * k)(*df), (C.c_int64 * k)(*n),
                                               k, table.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, _lib.lib().dmel_last_error().decode(errors="replace")


def special_floats(law: str) -> torch.Tensor:
    """NaN, +-inf, -0.0, denormals, +-1.0, +-2.0, and the s16 ties (k + 0.5) / 32768 on either side of every segment edge"""
    ties = [k + 0.5 for e in ref.segment_edges(law) for k in (e - 2, e - 1, e, e + 1)] + [32766.5, 32767.5, -32767.5, -32768.5]
    vals = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126,
            1.0, -1.0, 2.0, -2.0, 1.0 - 2.0 ** -16] + [t / 32768 for t in ties]
    y = torch.tensor(vals, dtype=torch.float32)
    assert torch.equal((y[15:] * 32768).double(), torch.tensor(ties, dtype=torch.float64))          # every tie is exact in fp32
    return y


def float_master(law: str, n_uniform: int = 5000) -> torch.Tensor:
    u = torch.rand(n_uniform, generator=torch.Generator().manual_seed(7)) * 2.4 - 1.2
    return torch.cat([special_floats(law), u])


def code_master(n: int) -> torch.Tensor:
    x = torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(9)).to(torch.uint8)
    x[:4] = torch.tensor([0x00, 0x7F, 0x80, 0xFF], dtype=torch.uint8)
    return x


@pytest.mark.parametrize("offsets", [(0, 0), (3, 1)])
@pytest.mark.parametrize("law", ref.LAWS)
def test_all_256_codes_decode_to_the_restatement(dev, law, offsets):
    x = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    src, dst = Guarded(256, law, dev, offsets[0], fill=x), Guarded(256, "f32", dev, offsets[1])
    rc, msg = call([src], [dst])
    assert rc == 0, msg
    got = dst.t.cpu()
    assert torch.equal(words(got), words(ref.law_to_f32(x, law))) and dst.guards_intact() and src.untouched()
    for code, value in ref.HAND_DECODE[law]:
        assert got[code] == value / 32768


@pytest.mark.parametrize("offsets", [(0, 0), (1, 3)])
@pytest.mark.parametrize("law", ref.LAWS)
def test_all_65536_values_and_the_special_ones_encode_to_the_restatement(dev, law, offsets):
    grid = torch.arange(-32768, 32768, dtype=torch.float32) / 32768
    y = torch.cat([grid, float_master(law)])
    src, dst = Guarded(y.numel(), "f32", dev, offsets[0], fill=y), Guarded(y.numel(), law, dev, offsets[1])
    rc, msg = call([src], [dst])
    assert rc == 0, msg
    got, want = dst.t.cpu(), ref.f32_to_law(y, law)
    assert got.dtype == torch.uint8 and torch.equal(got, want) and dst.guards_intact() and src.untouched()
    assert len(set(got.tolist())) == (255 if law == "ulaw" else 256)                     # every code but mu-law's negative zero
    for value, code in ref.HAND_ENCODE[law]:
        assert got[value + 32768] == code
    nan_at = 65536 + 0
    assert got[nan_at] == ref.NEUTRAL[law] and got[nan_at + 3] == ref.NEUTRAL[law] and got[nan_at + 4] == ref.NEUTRAL[law]


LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 5000]
LAW_OFFSETS = [(lo, fo) for lo in (0, 1, 3, 8) for fo in (0, 1)]       # law side in bytes, f32 side in elements (0 and 4 bytes)
OLD = [("f32", "s16"), ("s16", "f32"), ("f32", "f32")]
OLD_OFFSETS = [(0, 0), (1, 3)]


def test_ragged_items_of_every_direction_and_alignment_in_one_launch(dev):
    """every length x the four new directions x law offsets 0, 1, 3, 8 bytes x f32 offsets 0, 4 bytes, and the three older directions
    beside them, as ONE launch: outputs equal the restatement, an item has the same bits on the wide path (law offset 0 or 8 with f32
    offset 0) as on the element path, sentinels around every destination and every source are unchanged"""
    from test_gpu_pcm_convert import oracle_to_f32, oracle_to_s16, pcm_master
    masters = {"f32": float_master("ulaw")[:5000], "s16": pcm_master(5000), "ulaw": code_master(5000), "alaw": code_master(5000)}
    srcs, dsts, key = [], [], []
    for n in LENGTHS:
        for law in ref.LAWS:
            for lo, fo in LAW_OFFSETS:
                srcs.append(Guarded(n, law, dev, lo, fill=masters[law][:n]))
                dsts.append(Guarded(n, "f32", dev, fo))
                key.append((n, law, "f32", (lo, fo)))
                srcs.append(Guarded(n, "f32", dev, fo, fill=masters["f32"][:n]))
                dsts.append(Guarded(n, law, dev, lo))
                key.append((n, "f32", law, (lo, fo)))
        for sd, dd in OLD:
            for so, do in OLD_OFFSETS:
                srcs.append(Guarded(n, sd, dev, so, fill=masters[sd][:n]))
                dsts.append(Guarded(n, dd, dev, do))
                key.append((n, sd, dd, (so, do)))
    wide = [g for g, k in zip(dsts, key) if k[0] >= 8 and k[3] in ((0, 0), (8, 0)) and (k[1] in ref.LAWS or k[2] in ref.LAWS)]
    assert wide and all((g.t.data_ptr() % 16 == 0) if g.fmt == "f32" else (g.t.data_ptr() % 8 == 0) for g in wide)
    assert any(g.fmt in ref.LAWS and g.t.data_ptr() % 16 == 8 for g in wide)              # 8-byte aligned only: still the wide path
    rc, msg = call(srcs, dsts)
    assert rc == 0, msg
    aligned = {}
    for (n, sd, dd, off), s, d in zip(key, srcs, dsts):
        m = masters[sd][:n]
        if dd in ref.LAWS:
            want = ref.f32_to_law(m, dd)
        elif sd in ref.LAWS:
            want = ref.law_to_f32(m, sd)
        else:
            want = oracle_to_s16(m) if dd == "s16" else (oracle_to_f32(m) if sd == "s16" else m)
        got = d.t.cpu()
        assert got.dtype == DTYPE[dd] and torch.equal(words(got), words(want)), (n, sd, dd, off)
        assert d.guards_intact() and s.untouched(), (n, sd, dd, off)
        if off == (0, 0):
            aligned[(n, sd, dd)] = got
        else:
            assert torch.equal(words(got), words(aligned[(n, sd, dd)])), (n, sd, dd, off)


def test_idle_launch_writes_nothing(dev):
    dst = [Guarded(100, "ulaw", dev), Guarded(100, "f32", dev)]
    src = [Guarded(100, "f32", dev, fill=torch.ones(100)), Guarded(100, "alaw", dev, fill=torch.full((100,), 0x2A, dtype=torch.uint8))]
    rc, msg = call(src, dst, n=[0, 0])
    assert rc == 0 and all(d.untouched() for d in dst), msg
    rc, msg = call([0, src[1]], [dst[0], 0], n=[0, 0], sf=[F32, ALAW], df=[ULAW, F32])    # an idle item's pointers are not looked at
    assert rc == 0 and all(d.untouched() for d in dst), msg
    rc, msg = call(src, dst, n=[0, 5])                                                    # an idle item next to a live one
    assert rc == 0 and dst[0].untouched() and dst[1].guards_intact(), msg
    assert torch.equal(dst[1].t[:5].cpu(), torch.full((5,), -32256 / 32768)) and bool((dst[1].t[5:] == SENT[torch.float32]).all())


def test_refusals_launch_nothing(dev):
    f = Guarded(64, "f32", dev, fill=torch.zeros(64))
    s = Guarded(64, "s16", dev, fill=torch.zeros(64, dtype=torch.int16))
    u = Guarded(64, "ulaw", dev, fill=torch.full((64,), 0xFF, dtype=torch.uint8))
    df, ds, du, du2 = Guarded(64, "f32", dev), Guarded(64, "s16", dev), Guarded(64, "ulaw", dev), Guarded(64, "alaw", dev)
    # item 0 of every case is a valid law item
    cases = {"ulaw -> alaw": dict(srcs=[f, u], dsts=[du, du2]),
             "ulaw -> ulaw": dict(srcs=[f, u], dsts=[du, du2], df=[ULAW, ULAW]),
             "ulaw -> s16": dict(srcs=[f, u], dsts=[du, ds]),
             "s16 -> alaw": dict(srcs=[f, s], dsts=[du, du2]),
             "code 2": dict(srcs=[f, f], dsts=[du, du2], df=[ULAW, 2]),
             "code 7": dict(srcs=[f, u], dsts=[du, df], sf=[F32, 7]),
             "code 10": dict(srcs=[f, f], dsts=[du, du2], df=[ULAW, 10]),
             "NULL src": dict(srcs=[f, 0], dsts=[du, df], n=[64, 8], sf=[F32, ALAW], df=[ULAW, F32]),
             "NULL dst": dict(srcs=[f, f], dsts=[du, 0], n=[64, 8], sf=[F32, F32], df=[ULAW, ALAW]),
             "f32 dst off by 2": dict(srcs=[f, u], dsts=[du, df.t.data_ptr() + 2], n=[64, 8], sf=[F32, ULAW], df=[ULAW, F32])}
    for name, kw in cases.items():
        rc, msg = call(**kw)
        assert rc == -1 and "item 1" in msg, (name, rc, msg)
        assert all(d.untouched() for d in (df, ds, du, du2)), name
    rc, msg = call([f], [du])                                                             # and the valid item alone converts
    assert rc == 0 and torch.equal(du.t.cpu(), torch.full((64,), 0xFF, dtype=torch.uint8)) and du.guards_intact(), msg
