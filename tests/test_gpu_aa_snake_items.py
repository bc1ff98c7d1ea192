"""The anti-aliased activation over items of different lengths (dmel_aa_snake_items_f32, aa_snake.hip): rows of one pitch T, item b a row of
len[b] <= T columns with its own replicate padding.

  * columns [0, len[b]) of every (b, c) row are the bits of dmel_aa_snake_f32 on that item alone with T = len[b];
  * nothing at or beyond column len[b] is read (x holds NaN there) or written (y keeps its canary there);
  * the lengths sit on both sides of the 1008-output tile and of the three-tile workgroup and have every residue mod 4, so both global
    access paths are taken inside ONE launch; an odd pitch, and tensors that start off a 16-byte boundary, put every row on the dword path.

Operands are those of test_gpu_vocoder_ops_matrix (the plain kernel is held to float64 there and in test_gpu_aa_snake_blocked)."""
import pytest
import torch

from test_gpu_conv_matrix import check, lib, stream
from test_gpu_vocoder_ops_matrix import AA_C, aa_operands, taps32

TILE = 1008
C, B, PITCH = 3, 9, 3028
LENS = [0, 1, 2, 5, 1007, 1008, 1009, 3024, 3025]
CANARY = -777.0
KINDS = ("snakebeta_log", "snakebeta_lin", "snake_log")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_lengths_cover_the_seams_and_every_residue():
    assert C == AA_C and len(LENS) == B and max(LENS) <= PITCH
    assert {TILE - 1, TILE, TILE + 1, 3 * TILE, 3 * TILE + 1} <= set(LENS) and 0 in LENS
    assert {n % 4 for n in LENS} == {0, 1, 2, 3}
    assert PITCH % 4 == 0 and (PITCH + 1) % 2 == 1


def plain(dev, x, alpha, beta, logscale):
    """dmel_aa_snake_f32 on one item alone"""
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib().dmel_aa_snake_f32(x.data_ptr(), y.data_ptr(), alpha.data_ptr(), beta.data_ptr() if beta is not None else None,
                                  taps32().data_ptr(), taps32().data_ptr(), int(logscale), x.shape[0], x.shape[1], x.shape[2], stream()), "aa_snake")
    return y


@pytest.fixture(scope="module")
def cases(dev):
    """per kind: operands on the device and the plain kernel's output per item -- computed once, shared by every pitch / offset"""
    out = {}
    for kind in KINDS:
        x, _, alpha, beta, logscale, _ = aa_operands(kind, max(LENS), B=B)
        xd, ad = x.to(dev), alpha.to(dev)
        bd = beta.to(dev) if beta is not None else None
        want = [plain(dev, xd[b:b + 1, :, :n], ad, bd, logscale) if n else None for b, n in enumerate(LENS)]
        torch.cuda.synchronize()
        out[kind] = (xd, ad, bd, logscale, want)
    return out


def run_items(dev, case, pitch, off):
    """x and y as (B, C, pitch) views that start `off` floats behind a 16-byte boundary; x NaN and y canary outside the items"""
    xd, ad, bd, logscale, want = case
    n = B * C * pitch
    xb = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=dev)
    yb = torch.full((n + 8,), CANARY, dtype=torch.float32, device=dev)
    xt, yt = xb[off:off + n].view(B, C, pitch), yb[off:off + n].view(B, C, pitch)
    assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
    for b, m in enumerate(LENS):
        xt[b, :, :m] = xd[b, :, :m]
    lens = torch.tensor(LENS, dtype=torch.int64, device=dev)
    check(lib().dmel_aa_snake_items_f32(xt.data_ptr(), yt.data_ptr(), ad.data_ptr(), bd.data_ptr() if bd is not None else None,
                                        taps32().data_ptr(), taps32().data_ptr(), int(logscale), B, C, pitch, lens.data_ptr(), stream()),
          "aa_snake_items")
    torch.cuda.synchronize()
    bad = []
    for b, m in enumerate(LENS):
        if m and not torch.equal(yt[b, :, :m], want[b][0]):
            d = yt[b, :, :m] != want[b][0]
            bad.append(f"item {b} (len {m}): {int(d.sum())} of {d.numel()} elements differ from the item alone")
        if not bool((yt[b, :, m:] == CANARY).all()):
            bad.append(f"item {b} (len {m}): {int((yt[b, :, m:] != CANARY).sum())} columns at or beyond its length were written")
    if not bool((yb[:off] == CANARY).all() and (yb[off + n:] == CANARY).all()):
        bad.append("the output was written outside the tensor")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pitch,off", [(PITCH, 0), (PITCH + 1, 0), (PITCH, 1), (PITCH, 2), (PITCH + 2, 3)],
                         ids=["aligned", "odd_pitch", "off1", "off2", "pitch_mod4_2_off3"])
def test_items_have_the_bits_of_each_item_alone(dev, cases, kind, pitch, off):
    bad = run_items(dev, cases[kind], pitch, off)
    assert not bad, f"{kind} pitch {pitch} offset {off}: " + "; ".join(bad)


@pytest.mark.gpu
def test_lengths_beyond_the_pitch_are_clamped_and_bad_arguments_refused(dev, cases):
    """the table is clamped into [0, pitch] on the device: a length past the pitch cannot make the kernel leave the tensor"""
    xd, ad, bd, logscale, _ = cases["snakebeta_log"]
    T = 1010
    x = xd[:2, :, :T].contiguous()
    yb = torch.full((2 * C * T + 4096,), CANARY, dtype=torch.float32, device=dev)
    y = yb[:2 * C * T].view(2, C, T)
    lens = torch.tensor([T + 5000, -3], dtype=torch.int64, device=dev)
    check(lib().dmel_aa_snake_items_f32(x.data_ptr(), y.data_ptr(), ad.data_ptr(), bd.data_ptr(), taps32().data_ptr(), taps32().data_ptr(),
                                        int(logscale), 2, C, T, lens.data_ptr(), stream()), "aa_snake_items")
    torch.cuda.synchronize()
    assert torch.equal(y[0], plain(dev, x[:1], ad, bd, logscale)[0])
    assert bool((y[1] == CANARY).all()) and bool((yb[2 * C * T:] == CANARY).all())
    rc = lib().dmel_aa_snake_items_f32(x.data_ptr(), y.data_ptr(), ad.data_ptr(), bd.data_ptr(), taps32().data_ptr(), taps32().data_ptr(),
                                       int(logscale), 2, C, T, None, stream())
    assert rc != 0
