"""The register-blocked forward of the anti-aliased activation (aa_snake.hip): four consecutive outputs per thread, 16-byte LDS accesses,
and 16-byte global accesses when T % 4 == 0 and both tensors start on a 16-byte boundary -- dword accesses otherwise.

  1. forward against float64 at the bound of test_gpu_vocoder_ops_matrix (tau("snake fwd") times the abs-tap scale A_y), at the lengths around
     the kernel's tile and workgroup seams, at every residue of T mod 4 at and above the 6-sample halo, and on a multi-tile row that takes the
     16-byte path next to its two neighbours that do not;
  2. the two global-access paths give the same bits: one set of rows from an aligned tensor, from tensors whose x, y or both start 1, 2 or 3
     floats off a 16-byte boundary, and as the head of rows of odd length (rows 1... then start off the boundary);
  3. shift invariance, as test_activation_forward_is_shift_invariant, at offsets around the new seams.

Helpers, operands, the float64 reference and the bound are those of test_gpu_vocoder_ops_matrix; outputs are NaN-filled between sentinel
guards, so a 16-byte store past a row's end and an element left unwritten both show."""
import pytest
import torch

from test_gpu_conv_matrix import GUARD, SENTINEL, check, lib, stream
from test_gpu_vocoder_ops_matrix import AA_KINDS, LARGE_ALPHA, SHIFT_L, aa_case, aa_forward, aa_id, hold, taps32

TILE = 1008                      # kSnakeFwdTile: outputs per tile
G = 3 * TILE                     # outputs per workgroup (nsub = 3 tiles)

KINDS = AA_KINDS + tuple(LARGE_ALPHA)
T_MULTI = 2 * G + TILE + 100     # 7156 = 4 * 1789: three workgroups, the last with one full tile and a 100-sample one
SHIFT_S = (1, 2, 3, 4, 5, 7, TILE - 5, TILE, TILE + 1, G - 1, G)
SHIFT_T = 4200                   # the full row of the shift test: G + SHIFT_L + 1 and a little more
T_GROUPS = {
    "tile_seam": list(range(TILE - 7, TILE + 8)),
    "group_seam": list(range(G - 7, G + 8)),
    "halo_mod4": list(range(4, 20)),
    "multi_tile": [T_MULTI - 1, T_MULTI, T_MULTI + 1],
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_lengths_cover_both_paths_and_the_seams():
    assert T_MULTI % 4 == 0 and T_MULTI > 2 * G
    for name, ts in T_GROUPS.items():
        assert {t % 4 for t in ts} == ({0, 1, 3} if name == "multi_tile" else {0, 1, 2, 3}), name
    assert SHIFT_T % 4 == 0 and SHIFT_T >= max(SHIFT_S) + SHIFT_L + 1


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(T_GROUPS))
@pytest.mark.parametrize("kind", KINDS)
def test_blocked_forward_against_float64(dev, kind, group):
    for T in T_GROUPS[group]:
        case = aa_case(kind, T)
        y = aa_forward(dev, case["x"], case["alpha"], case["beta"], case["logscale"], aa_id(kind, T))
        hold(y, case["ref"][0], case["A"][0], "snake fwd", aa_id(kind, T))


def forward_at_offsets(dev, x, alpha, beta, logscale, xoff, yoff, what):
    """aa_forward with x starting xoff floats and y starting yoff floats past a 16-byte boundary; guards as In / Out have them."""
    B, Cc, T = x.shape
    n = x.numel()
    xb = torch.full((n + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device=dev)
    xt = xb[GUARD + xoff:GUARD + xoff + n].view(x.shape)
    xt.copy_(x)
    xbits = xb.view(torch.int32).clone()
    yb = torch.empty(n + 2 * GUARD + 4, dtype=torch.float32, device=dev)
    yb.view(torch.int32).fill_(SENTINEL)
    yt = yb[GUARD + yoff:GUARD + yoff + n].view(x.shape)
    yt.fill_(float("nan"))
    assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
    assert xt.data_ptr() % 16 == 4 * xoff and yt.data_ptr() % 16 == 4 * yoff
    ad = alpha.to(dev)
    bd = beta.to(dev) if beta is not None else None
    check(lib().dmel_aa_snake_f32(xt.data_ptr(), yt.data_ptr(), ad.data_ptr(), bd.data_ptr() if bd is not None else None, taps32().data_ptr(),
                                  taps32().data_ptr(), int(logscale), B, Cc, T, stream()), what)
    torch.cuda.synchronize()
    ybits = yb.view(torch.int32)
    bad = int((ybits[:GUARD + yoff] != SENTINEL).sum()) + int((ybits[GUARD + yoff + n:] != SENTINEL).sum())
    assert bad == 0, f"{what}: {bad} guard words around the output were written"
    assert bool(torch.isfinite(yt).all()), f"{what}: output elements left unwritten (NaN) or non-finite"
    assert torch.equal(xb.view(torch.int32), xbits), f"{what}: the input or its NaN guard was written"
    return yt.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["snakebeta_log", "large_lin"])
def test_access_path_never_changes_a_bit(dev, kind):
    case = aa_case(kind, T_MULTI)
    x, args = case["x"], (case["alpha"], case["beta"], case["logscale"])
    y = aa_forward(dev, x, *args, f"{kind} aligned")
    hold(y, case["ref"][0], case["A"][0], "snake fwd", aa_id(kind, T_MULTI))
    bad = []
    for xoff, yoff in [(0, 0)] + [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(o, o) for o in (1, 2, 3)] + [(1, 2), (3, 1)]:
        yo = forward_at_offsets(dev, x, *args, xoff, yoff, f"{kind} x+{xoff} y+{yoff}")
        if not torch.equal(yo, y):
            bad.append(f"x+{xoff} y+{yoff}: {int((yo != y).sum())} elements differ, max |diff| {float((yo - y).abs().max()):.3e}")
    # rows of odd length: rows 1... start off the boundary, dword path.  An output depends on x[t - 6 .. t + 6], so all but the last six
    # outputs of the shortened rows see the same samples as the full rows'
    for To in (T_MULTI - 1, T_MULTI - 3, TILE + 3):
        yo = aa_forward(dev, x[..., :To].contiguous(), *args, f"{kind} rows cut to {To}")
        if not torch.equal(yo[..., :To - 6], y[..., :To - 6]):
            d = yo[..., :To - 6] != y[..., :To - 6]
            bad.append(f"rows cut to {To}: {int(d.sum())} elements differ")
    assert not bad, f"{kind}: the output depends on the global-access path: " + "; ".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["snakebeta_log", *LARGE_ALPHA])
def test_blocked_forward_is_shift_invariant(dev, kind):
    """y(x)[..., s + 6 : s + L - 6] is torch.equal to the run on the window x[..., s : s + L] cropped by 6, wherever the window starts against
    the 1008-sample tiles, the 4-sample register blocks and the 64-lane waves; L = SHIFT_L takes the 16-byte path, L + 1 the dword path."""
    case = aa_case(kind, SHIFT_T)
    y = aa_forward(dev, case["x"], case["alpha"], case["beta"], case["logscale"], f"{kind} full row")
    hold(y, case["ref"][0], case["A"][0], "snake fwd", f"{kind} T{SHIFT_T}")
    bad = []
    for s in SHIFT_S:
        for L in (SHIFT_L, SHIFT_L + 1):
            yw = aa_forward(dev, case["x"][..., s:s + L].contiguous(), case["alpha"], case["beta"], case["logscale"], f"{kind} window {L} at {s}")
            a, b = yw[..., 6:-6], y[..., s + 6:s + L - 6]
            if not torch.equal(a, b):
                bad.append(f"s={s} L={L}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a - b).abs().max()):.3e}")
    assert not bad, f"{kind}: the output depends on where the window starts: " + "; ".join(bad)
