"""The FSQ kernels alone -- fsq_encode_kernel, fsq_decode_kernel, fsq_bwd_point_kernel, fsq_bwd_param_kernel -- through dmel_fsq_encode_f32 /
dmel_fsq_decode_f32 / dmel_fsq_backward_f32, without the down- and up-sampling stacks the quantiser handle puts around them: against
float64 of the same operands, with the guarded buffers of test_gpu_conv_matrix.py and the per-element bound |y - ref| <= tau * A.  Cases,
references, scales A and tolerances: tests/convnext_fsq_ref.py.

  encode:   prequant within tau * A of float64 (A carries the Linear's bound through the tanh bound(s), fsq_prequant); ids EQUAL to the
            digits packed from rint of the GPU's own prequant (the integer logic, basis, half_width); ids equal to the float64 ids wherever
            the float64 prequant lies farther from an x.5 boundary than that element's own bound -- at most 0.5 % of the (token, level)
            pairs may lie nearer, the count is reported; strict mode: ids equal to the float64 ids everywhere -- to the digits of the float64
            value itself and of that value rounded to fp32 once, which is what the kernel hands to rintf (the two could only part where
            the float64 value lies within half an fp32 ulp of an x.5 boundary; no case has such a value, and both are asserted).
  decode:   codes 0, 1, 2, ... in token order at the encode cases' token counts, plus, for every kind, two cases that each enumerate the whole
            codebook (1000 codes for [8, 5, 5, 5]).
  backward: inputs with a 1e-4 margin to every boundary; dx and the four parameter gradients against the straight-through formulas.
  items:    lengths 0, a middle value, T4, T4 + 5 and -3 (clamped on the device), NaN in z and a code of 2^31 - 1 in ids behind each length:
            ids, prequant and z 0 / 0.f behind, torch.equal to the plain launch in front.
Nothing is masked out of any comparison."""
import ctypes as C

import pytest
import torch

import convnext_fsq_ref as cf
from conftest import report
from test_gpu_conv_matrix import GUARD, SENTINEL, In, Out, check, lib, stream

pytestmark = pytest.mark.gpu

MEASURED = {}
NEAR = {"near": 0, "pairs": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def measured_error_report():
    yield
    for mode in sorted(MEASURED):
        report(f"fsq matrix, {mode}: max |y - ref| / A = {MEASURED[mode]:.3e}  (tau {cf.tau(mode):.2e})")
    if NEAR["pairs"]:
        report(f"fsq matrix, encode: {NEAR['near']} of {NEAR['pairs']} (token, level) pairs lie nearer to a rounding boundary than their own bound "
               f"and are excluded from the id comparison (cap {cf.NEAR_CAP:.1%})")


def hold(y, ref, terms, what):
    (mode, A), = terms
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    r = cf.err_over(y, ref, [(1.0, A)])
    MEASURED[mode] = max(MEASURED.get(mode, 0.0), r)
    print(f"{what}: {mode} max |y - ref| / A = {r:.3e} (tau {cf.tau(mode):.2e})")
    assert r <= cf.tau(mode), f"{what}: max |y - ref| / A = {r:.3e} > tau {cf.tau(mode):.2e} ({mode})"


def untouched(out):
    torch.cuda.synchronize()
    bits = out.base.view(torch.int32)
    return bool(torch.isnan(out.t).all()) and bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + out.n:] == SENTINEL).all())


def as_float(ids):
    """int32 ids in a float32 buffer, bit for bit (In / Out are float32 allocations)"""
    return ids.contiguous().view(torch.float32)


def levels_arg(lv):
    return (C.c_int * len(lv))(*lv)


def encode(dev, case, op, strict, lens=None, prequant=True):
    """dmel_fsq_encode_f32 into guarded outputs: ids (B, G, T4) int32 and prequant (G, B, T4, D), both on the CPU."""
    lv, pb, Cc, G, B, T4 = case
    z, w, b = In(op["z"], dev), In(op["w_in"], dev), In(op["b_in"], dev)
    ids = Out((B, G, T4), dev)
    pre = Out((G, B, T4, len(lv)), dev) if prequant else None
    ld = torch.tensor(lens, dtype=torch.int64, device=dev) if lens is not None else None
    what = f"{cf.fsq_id(case)} encode{' strict' if strict else ''}"
    check(lib().dmel_fsq_encode_f32(z.ptr(), w.ptr(), b.ptr(), levels_arg(lv), len(lv), int(pb), int(strict), ld.data_ptr() if ld is not None else None,
                                    ids.ptr(), pre.ptr() if pre else None, B, G, Cc, T4, stream()), what)
    torch.cuda.synchronize()
    idv = ids.check(what).view(torch.int32).cpu()
    for buf in (z, w, b):
        buf.check(what)
    return idv, pre.check(what).cpu() if pre else None      # with lengths too: prequant is written (as 0.f) behind every length


def decode(dev, case, op, ids, lens=None):
    lv, pb, Cc, G, B, T4 = case
    i, w, b = In(as_float(ids), dev), In(op["w_out"], dev), In(op["b_out"], dev)
    z = Out((B * G, Cc, T4), dev)
    ld = torch.tensor(lens, dtype=torch.int64, device=dev) if lens is not None else None
    what = f"{cf.fsq_id(case)} decode"
    check(lib().dmel_fsq_decode_f32(i.ptr(), w.ptr(), b.ptr(), levels_arg(lv), len(lv), ld.data_ptr() if ld is not None else None, z.ptr(),
                                    B, G, Cc, T4, stream()), what)
    out = z.check(what).cpu()
    for buf in (i, w, b):
        buf.check(what)
    return out


@pytest.mark.parametrize("case", cf.FSQ_CASES, ids=cf.fsq_id)
def test_encode(dev, case):
    lv, pb, Cc, G, B, T4 = case
    op = cf.fsq_operands(case)
    pre64, A = cf.fsq_prequant(op, case)
    d64 = cf.fsq_digits(pre64, lv)
    ids, pre = encode(dev, case, op, strict=False)
    hold(pre, pre64, [("fsq prequant", A)], cf.fsq_id(case))
    assert torch.equal(ids, cf.fsq_pack(cf.fsq_digits(pre, lv), lv, B, G)), "ids are not the digits packed from rint of the kernel's own prequant"
    safe = cf.fsq_safe(pre64, A)
    NEAR["near"] += int((~safe).sum())
    NEAR["pairs"] += safe.numel()
    digits = cf.fsq_unpack(ids, lv)
    assert not bool(((digits != d64) & safe).any()), f"{int(((digits != d64) & safe).sum())} digits differ from float64 away from every rounding boundary"
    assert int((~safe).sum()) <= cf.NEAR_CAP * safe.numel(), (int((~safe).sum()), safe.numel())
    ids_nopre, _ = encode(dev, case, op, strict=False, prequant=False)
    assert torch.equal(ids_nopre, ids)
    # strict: the Linear and the bounds in float64, rounded to fp32 once -- the ids are the float64 ids everywhere
    ids_s, pre_s = encode(dev, case, op, strict=True)
    assert torch.equal(ids_s, cf.fsq_pack(d64, lv, B, G)), int((cf.fsq_unpack(ids_s, lv) != d64).sum())
    assert torch.equal(ids_s, cf.fsq_pack(cf.fsq_digits(pre64.float(), lv), lv, B, G))
    assert torch.equal(ids_s, cf.fsq_pack(cf.fsq_digits(pre_s, lv), lv, B, G))
    hold(pre_s, pre64, [("fsq prequant", A)], cf.fsq_id(case) + " strict")


@pytest.mark.parametrize("case", cf.FSQ_DECODE_CASES, ids=cf.fsq_id)
def test_decode(dev, case):
    op = cf.fsq_operands(case)
    ids = cf.fsq_decode_ids(case)
    ref, A = cf.fsq_decode_ref(op, case, ids)
    hold(decode(dev, case, op, ids), ref, [("fsq decode", A)], cf.fsq_id(case))


def backward(dev, case, op, scratch_floats=None):
    lv, pb, Cc, G, B, T4 = case
    D = len(lv)
    x, dout, w_in, b_in, w_out = (In(op[k], dev) for k in ("z", "dout", "w_in", "b_in", "w_out"))
    outs = dict(dx=Out((B * G, Cc, T4), dev), dw_in=Out((G, D, Cc), dev), db_in=Out((G, D), dev), dw_out=Out((G, Cc, D), dev), db_out=Out((G, Cc), dev))
    need = 2 * B * G * T4 * D
    scratch = Out((need if scratch_floats is None else max(1, scratch_floats),), dev)
    rc = lib().dmel_fsq_backward_f32(x.ptr(), dout.ptr(), w_in.ptr(), b_in.ptr(), w_out.ptr(), levels_arg(lv), D, int(pb), outs["dx"].ptr(),
                                     outs["dw_in"].ptr(), outs["db_in"].ptr(), outs["dw_out"].ptr(), outs["db_out"].ptr(), scratch.ptr(),
                                     need if scratch_floats is None else scratch_floats, B, G, Cc, T4, stream())
    return rc, outs, scratch, (x, dout, w_in, b_in, w_out)


@pytest.mark.parametrize("case", cf.FSQ_BWD_CASES, ids=cf.fsq_id)
def test_backward(dev, case):
    """fsq_bwd_point_kernel and fsq_bwd_param_kernel: 1, 63, 255, 256, 257 and 700 points per (channel, group) workgroup -- the n += 256 loop
    runs once, twice and three times -- as one item and as several."""
    op = cf.fsq_bwd_operands(case)
    what = cf.fsq_id(case) + " backward"
    rc, outs, scratch, ins = backward(dev, case, op)
    check(rc, what)
    refs = cf.fsq_backward_refs(op, case)
    for name, o in outs.items():
        hold(o.check(f"{what} {name}").cpu(), *refs[name], f"{what} {name}")
    scratch.check(what)              # both halves of the scratch are written in full, nothing beyond it
    for buf in ins:
        buf.check(what)


@pytest.mark.parametrize("case", cf.FSQ_ITEM_CASES, ids=cf.fsq_id)
def test_items(dev, case):
    lv, pb, Cc, G, B, T4 = case
    lens = cf.FSQ_ITEM_LENS(T4)
    assert len(lens) == B
    lim = [min(max(l, 0), T4) for l in lens]
    op = cf.fsq_operands(case)
    plain_ids, plain_pre = encode(dev, case, op, strict=False)
    zn = op["z"].clone().view(B, G, Cc, T4)
    for b, l in enumerate(lim):
        zn[b, :, :, l:] = float("nan")
    for strict in (False, True):
        ref_ids, ref_pre = (plain_ids, plain_pre) if not strict else encode(dev, case, op, strict=True)
        ids, pre = encode(dev, case, dict(op, z=zn.view(B * G, Cc, T4)), strict=strict, lens=lens)
        for b, l in enumerate(lim):
            assert torch.equal(ids[b, :, :l], ref_ids[b, :, :l]) and not bool(ids[b, :, l:].any()), (b, l, strict)
            assert torch.equal(pre[:, b, :l], ref_pre[:, b, :l]) and not bool(pre[:, b, l:].any()), (b, l, strict)      # prequant: (G, B, T4, D)
    codes = cf.fsq_decode_ids(case)
    plain = decode(dev, case, op, codes).view(B, G, Cc, T4)
    poisoned = codes.clone()
    for b, l in enumerate(lim):
        poisoned[b, :, l:] = 2 ** 31 - 1
    z = decode(dev, case, op, poisoned, lens=lens).view(B, G, Cc, T4)
    for b, l in enumerate(lim):
        assert torch.equal(z[b, :, :, :l], plain[b, :, :, :l]) and not bool(z[b, :, :, l:].any()), (b, l)


def test_entry_points_refuse_bad_arguments_and_write_nothing(dev):
    case = ((7, 5, 5), True, 70, 3, 2, 9)
    lv, pb, Cc, G, B, T4 = case
    op = cf.fsq_operands(case)
    z, w, b, wo, bo = (In(op[k], dev) for k in ("z", "w_in", "b_in", "w_out", "b_out"))
    ids, pre, zo = Out((B, G, T4), dev), Out((G, B, T4, 3), dev), Out((B * G, Cc, T4), dev)
    L = lib()

    def enc(levels, n, B_=B, zp=z.ptr()):
        return L.dmel_fsq_encode_f32(zp, w.ptr(), b.ptr(), levels_arg(levels), n, 1, 0, None, ids.ptr(), pre.ptr(), B_, G, Cc, T4, stream())

    for rc in (enc(lv, 5), enc(lv, 0), enc((7, 1, 5), 3), enc(lv, 3, B_=0), enc(lv, 3, zp=None), enc((1024, 1024, 1024, 2), 4)):
        assert rc == -1, (rc, L.dmel_last_error())
    assert untouched(ids) and untouched(pre)
    for rc in (L.dmel_fsq_decode_f32(ids.ptr(), wo.ptr(), bo.ptr(), levels_arg(lv), 5, None, zo.ptr(), B, G, Cc, T4, stream()),
               L.dmel_fsq_decode_f32(ids.ptr(), wo.ptr(), bo.ptr(), levels_arg(lv), 3, None, zo.ptr(), B, G, Cc, 0, stream()),
               L.dmel_fsq_decode_f32(None, wo.ptr(), bo.ptr(), levels_arg(lv), 3, None, zo.ptr(), B, G, Cc, T4, stream())):
        assert rc == -1, (rc, L.dmel_last_error())
    assert untouched(zo)
    rc, outs, scratch, ins = backward(dev, case, op, scratch_floats=2 * B * G * T4 * 3 - 1)
    assert rc == -1 and "scratch" in L.dmel_last_error().decode(), (rc, L.dmel_last_error())
    assert all(untouched(o) for o in outs.values()) and untouched(scratch)
    for buf in (z, w, b, wo, bo, *ins):
        buf.check("refused fsq call")
