"""CPU checks of what tests/test_gpu_convnext_matrix.py and tests/test_gpu_fsq_matrix.py rest on (tests/convnext_fsq_ref.py): the recorded
reference ratios, the near-boundary cap of the fp32 reference's ids, the workspace layouts the ConvNeXt matrix mirrors, and the float64
references against autograd through the oracle."""
import ctypes as C
import math
import os
import re

import torch

import convnext_fsq_ref as cf
from conftest import ROOT
from oracle import ref_cpu


def test_reference_ratios_do_not_exceed_the_recorded_ones():
    """The fp32 CPU reference (torch in float32) against float64 of the same operands, in units of A, over every case of the two GPU modules:
    none above the recorded R_mode the kernel bounds are multiples of (nor below half of it: a stale constant), every bound at or below its
    ceiling.  Measured: H0 2.205e-7, LN fwd 2.294e-7, gelu fwd 3.506e-7, gelu bwd 6.166e-7, layerscale 1.114e-7, dgamma 1.104e-7,
    ln dx 1.575e-7, ln dparams 1.098e-7, dw dx 2.146e-7, dw dparams 1.185e-7, fsq prequant 8.718e-8, fsq decode 1.682e-7, fsq dx 2.857e-7,
    fsq dparams 1.753e-7.  (The largest gelu ratios come from the 8.4 million samples of the long case.)"""
    got, _ = cf.reference_ratios()
    for mode, r in got.items():
        print(f"R[{mode!r}] measured {r:.3e}, recorded {cf.R[mode]:.2e}, tau {cf.tau(mode):.2e}")
    for mode, r in got.items():
        assert 0.5 * cf.R[mode] <= r <= cf.R[mode], (mode, r, cf.R[mode])
        assert cf.tau(mode) <= cf.CEIL[mode]


def test_fp32_reference_ids_stay_within_the_near_boundary_cap():
    """On the encode inputs of the FSQ matrix, the fp32 CPU reference's digits equal the float64 ones wherever the float64 pre-quantised value
    lies farther from an x.5 boundary than that element's own bound, and at most 0.5 % of the (token, level) pairs lie nearer."""
    near = wrong = pairs = 0
    for case in cf.FSQ_CASES + cf.FSQ_ITEM_CASES:
        op = cf.fsq_operands(case)
        pre, A = cf.fsq_prequant(op, case)
        safe = cf.fsq_safe(pre, A)
        d32, d64 = cf.fsq_digits(cf.fsq_prequant32(op, case), case[0]), cf.fsq_digits(pre, case[0])
        assert not bool(((d32 != d64) & safe).any()), cf.fsq_id(case)
        # strict mode rounds the float64 value to fp32 once before rintf: on these inputs that never moves a value across (or onto) a boundary
        assert torch.equal(cf.fsq_digits(pre.float(), case[0]), d64), cf.fsq_id(case)
        assert int((~safe).sum()) <= cf.NEAR_CAP * safe.numel(), (cf.fsq_id(case), int((~safe).sum()), safe.numel())
        near += int((~safe).sum())
        wrong += int(((d32 != d64) & ~safe).sum())
        pairs += safe.numel()
        # the digits cover the codebook: the packed id round-trips
        lv, _, C, G, B, T4 = case
        assert torch.equal(cf.fsq_unpack(cf.fsq_pack(d64, lv, B, G), lv), d64)
    print(f"{near} of {pairs} (token, level) pairs nearer to a boundary than their bound; {wrong} of them round the other way in fp32")
    assert near <= cf.NEAR_CAP * pairs


def test_every_backward_case_finds_its_margin():
    for case in cf.FSQ_BWD_CASES:
        cf.fsq_bwd_operands(case)
    points = {B * T4 for (_, _, _, _, B, T4) in cf.FSQ_BWD_CASES}
    assert points == {1, 63, 255, 256, 257, 700}
    assert {(G * B * T4) for (_, _, _, G, B, T4) in cf.FSQ_CASES if G == 1} == {1, 255, 256, 257, 600}
    assert {(G * B * T4) for (_, _, _, G, B, T4) in cf.FSQ_CASES if G == 3} == {3, 255, 258, 600}
    for count in {G * B * T4 for (_, _, _, G, B, T4) in cf.FSQ_CASES}:
        assert {C for (_, _, C, G, B, T4) in cf.FSQ_CASES if G * B * T4 == count} == {1, 70}
    # decode: for every kind, each of its two full cases (G = 3 with C = 70, G = 1 with C = 1) enumerates every code of the codebook, so every
    # digit of every level is decoded; the other decode cases are the encode cases
    assert cf.FSQ_DECODE_CASES[:len(cf.FSQ_CASES)] == cf.FSQ_CASES
    for lv, pb in cf.FSQ_KINDS:
        full = [c for c in cf.FSQ_DECODE_FULL if c[:2] == (lv, pb)]
        assert {(c[2], c[3]) for c in full} == {(70, 3), (1, 1)}
        for c in full:
            ids = cf.fsq_decode_ids(c)
            assert sorted(set(ids.view(-1).tolist())) == list(range(math.prod(lv))), cf.fsq_id(c)
            digits = cf.fsq_unpack(ids, lv)
            for j, L in enumerate(lv):
                assert set(digits[..., j].reshape(-1).tolist()) == set(range(L)), (cf.fsq_id(c), j)


def test_layouts_mirror_the_source():
    """The Python mirror of the two workspace layouts against the lines of csrc/modules.hip it transcribes."""
    src = open(os.path.join(ROOT, "dmel_codec_amd", "csrc", "modules.hip")).read()
    for line in ("p.H0 = a.take<float>(n); p.H1 = a.take<float>(n); p.U = a.take<float>(4 * n); p.G = a.take<float>(4 * n); p.V = a.take<float>(n);",
                 "p.DV = a.take<float>(n); p.DG = a.take<float>(4 * n); p.DH1 = a.take<float>(n); p.DH0 = a.take<float>(n);",
                 "return run_convnext(m->cx, x, y, h1, h1 + (size_t)N * m->C * T, N, m->C, T, (hipStream_t)stream);",
                 "return align_up((size_t)5 * N * m->C * T * sizeof(float), 256);"):
        assert line in src, f"modules.hip no longer contains `{line}`: update cx_train_layout / cx_infer_layout"
    assert re.search(r"size_t o = align_up\(off, 256\);", open(os.path.join(ROOT, "dmel_codec_amd", "csrc", "common.h")).read())
    lay, total = cf.cx_train_layout(7)
    assert [lay[k][0] * 4 for k in ("H0", "H1", "U", "G", "V")] == [0, 256, 512, 768, 1024] and total == 256 * 9
    assert cf.cx_infer_layout(7) == ({"h1": (0, 7), "h2": (7, 28)}, 256)


def test_stage_references_compose_to_the_oracle():
    """The float64 stage references, chained, are the oracle's block and its autograd gradients: a wrong formula here would hold the kernels
    to the wrong value."""
    for shape in ((7, 2, 6), (9, 3, 33)):
        c = cf.cx_case(shape)
        p64 = {k: v.double().requires_grad_() for k, v in c["p"].items()}
        x64 = c["x"].double().requires_grad_()
        y64 = ref_cpu.convnext_block(p64, "", x64)
        (y64 * c["dy"].double()).sum().backward()
        # feed every stage the (float64) output of the one before: the chain itself
        x, dy, p = c["x"].double(), c["dy"].double(), {k: v.double() for k, v in c["p"].items()}
        C, N, T = shape
        ws = {k: torch.zeros(N, C * (4 if k in ("U", "G", "DG") else 1), T, dtype=torch.float64)
              for k in ("H0", "H1", "U", "G", "V", "DV", "DG", "DH1", "DH0")}
        for name in ("H0", "H1", "U", "G", "V"):
            ws[name] = cf.cx_forward_refs(p, x, ws)[name][0]
        fwd = cf.cx_forward_refs(p, x, ws)
        assert torch.allclose(fwd["y"][0], y64.detach(), rtol=0, atol=1e-12)
        for name, key in (("DV", "DV"), ("dU", "DG"), ("DH1", "DH1"), ("DH0", "DH0")):
            ws[key] = cf.cx_backward_refs(p, x, dy, ws)[name][0]
        bwd = cf.cx_backward_refs(p, x, dy, ws)
        assert torch.allclose(bwd["dx"][0], x64.grad, rtol=0, atol=1e-11)
        for name, key in cf.CX_GRAD_OF.items():
            assert torch.allclose(bwd[name][0], p64[key].grad.view(bwd[name][0].shape), rtol=0, atol=1e-10), name
    # FSQ: the explicit straight-through formulas against autograd in float64
    for case in (cf.FSQ_BWD_CASES[1], cf.FSQ_BWD_CASES[12], cf.FSQ_BWD_CASES[75]):
        op = cf.fsq_bwd_operands(case)
        refs = cf.fsq_backward_refs(op, case)
        auto = cf.fsq_backward32({k: v.double() for k, v in op.items()}, case)
        for name, (ref, _) in refs.items():
            assert torch.allclose(ref, auto[name].double(), rtol=0, atol=2e-6 * float(ref.abs().max().clamp_min(1))), (cf.fsq_id(case), name)


def test_bounds_see_what_the_global_bar_hides():
    """An error of 1e-5 of the tensor's largest value, planted into the element whose scale A is smallest, passes the module tests' bar
    (rel_err = max |a - b| / max |b| < 2e-5) and violates the per-element bound -- for the maps, the per-channel sums and the FSQ input
    gradient.  (The FSQ parameter gradients are left out: 1 - tanh^2 cancels where the bound saturates, their honest scale A is far above
    the sums themselves, and an error of that size in the smallest of them is within fp32 reach.)"""
    from conftest import rel_err
    c = cf.cx_case((70, 2, 33))
    ws, out = cf.cx_chain32(c["p"], c["x"], c["dy"])
    refs = dict(cf.cx_forward_refs(c["p"], c["x"], ws))
    refs.update(cf.cx_backward_refs(c["p"], c["x"], c["dy"], ws, dgpre=ws["DGpre"], only=()))
    case = next(s for s in cf.FSQ_BWD_CASES if s[4] * s[5] == 257 and s[2] == 70)
    op = cf.fsq_bwd_operands(case)
    fsq = cf.fsq_backward_refs(op, case)
    out.update({"fsq " + k: v for k, v in cf.fsq_backward32(op, case).items()})
    refs.update({"fsq " + k: v for k, v in fsq.items()})
    for name in ("H0", "H1", "G", "y", "dgamma", "DH0", "dln_w", "dln_b", "dx", "ddw", "fsq dx"):
        ref, ((mode, A),) = refs[name]
        y = out[name].contiguous().clone().view(ref.shape)
        assert cf.err_over(y, ref, [(1.0, A)]) <= cf.tau(mode), name                    # unplanted: within the bound
        y.view(-1)[int(A.reshape(-1).argmin())] += 1e-5 * float(ref.abs().max())
        assert rel_err(y, ref) < 2e-5 and cf.err_over(y, ref, [(1.0, A)]) > cf.tau(mode), name


def test_training_handles_above_the_ln_bwd_lds_limit_are_refused_at_finalize():
    """ln_bwd keeps two [C][33] fp32 tiles in the 64 KiB LDS (C <= 246); the forward's single tile would take 494.  A TRAINING ConvNeXt handle of
    247 channels and a TRAINING quantiser of 247 channels per group are refused by finalize with DMEL_EUNSUPPORTED before anything is read,
    packed or launched, and the message names the limit; 246 and the inference handles pass that check (they then miss their tensors)."""
    from dmel_codec_amd import _lib
    L = _lib.lib()
    UNSUPPORTED, MISSING = -2, -3
    for dim, train, want in ((247, 1, UNSUPPORTED), (246, 1, MISSING), (247, 0, MISSING), (494, 0, MISSING)):
        h = C.c_void_p()
        assert L.dmel_convnext_create(C.byref(h), dim) == 0
        assert L.dmel_convnext_enable_training(h, train) == 0
        rc, msg = L.dmel_convnext_finalize(h), L.dmel_last_error().decode()
        L.dmel_convnext_destroy(h)
        assert rc == want, (dim, train, rc, msg)
        assert ("LDS" in msg and "246" in msg and "convnext_finalize" in msg) == (want == UNSUPPORTED), msg
    lv, fs = (C.c_int * 3)(7, 5, 5), (C.c_int * 2)(2, 2)
    for cg, groups, train, want in ((247, 1, 1, UNSUPPORTED), (247, 3, 1, UNSUPPORTED), (246, 3, 1, MISSING), (247, 3, 0, MISSING)):
        q = C.c_void_p()
        assert L.dmel_quantizer_create(C.byref(q), cg * groups, groups, lv, 3, fs, 2, 1) == 0
        assert L.dmel_quantizer_enable_training(q, train) == 0
        rc, msg = L.dmel_quantizer_finalize(q), L.dmel_last_error().decode()
        assert L.dmel_quantizer_grad_floats(q) == 0
        L.dmel_quantizer_destroy(q)
        assert rc == want, (cg, groups, train, rc, msg)
        assert ("LDS" in msg and "246" in msg and "quantizer_finalize" in msg) == (want == UNSUPPORTED), msg
