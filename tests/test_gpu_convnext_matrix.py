"""The standalone ConvNeXt block handle (dmel_convnext_*), every stage held to a float64 evaluation of the tensors the GPU actually fed it.

The handle keeps every intermediate in the workspace the caller owns (inference: h1, h2; training: H0, H1, U, G, V, DV, DG, DH1, DH0 --
convnext_fsq_ref.cx_infer_layout / cx_train_layout mirror csrc/modules.hip and are asserted against the library's byte counts for every
case), so dwconv_ln_kernel, the two 1x1 convolutions with the GELU and row_scale + residual epilogues, gelu_fwd / gelu_bwd,
layerscale_res_fwd / layerscale_bwd, ln_bwd and dwconv_bwd are each compared with float64 of their own operands: the rounding of earlier
stages does not enter a bound.  Guarded buffers (In / Out of test_gpu_conv_matrix.py) for x, dy, y, dx, the gradient buffer and the
workspace; per-element bound |y - ref| <= tau * A with the references, the scales A and the tolerances of tests/convnext_fsq_ref.py.
Nothing is masked out of any comparison."""
import ctypes as C

import pytest
import torch

import convnext_fsq_ref as cf
from conftest import report
from test_gpu_conv_matrix import GUARD, SENTINEL, In, Out, check, lib, stream

pytestmark = pytest.mark.gpu

MEASURED = {}                    # mode -> largest max |y - ref| / A seen by this module
COMBINED = "dU: conv dx x |gelu'| + gelu bwd (fraction of the bound)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def measured_error_report():
    yield
    for mode in sorted(MEASURED):
        bound = "1" if mode == COMBINED else f"{cf.tau(mode):.2e}"
        report(f"convnext matrix, {mode}: max |y - ref| / A = {MEASURED[mode]:.3e}  (tau {bound})")


def hold(y, ref, terms, what):
    """|y - ref| <= sum tau(mode) * A over the stage's terms, every element; with one term the measured max |y - ref| / A is recorded."""
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite"
    if len(terms) == 1:
        mode, A = terms[0]
        r = cf.err_over(y, ref, [(1.0, A)])
        MEASURED[mode] = max(MEASURED.get(mode, 0.0), r)
        print(f"{what}: {mode} max |y - ref| / A = {r:.3e} (tau {cf.tau(mode):.2e})")
        assert r <= cf.tau(mode), f"{what}: max |y - ref| / A = {r:.3e} > tau {cf.tau(mode):.2e} ({mode})"
    else:
        r = cf.err_over(y, ref, [(cf.tau(m), A) for m, A in terms])
        MEASURED[COMBINED] = max(MEASURED.get(COMBINED, 0.0), r)
        print(f"{what}: {' + '.join(m for m, _ in terms)}: max |y - ref| / bound = {r:.3e}")
        assert r <= 1.0, f"{what}: max |y - ref| / (sum tau A) = {r:.3e} > 1 ({[m for m, _ in terms]})"


def hold_abs(y, ref, bound, what):
    assert tuple(y.shape) == tuple(ref.shape) and bool(torch.isfinite(y).all()), what
    r = float(((y.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |y - ref| / bound = {r:.3e}")
    assert r <= 1.0, f"{what}: max |y - ref| / bound = {r:.3e} > 1"


class Block:
    """A dmel_convnext handle over the case's nine tensors, destroyed by close()."""

    def __init__(self, p, train, expect=0):
        from dmel_codec_amd import _lib
        self.C = p["gamma"].numel()
        self.h = C.c_void_p()
        check(lib().dmel_convnext_create(C.byref(self.h), self.C), "convnext_create")
        try:
            if train:
                check(lib().dmel_convnext_enable_training(self.h, 1), "convnext_enable_training")
            _lib.set_tensors(lib().dmel_convnext_set_tensor, self.h, p, "convnext")
            self.rc = lib().dmel_convnext_finalize(self.h)
            self.error = lib().dmel_last_error().decode(errors="replace")
            assert (self.rc == 0) == (expect == 0), (self.rc, self.error)
        except BaseException:
            self.close()
            raise

    def slot(self, key):
        off, num = C.c_int64(), C.c_int64()
        check(lib().dmel_convnext_grad_slot(self.h, key.encode(), C.byref(off), C.byref(num)), "convnext_grad_slot")
        return off.value, num.value

    def close(self):
        lib().dmel_convnext_destroy(self.h)


def guards_intact(out, what):
    torch.cuda.synchronize()
    bits = out.base.view(torch.int32)
    bad = int((bits[:GUARD] != SENTINEL).sum()) + int((bits[GUARD + out.n:] != SENTINEL).sum())
    assert bad == 0, f"{what}: {bad} guard words around the buffer were written"


def untouched(out):
    """A refused call left its guarded buffer as it was: all NaN, guards intact."""
    torch.cuda.synchronize()
    bits = out.base.view(torch.int32)
    return bool(torch.isnan(out.t).all()) and bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + out.n:] == SENTINEL).all())


def views(ws, layout, shapes):
    """The named regions of a guarded workspace as CPU tensors."""
    return {name: ws.t[off:off + n].view(shapes[name]).cpu() for name, (off, n) in layout.items()}


def train_case(dev, shape, light=False):
    """forward_train, backward into a NaN-filled gradient buffer, backward again into the same buffer: every stage within its bound."""
    Cc, N, T = shape
    c = cf.cx_case(shape)
    p, n = c["p"], N * Cc * T
    layout, total = cf.cx_train_layout(n)
    b = Block(p, train=True)
    try:
        assert lib().dmel_convnext_train_workspace_bytes(b.h, N, T) == total, "cx_plan_at changed: update cx_train_layout"
        x, dy = In(c["x"], dev), In(c["dy"], dev)
        y, dx, ws = Out((N, Cc, T), dev), Out((N, Cc, T), dev), Out((total // 4,), dev)
        grads = Out((lib().dmel_convnext_grad_floats(b.h),), dev)
        assert grads.n == sum(v.numel() for v in p.values())
        what = cf.cx_id(shape)
        check(lib().dmel_convnext_forward_train(b.h, x.ptr(), y.ptr(), N, T, ws.ptr(), total, stream()), what)
        yv = y.check(what).cpu()
        guards_intact(ws, what)
        small, big = (N, Cc, T), (N, 4 * Cc, T)
        shapes = dict(H0=small, H1=small, U=big, G=big, V=small, DV=small, DG=big, DH1=small, DH0=small)
        fwd_names = ("H0", "H1", "U", "G", "V")
        wf = views(ws, {k: layout[k] for k in fwd_names}, shapes)
        refs = cf.cx_forward_refs(p, c["x"], wf)
        for name in fwd_names:
            hold(wf[name], *refs[name], f"{what} {name}")
        hold(yv, *refs["y"], f"{what} y")
        for call in (1, 2):      # the second call finds the first one's gradients in the buffer: nothing may accumulate
            whatb = f"{what} backward {call}"
            dx.poison()
            check(lib().dmel_convnext_backward(b.h, x.ptr(), dy.ptr(), dx.ptr(), grads.ptr(), N, T, ws.ptr(), total, stream()), whatb)
            dxv = dx.check(whatb).cpu()
            gv = grads.check(whatb).cpu()      # filled with NaN before the first call: every slot was written and is finite
            guards_intact(ws, whatb)
            w = views(ws, layout, shapes)
            for name in fwd_names:
                assert torch.equal(w[name], wf[name]), f"{whatb} changed the saved {name}"
            refs = cf.cx_backward_refs(p, c["x"], c["dy"], w, only=() if light else None)
            for name, key in (("DV", "DV"), ("dU", "DG"), ("DH1", "DH1"), ("DH0", "DH0")):
                hold(w[key], *refs[name], f"{whatb} {name}")
            hold(dxv, *refs["dx"], f"{whatb} dx")
            for name, key in cf.CX_GRAD_OF.items():
                if name in refs:
                    off, num = b.slot(key)
                    hold(gv[off:off + num].view(p[key].shape), *refs[name], f"{whatb} {name}")
        x.check(what)
        dy.check(what)
    finally:
        b.close()


@pytest.mark.parametrize("shape", cf.CX_CASES, ids=cf.cx_id)
def test_training_path_stage_by_stage(dev, shape):
    """T edges (below the seven taps; 31 / 32 / 33, 63 / 64 / 65, 97 against the 32-column tiles) at C = 7 and 70; C edges (1, no multiple of
    8, the ln_bwd LDS limit 246); the flattened (item, frame) loops of layerscale_bwd and dwconv_bwd at 1, 15, 255, 256, 257 and 679 points."""
    train_case(dev, shape)


def test_training_path_above_the_grid_cap(dev):
    """C = 16, N = 3, T = 43700: 2,097,600 elements, just over the 8192 x 256 cap of the elementwise launchers -- gelu_fwd / gelu_bwd
    (4n elements) wrap four times, layerscale_res_fwd once.  The weight and bias gradients of the two 1x1 convolutions are left to the conv
    matrix here (the float64 outer products over 131,100 columns are the slow part); every other stage is checked, on both backward calls."""
    train_case(dev, cf.CX_LONG, light=True)


def infer_case(dev, shape, names=("h1", "h2", "y")):
    Cc, N, T = shape
    c = cf.cx_case(shape)
    layout, total = cf.cx_infer_layout(N * Cc * T)
    b = Block(c["p"], train=False)
    try:
        assert lib().dmel_convnext_workspace_bytes(b.h, N, T) == total, "run_convnext's workspace changed: update cx_infer_layout"
        x = In(c["x"], dev)
        y, ws = Out((N, Cc, T), dev), Out((total // 4,), dev)
        what = cf.cx_id(shape) + " inference"
        check(lib().dmel_convnext_forward(b.h, x.ptr(), y.ptr(), N, T, ws.ptr(), total, stream()), what)
        yv = y.check(what).cpu()
        guards_intact(ws, what)
        x.check(what)
        w = views(ws, layout, dict(h1=(N, Cc, T), h2=(N, 4 * Cc, T)))
        refs = cf.cx_infer_refs(c["p"], c["x"], w)
        w["y"] = yv
        for name in names:
            hold_abs(w[name], *refs[name], f"{what} {name}")
    finally:
        b.close()


@pytest.mark.parametrize("shape", cf.CX_CASES, ids=cf.cx_id)
def test_inference_path_stage_by_stage(dev, shape):
    """dwconv_ln_kernel without the saved pre-norm tensor, and the GELU and row_scale + residual epilogues of the convolution kernel, which
    only this path uses: h1 from x, h2 from the GPU's h1, y from the GPU's h2."""
    infer_case(dev, shape)


def test_inference_at_the_lds_limit(dev):
    """C = 494 is the most dwconv_ln_kernel's [C][33] tile allows: it runs and h1 holds its bound.  C = 495 is refused with a non-zero code,
    y and the workspace untouched."""
    infer_case(dev, (494, 1, 33), names=("h1",))
    Cc, N, T = 495, 1, 33
    b = Block(cf.cx_params(Cc, 495), train=False)
    try:
        total = lib().dmel_convnext_workspace_bytes(b.h, N, T)
        assert total == cf.cx_infer_layout(N * Cc * T)[1]
        x = In(torch.randn(N, Cc, T, generator=torch.Generator().manual_seed(495)), dev)
        y, ws = Out((N, Cc, T), dev), Out((total // 4,), dev)
        rc = lib().dmel_convnext_forward(b.h, x.ptr(), y.ptr(), N, T, ws.ptr(), total, stream())
        assert rc != 0 and "LDS" in lib().dmel_last_error().decode(), (rc, lib().dmel_last_error())
        assert untouched(y) and untouched(ws), "a refused forward wrote its output or its workspace"
        x.check("refused forward")
    finally:
        b.close()


def test_training_handle_above_246_channels_is_refused_before_any_launch(dev):
    """ln_bwd keeps two [C][33] tiles in the LDS: C <= 246.  A training handle of 247 channels used to run forward_train and then fail inside
    backward with three gradients already written; it is refused at finalize, the message names the LDS limit, forward_train and backward
    return an error and y, dx, the gradient buffer and the workspace stay untouched.  An inference handle of 247 channels still runs."""
    Cc, N, T = 247, 1, 33
    p = cf.cx_params(Cc, 247)
    b = Block(p, train=True, expect=-2)
    try:
        assert b.rc == -2 and "LDS" in b.error and "246" in b.error, (b.rc, b.error)
        total = cf.cx_train_layout(N * Cc * T)[1]
        g = torch.Generator().manual_seed(247)
        x, dy = In(torch.randn(N, Cc, T, generator=g), dev), In(torch.randn(N, Cc, T, generator=g), dev)
        y, dx, ws = Out((N, Cc, T), dev), Out((N, Cc, T), dev), Out((total // 4,), dev)
        grads = Out((sum(v.numel() for v in p.values()),), dev)
        assert lib().dmel_convnext_grad_floats(b.h) == 0
        assert lib().dmel_convnext_forward_train(b.h, x.ptr(), y.ptr(), N, T, ws.ptr(), total, stream()) != 0
        assert lib().dmel_convnext_backward(b.h, x.ptr(), dy.ptr(), dx.ptr(), grads.ptr(), N, T, ws.ptr(), total, stream()) != 0
        assert lib().dmel_convnext_forward(b.h, x.ptr(), y.ptr(), N, T, ws.ptr(), total, stream()) != 0      # a failed finalize leaves no handle to run
        for buf, name in ((y, "y"), (dx, "dx"), (grads, "grads"), (ws, "workspace")):
            assert untouched(buf), f"a refused training call wrote {name}"
        x.check("refused training")
        dy.check("refused training")
    finally:
        b.close()
    infer_case(dev, (247, 1, 33), names=("h1", "y"))


def test_items_form_at_the_tile_edges(dev):
    """dmel_convnext_forward_items at C = 9, T = 70 with lengths 0, 1, 3, 31, 32, 33, 70 and NaN behind every length in x: each row
    (y, h1 and h2) torch.equal to the plain launch on the cropped item, exactly zero behind its length."""
    Cc, T, lens = cf.CX_ITEMS
    N = len(lens)
    p = cf.cx_params(Cc, 970)
    xc = torch.randn(N, Cc, T, generator=torch.Generator().manual_seed(971))
    for n, l in enumerate(lens):
        xc[n, :, l:] = float("nan")
    layout, total = cf.cx_infer_layout(N * Cc * T)
    b = Block(p, train=False)
    try:
        x = In(xc, dev)
        y, ws = Out((N, Cc, T), dev), Out((total // 4,), dev)
        ld = torch.tensor(lens, dtype=torch.int64, device=dev)
        check(lib().dmel_convnext_forward_items(b.h, x.ptr(), ld.data_ptr(), y.ptr(), N, T, ws.ptr(), total, stream()), "forward_items")
        yv = y.check("forward_items").cpu()
        guards_intact(ws, "forward_items")
        x.check("forward_items")
        w = views(ws, layout, dict(h1=(N, Cc, T), h2=(N, 4 * Cc, T)))
        for n, l in enumerate(lens):
            for t in (yv, w["h1"], w["h2"]):
                assert not bool(t[n, :, l:].any()) and not bool(torch.isnan(t[n]).any()), (n, l)
            if l == 0:
                continue
            xi = In(xc[n:n + 1, :, :l].contiguous(), dev)
            tot1 = cf.cx_infer_layout(Cc * l)[1]
            yi, wsi = Out((1, Cc, l), dev), Out((tot1 // 4,), dev)
            check(lib().dmel_convnext_forward(b.h, xi.ptr(), yi.ptr(), 1, l, wsi.ptr(), tot1, stream()), f"plain launch on item {n}")
            assert torch.equal(yi.check(f"item {n}").cpu()[0], yv[n, :, :l]), (n, l)
            assert torch.equal(wsi.t[:Cc * l].view(Cc, l).cpu(), w["h1"][n, :, :l]), (n, l)
            assert torch.equal(wsi.t[Cc * l:5 * Cc * l].view(4 * Cc, l).cpu(), w["h2"][n, :, :l]), (n, l)
    finally:
        b.close()
