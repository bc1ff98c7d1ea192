"""The backward of the STFT magnitude (csrc/stft_bwd.hip) against float64 autograd, element by element, at the edges of its four steps:
one frame shorter than n_fft, tail samples that lie in no frame (their gradient is exactly 0.f), hop = n_fft (no padding, no overlap),
T around the 256-frame block of the spectrum step, L around the 256-sample blocks of the reflect-pad and overlap-add steps, hop = 2.

dmel_stft_magnitude_backward_f32 is called directly: audio rows of stride L + 3 with NaN slack, gradient rows of stride L + 4 whose
slack must come back untouched, the workspace sized by dmel_stft_grad_workspace_bytes.  The cotangent is d/d mag of
sum w mag + sum log(mag + 0.3) at the float64 magnitudes (tests/stft_truth.py: backward_inputs), the reference float64 autograd through
frames64 / mag64, and the bar holds per element:

    |dy - dy64| <= max(3 e_ref, floor) eps scale[b, j]

scale is the same gradient with the absolute value of every term taken, so a sample that few frames touch is held as tightly as one
that many touch; e_ref is fp32 autograd through the oracle's torch.stft in the same units; the floor (stft_truth.floor_bwd) is derived
from the split products and the accumulation chain of the GEMM the kernel runs, and is zero wherever scale is: there the kernel owes an
exact zero.  The oracle is an FFT and has no such chain, so the floor, not 3 e_ref, is the bar in most cases; each case reports
e_gpu / e_ref.  Every case is also held to the older max-norm bar of test_stft_magnitude_backward_matches_autograd,
max |dy - dy64| <= max(2e-5, 3 e_ref) max |dy64|, so that the per-element bar is nowhere the looser of the two.

Measured on the MI355X: e_gpu 0.8 .. 10.1 beside e_ref 0.5 .. 2.0.  The kernel is NOT within 3 e_ref everywhere: e_gpu / e_ref is above 3 in
six cases (1024-short-T1 4.7, 1024-tail-quarter-hop 3.4, 2048-tail 5.3 -- 10.06 against 1.91 --, 2048-hop-is-n_fft 4.0, 1024-B3 3.6,
1024-full-window 3.1) and grows with n_fft, as a dense DFT's accumulation does against an FFT's; all of them sit below a tenth of the
floor and below 5.4e-6 in max-norm."""
import pytest
import torch

import stft_truth as st
from conftest import report

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
BY_ID = {c.id: c for c in st.BACKWARD}
_worst = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    if _worst:
        worst, near = max(_worst), max(_worst, key=lambda r: r[0] / r[2])
        report(f"[stft bwd matrix] {len(_worst)} cases; worst e_gpu {worst[0]:.2f} (e_ref {worst[1]:.2f}, bar {worst[2]:.2f}) in {worst[3]}; "
               f"closest to its bar: {near[3]}, e_gpu {near[0]:.2f} = {near[0] / near[2]:.2f} of the bar {near[2]:.2f} (e_ref {near[1]:.2f})")


def backward(dev, c, x, g):
    """one dmel_stft_magnitude_backward_f32 call -> dy (B, L)"""
    import ctypes as C
    from dmel_codec_amd import _lib
    from dmel_codec_amd.torch_ops import _stft_grad_handle
    B, L = x.shape
    w32 = st.backward_window(c)
    audio = torch.full((B, L + 3), float("nan"), device=dev)
    audio[:, :L] = x.to(dev)
    dy = torch.full((B, L + 4), SENTINEL, device=dev)
    gd = g.to(dev).contiguous()
    lib = _lib.lib()
    with torch.cuda.device(dev):
        if w32 is None:
            h = _stft_grad_handle(dev, c.n_fft, c.win, c.hop)
        else:                                                      # a handle of its own for a window of its own
            hv = C.c_void_p()
            _lib.check(lib.dmel_stft_grad_create(C.byref(hv), c.n_fft, c.win, c.hop, w32.contiguous().data_ptr()), "stft_grad_create")
            h = hv.value
        try:
            nbytes = lib.dmel_stft_grad_workspace_bytes(h, B, L)
            assert nbytes > 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.dmel_stft_magnitude_backward_f32(h, audio.data_ptr(), L + 3, gd.data_ptr(), dy.data_ptr(), L + 4, B, L, ws.data_ptr(),
                                                            nbytes, _lib.stream_ptr()), "stft_magnitude_backward")
            torch.cuda.synchronize()
        finally:
            if w32 is not None:
                lib.dmel_stft_grad_destroy(h)
    assert bool((dy[:, L:] == SENTINEL).all()), "the slack behind a gradient row was written"
    return dy[:, :L].cpu()


@pytest.mark.parametrize("cid", [c.id for c in st.BACKWARD])
def test_backward(dev, cid):
    c = BY_ID[cid]
    x, g = st.backward_inputs(c)
    assert g.shape == (c.B, c.L // c.hop, c.n_fft // 2 + 1)
    dy64, scale = st.backward64(c, x, g)
    dy32 = st.backward32(c, x, g)
    dy = backward(dev, c, x, g)
    assert bool(torch.isfinite(dy).all()), "a NaN slack word was read"
    cut = st.first_untouched(c)
    live = scale > 0                     # not live: behind the last frame, or under a zero of the window where frames do not overlap
    assert not bool(live[:, cut:].any()) and (cut < c.L) == cid.endswith("-tail")
    assert bool((dy[:, cut:] == 0).all()), "a sample that no frame reads has a gradient"
    assert bool((dy[~live] == 0).all()) and bool((dy64[~live] == 0).all())
    unit = st.EPS * scale[live]
    e_gpu = float(((dy.double() - dy64)[live].abs() / unit).max())
    e_ref = float(((dy32.double() - dy64)[live].abs() / unit).max())
    bar = max(3.0 * e_ref, st.floor_bwd(c))
    top = float(dy64.abs().max())
    m_gpu, m_ref = float((dy.double() - dy64).abs().max()) / top, float((dy32.double() - dy64).abs().max()) / top
    report(f"[stft bwd matrix] {cid}: e_gpu {e_gpu:.2f} e_ref {e_ref:.2f} (ratio {e_gpu / max(e_ref, 1e-30):.1f}, floor {st.floor_bwd(c):.0f}), in eps * scale "
           f"per element; max-norm gpu {m_gpu:.1e} ref {m_ref:.1e}")
    _worst.append((e_gpu, e_ref, bar, cid))
    assert e_gpu <= bar, (cid, e_gpu, e_ref)
    assert m_gpu <= max(st.MAXNORM_BWD, 3.0 * m_ref), (cid, m_gpu, m_ref)
