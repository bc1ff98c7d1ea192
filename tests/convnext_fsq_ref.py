"""Cases, float64 references with their scales A, fp32 CPU references and the recorded tolerances of tests/test_gpu_convnext_matrix.py and
tests/test_gpu_fsq_matrix.py (GPU) and tests/test_convnext_fsq_refs_cpu.py (CPU).  No GPU is needed to import or run anything here.

Every kernel is compared with a float64 evaluation of ITS OWN operands (the tensors the GPU fed it, read back from the caller-owned
workspace), element by element: |y - ref| <= tau * A, where A is the same formula with every operand replaced by its absolute value and no
cancellation.  A is written next to each reference below.

Tolerances (the method of test_gpu_vocoder_ops_matrix.py): tau_mode = min(FACTOR * R_mode, ceiling).  R_mode is the largest
max |y32 - ref64| / A of the fp32 CPU reference (torch in float32) over the cases of the two GPU modules, recorded in R below rounded up by
5-10 % and recomputed by test_reference_ratios_do_not_exceed_the_recorded_ones.  FACTOR = 8: the kernels sum in another order than torch and
use the device erff / tanhf / expf.  Ceilings: 2^-19 for elementwise results, 2^-16 for reductions.  The two 1x1 convolutions, their
backward-data and their weight / bias gradients use the conv matrix's TAU, unchanged.  No bound is taken from a kernel under test."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_conv_matrix import TAU

EPS = 1e-6
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
GELU_SLOPE = 1.13                # max |gelu'| = 1.1290 (at u = sqrt(2))

# ------------------------------------------------------------------------------------ tolerances
R = {
    "H0": 2.4e-7,
    "LN fwd": 2.5e-7,
    "gelu fwd": 3.8e-7,
    "gelu bwd": 6.6e-7,
    "layerscale": 1.2e-7,
    "dgamma": 1.2e-7,
    "ln dx": 1.7e-7,
    "ln dparams": 1.2e-7,
    "dw dx": 2.3e-7,
    "dw dparams": 1.28e-7,
    "fsq prequant": 9.4e-8,
    "fsq decode": 1.8e-7,
    "fsq dx": 3.1e-7,
    "fsq dparams": 1.9e-7,
}
FACTOR = 8
ELEMENTWISE, REDUCTION = 2.0 ** -19, 2.0 ** -16
CEIL = {
    "H0": ELEMENTWISE, "LN fwd": ELEMENTWISE, "gelu fwd": ELEMENTWISE, "gelu bwd": ELEMENTWISE, "layerscale": ELEMENTWISE,
    "dgamma": REDUCTION, "ln dx": ELEMENTWISE, "ln dparams": REDUCTION, "dw dx": ELEMENTWISE, "dw dparams": REDUCTION,
    "fsq prequant": ELEMENTWISE, "fsq decode": ELEMENTWISE, "fsq dx": ELEMENTWISE, "fsq dparams": REDUCTION,
}
CONV_FWD, CONV_DX, CONV_DW, CONV_DB = "fwd NP=3", "dx NP=3", "dw", "db"      # a handle's default precision is FP32: the six-product split


def tau(mode):
    return TAU[mode] if mode in TAU else min(FACTOR * R[mode], CEIL[mode])


def err_over(y, ref, terms):
    """max over all elements of |y - ref| / sum_i k_i * A_i (float64), terms = [(k, A), ...].  With one term (1, A) this is max |y - ref| / A."""
    err = (y.detach().double().cpu() - ref).abs()
    den = sum(k * A for k, A in terms)
    return float((err / den.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ==================================================================================== ConvNeXt block
CX_KEYS = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias",
           "gamma")
CX_T_EDGES = [1, 2, 3, 4, 6, 7, 8, 31, 32, 33, 63, 64, 65, 97]
# (C, N, T)
CX_CASES = ([(C, 2, T) for C in (7, 70) for T in CX_T_EDGES]                        # T edges: below the 7 taps, around one, two, three 32-column tiles
            + [(C, 1, 33) for C in (1, 7, 8, 9, 70, 246)]                           # C edges: no multiple of 8, the LDS limit of ln_bwd
            + [(9, 1, 1), (9, 3, 5), (9, 5, 51), (9, 4, 64), (9, 1, 257), (9, 7, 97)])   # flattened (N, T): 1, 15, 255, 256, 257, 679 points
CX_CASES = list(dict.fromkeys(CX_CASES))
CX_LONG = (16, 3, 43700)         # 2,097,600 elements: above the 8192 x 256 grid cap of the elementwise launchers
CX_ITEMS = (9, 70, (0, 1, 3, 31, 32, 33, 70))     # C, T, lengths


def cx_id(s):
    return f"C{s[0]}-N{s[1]}-T{s[2]}"


def cx_params(C, seed):
    """The nine tensors of a block, O(1) so that every term matters: gamma ~ N(0, 0.5), norm.weight ~ N(1, 0.3)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {
        "dwconv.weight": rn(C, 1, 7) / math.sqrt(7), "dwconv.bias": rn(C) * 0.1,
        "norm.weight": 1 + rn(C) * 0.3, "norm.bias": rn(C) * 0.3,
        "pwconv1.weight": rn(4 * C, C) / math.sqrt(C), "pwconv1.bias": rn(4 * C) * 0.1,
        "pwconv2.weight": rn(C, 4 * C) / math.sqrt(4 * C), "pwconv2.bias": rn(C) * 0.1,
        "gamma": rn(C) * 0.5,
    }


@functools.lru_cache(maxsize=None)
def cx_case(shape):
    C, N, T = shape
    seed = C * 7919 + N * 104729 + T
    g = torch.Generator().manual_seed(seed + 1)
    return dict(p=cx_params(C, seed), x=torch.randn(N, C, T, generator=g), dy=torch.randn(N, C, T, generator=g))


def cx_train_layout(n):
    """cx_plan_at (csrc/modules.hip): H0, H1, U, G, V, DV, DG, DH1, DH0 of n, n, 4n, 4n, n, n, 4n, n, n floats, each on a 256-byte boundary;
    after backward DG holds dU.  -> ({name: (float offset, floats)}, total bytes)"""
    off, out = 0, {}
    for name, k in (("H0", 1), ("H1", 1), ("U", 4), ("G", 4), ("V", 1), ("DV", 1), ("DG", 4), ("DH1", 1), ("DH0", 1)):
        off = (off + 255) // 256 * 256
        out[name] = (off // 4, k * n)
        off += 4 * k * n
    return out, (off + 255) // 256 * 256


def cx_infer_layout(n):
    """run_convnext (csrc/modules.hip): h1 of n floats at offset 0, h2 of 4n floats directly behind it."""
    return {"h1": (0, n), "h2": (n, 4 * n)}, (5 * n * 4 + 255) // 256 * 256


def erf_(v):
    return torch.special.erf(v)


def gelu_prime(u):
    return 0.5 * (1 + erf_(u * SQRT1_2)) + u * INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def gelu_prime_abs(u):
    """|Phi| + |u| phi with Phi = (1 + |erf|) / 2: no cancellation"""
    return 0.5 * (1 + erf_(u * SQRT1_2).abs()) + u.abs() * INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def dwconv(x, w, b):
    return F.conv1d(x, w, b, padding=3, groups=x.shape[1])


def ln_stats(h):
    mean = h.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((h - mean) ** 2).mean(1, keepdim=True) + EPS)
    return mean, rstd


def pw(h, w, b=None):
    return F.conv1d(h, w[:, :, None], b)


def col(v):
    return v.view(1, -1, 1)


def cx_forward_refs(p, x, ws):
    """float64 references of the training forward, each from the fp32 tensors `ws` the stage was fed: name -> (ref, [(mode, A)])."""
    d = {k: v.double() for k, v in p.items()}
    x = x.double()
    out = {}
    # H0 = dwconv7(x) + b                                         A = sum |w| |x| + |b|
    out["H0"] = (dwconv(x, d["dwconv.weight"], d["dwconv.bias"]),
                 [("H0", dwconv(x.abs(), d["dwconv.weight"].abs(), d["dwconv.bias"].abs()))])
    # H1 = (h - mean_c h) rstd ln_w + ln_b, biased variance       A = |ln_w| rstd (|h| + mean_c |h|) + |ln_b|
    h = ws["H0"].double()
    mean, rstd = ln_stats(h)
    out["H1"] = ((h - mean) * rstd * col(d["norm.weight"]) + col(d["norm.bias"]),
                 [("LN fwd", col(d["norm.weight"]).abs() * rstd * (h.abs() + h.abs().mean(1, keepdim=True)) + col(d["norm.bias"]).abs())])
    # U = W1 H1 + b1, V = W2 G + b2                               the conv matrix's A = sum |w| |x| + |b| and its TAU
    for name, src, wk, bk in (("U", "H1", "pwconv1.weight", "pwconv1.bias"), ("V", "G", "pwconv2.weight", "pwconv2.bias")):
        s = ws[src].double()
        out[name] = (pw(s, d[wk], d[bk]), [(CONV_FWD, pw(s.abs(), d[wk].abs(), d[bk].abs()))])
    # G = u (1 + erf(u / sqrt 2)) / 2                             A = |u| (1 + |erf|) / 2
    u = ws["U"].double()
    e = erf_(u * SQRT1_2)
    out["G"] = (0.5 * u * (1 + e), [("gelu fwd", 0.5 * u.abs() * (1 + e.abs()))])
    # y = x + gamma V                                             A = |x| + |gamma| |V|
    v = ws["V"].double()
    out["y"] = (x + col(d["gamma"]) * v, [("layerscale", x.abs() + col(d["gamma"]).abs() * v.abs())])
    return out


def ln_propagated(p, x, tau_h0):
    """The inference path's h1 = LN(dwconv(x)) comes out of ONE kernel, its pre-norm tensor is never stored: the bound is the LN bound on the
    float64 h plus the depthwise conv's own bound e = tau_H0 * A_H0 carried through the LayerNorm's derivative
    d h1_c = ln_w_c rstd (d_c - mean(d) - xhat_c mean(xhat d)):   |ln_w| rstd (e + mean_c e + |xhat| mean_c(|xhat| e)).  -> (ref, bound)"""
    d = {k: v.double() for k, v in p.items()}
    x = x.double()
    h = dwconv(x, d["dwconv.weight"], d["dwconv.bias"])
    e = tau_h0 * dwconv(x.abs(), d["dwconv.weight"].abs(), d["dwconv.bias"].abs())
    mean, rstd = ln_stats(h)
    xhat = (h - mean) * rstd
    lw = col(d["norm.weight"]).abs()
    A_ln = lw * rstd * (h.abs() + h.abs().mean(1, keepdim=True)) + col(d["norm.bias"]).abs()
    carried = lw * rstd * (e + e.mean(1, keepdim=True) + xhat.abs() * (xhat.abs() * e).mean(1, keepdim=True))
    return xhat * col(d["norm.weight"]) + col(d["norm.bias"]), tau("LN fwd") * A_ln + carried


def cx_infer_refs(p, x, ws):
    """The inference path: name -> (ref, bound) with the bound already in absolute units.
    h2 = gelu(W1 h1 + b1) from the GPU's h1: the conv bound carried through |gelu'| <= 1.13, plus the GELU bound at |u| + the conv bound;
    y = x + gamma (W2 h2 + b2) from the GPU's h2: the conv TAU on A = |x| + |gamma| (sum |W2| |h2| + |b2|)."""
    d = {k: v.double() for k, v in p.items()}
    out = {"h1": ln_propagated(p, x, tau("H0"))}
    h1 = ws["h1"].double()
    u = pw(h1, d["pwconv1.weight"], d["pwconv1.bias"])
    eu = tau(CONV_FWD) * pw(h1.abs(), d["pwconv1.weight"].abs(), d["pwconv1.bias"].abs())
    e = erf_(u * SQRT1_2)
    out["h2"] = (0.5 * u * (1 + e), GELU_SLOPE * eu + tau("gelu fwd") * 0.5 * (u.abs() + eu) * (1 + e.abs()))
    h2 = ws["h2"].double()
    out["y"] = (x.double() + col(d["gamma"]) * pw(h2, d["pwconv2.weight"], d["pwconv2.bias"]),
                tau(CONV_FWD) * (x.double().abs() + col(d["gamma"]).abs() * pw(h2.abs(), d["pwconv2.weight"].abs(), d["pwconv2.bias"].abs())))
    return out


def cx_backward_refs(p, x, dy, ws, dgpre=None, only=None):
    """float64 references of the backward, each from the fp32 tensors `ws` the stage was fed: name -> (ref, [(mode, A), ...]); the bound of a
    stage is sum tau(mode) * A.  dgpre: the tensor W2^T DV the GELU backward was fed, where it exists (the fp32 CPU chain); the GPU overwrites
    it in place, so there dU is held to the conv bound times |gelu'| plus the GELU-backward bound.  only: names to compute (None: all)."""
    d = {k: v.double() for k, v in p.items()}
    x, dy = x.double(), dy.double()
    want = lambda name: only is None or name in only
    out = {}
    g = col(d["gamma"])
    # DV = dy gamma                                               A = |dy| |gamma|
    out["DV"] = (dy * g, [("layerscale", dy.abs() * g.abs())])
    # dgamma = sum_{n,t} dy V                                     A = sum |dy| |V|
    v = ws["V"].double()
    out["dgamma"] = ((dy * v).sum((0, 2)), [("dgamma", (dy.abs() * v.abs()).sum((0, 2)))])
    dv, gg, u, h1 = ws["DV"].double(), ws["G"].double(), ws["U"].double(), ws["H1"].double()
    du = ws["DG"].double()
    # dW2 = sum DV (x) G, db2 = sum DV; dW1 = sum dU (x) H1, db1 = sum dU       A = the sums of absolute products; the conv matrix's TAU
    if want("dW2"):
        out["dW2"] = (torch.einsum("nct,nkt->ck", dv, gg), [(CONV_DW, torch.einsum("nct,nkt->ck", dv.abs(), gg.abs()))])
        out["db2"] = (dv.sum((0, 2)), [(CONV_DB, dv.abs().sum((0, 2)))])
    if want("dW1"):
        out["dW1"] = (torch.einsum("nkt,nct->kc", du, h1), [(CONV_DW, torch.einsum("nkt,nct->kc", du.abs(), h1.abs()))])
        out["db1"] = (du.sum((0, 2)), [(CONV_DB, du.abs().sum((0, 2)))])
    # dU = (W2^T DV) gelu'(U), gelu' = Phi(u) + u phi(u)          A_conv = |W2|^T |DV|;  A_gelu = |dG| (|Phi| + |u| phi)
    gp, gpa = gelu_prime(u), gelu_prime_abs(u)
    w2t = d["pwconv2.weight"].t().contiguous()
    if dgpre is not None:
        dg = dgpre.double()
        out["dU"] = (dg * gp, [("gelu bwd", dg.abs() * gpa)])
    else:
        dg, A_conv = pw(dv, w2t), pw(dv.abs(), w2t.abs())
        out["dU"] = (dg * gp, [(CONV_DX, A_conv * gp.abs()), ("gelu bwd", (dg.abs() + tau(CONV_DX) * A_conv) * gpa)])
    # DH1 = W1^T dU                                               A = |W1|^T |dU|
    w1t = d["pwconv1.weight"].t().contiguous()
    out["DH1"] = (pw(du, w1t), [(CONV_DX, pw(du.abs(), w1t.abs()))])
    # DH0 = rstd (dxh - mean_c dxh - xhat mean_c(dxh xhat)), dxh = DH1 ln_w, xhat = (h - mean) rstd
    #   A = rstd (|dxh| + mean_c |dxh| + X mean_c(|dxh| X)),  X = rstd (|h| + mean_c |h|)
    h, dh1 = ws["H0"].double(), ws["DH1"].double()
    mean, rstd = ln_stats(h)
    xhat = (h - mean) * rstd
    X = rstd * (h.abs() + h.abs().mean(1, keepdim=True))
    dxh = dh1 * col(d["norm.weight"])
    out["DH0"] = (rstd * (dxh - dxh.mean(1, keepdim=True) - xhat * (dxh * xhat).mean(1, keepdim=True)),
                  [("ln dx", rstd * (dxh.abs() + dxh.abs().mean(1, keepdim=True) + X * (dxh.abs() * X).mean(1, keepdim=True)))])
    # dln_w = sum DH1 xhat, dln_b = sum DH1                       A = sum |DH1| X, sum |DH1|
    out["dln_w"] = ((dh1 * xhat).sum((0, 2)), [("ln dparams", (dh1.abs() * X).sum((0, 2)))])
    out["dln_b"] = (dh1.sum((0, 2)), [("ln dparams", dh1.abs().sum((0, 2)))])
    # dx = dy + dwconv^T(DH0)                                     A = |dy| + |w|^T |DH0|
    dh0 = ws["DH0"].double()
    w = d["dwconv.weight"]
    C = x.shape[1]
    out["dx"] = (dy + F.conv_transpose1d(dh0, w, padding=3, groups=C), [("dw dx", dy.abs() + F.conv_transpose1d(dh0.abs(), w.abs(), padding=3, groups=C))])
    # ddw[c, k] = sum_{n,t} DH0[n, c, t] x[n, c, t + k - 3], ddb = sum DH0        A = the sums of absolute products
    T = x.shape[2]
    xp = F.pad(x, (3, 3))
    ddw = torch.stack([(dh0 * xp[..., k:k + T]).sum((0, 2)) for k in range(7)], 1)
    Addw = torch.stack([(dh0.abs() * xp[..., k:k + T].abs()).sum((0, 2)) for k in range(7)], 1)
    out["ddw"] = (ddw.view(C, 1, 7), [("dw dparams", Addw.view(C, 1, 7))])
    out["ddb"] = (dh0.sum((0, 2)), [("dw dparams", dh0.abs().sum((0, 2)))])
    return out


CX_GRAD_OF = {"ddw": "dwconv.weight", "ddb": "dwconv.bias", "dln_w": "norm.weight", "dln_b": "norm.bias", "dW1": "pwconv1.weight",
              "db1": "pwconv1.bias", "dW2": "pwconv2.weight", "db2": "pwconv2.bias", "dgamma": "gamma"}


def cx_chain32(p, x, dy):
    """The block and its backward stage by stage in float32 on the CPU with torch: the tensors every stage was fed (`ws`, the names of the
    workspace plus DGpre) and what it produced (`out`, the names of cx_forward_refs / cx_backward_refs)."""
    C = x.shape[1]
    leaf = lambda t: t.detach().clone().requires_grad_()

    def vjp(fn, ins, grad):
        ins = [leaf(t) for t in ins]
        return torch.autograd.grad(fn(*ins), ins, grad)

    H0 = dwconv(x, p["dwconv.weight"], p["dwconv.bias"])
    ln = lambda h, w, b: F.layer_norm(h.permute(0, 2, 1), (C,), w, b, EPS).permute(0, 2, 1)
    H1 = ln(H0, p["norm.weight"], p["norm.bias"]).contiguous()
    U = pw(H1, p["pwconv1.weight"], p["pwconv1.bias"])
    G = F.gelu(U)
    V = pw(G, p["pwconv2.weight"], p["pwconv2.bias"])
    y = x + col(p["gamma"]) * V
    DV = dy * col(p["gamma"])
    dgamma = (dy * V).sum((0, 2))
    DGpre = pw(DV, p["pwconv2.weight"].t().contiguous())
    dU, = vjp(F.gelu, [U], DGpre)
    DH1 = pw(dU, p["pwconv1.weight"].t().contiguous())
    DH0, dln_w, dln_b = vjp(ln, [H0, p["norm.weight"], p["norm.bias"]], DH1)
    dxc, ddw, ddb = vjp(dwconv, [x, p["dwconv.weight"], p["dwconv.bias"]], DH0)
    ws = dict(H0=H0, H1=H1, U=U, G=G, V=V, DV=DV, DG=dU, DH1=DH1, DH0=DH0, DGpre=DGpre)
    out = dict(H0=H0, H1=H1, G=G, y=y, DV=DV, dgamma=dgamma, dU=dU, DH0=DH0, dln_w=dln_w, dln_b=dln_b, dx=dy + dxc, ddw=ddw, ddb=ddb)
    return {k: v.detach() for k, v in ws.items()}, {k: v.detach() for k, v in out.items()}


# ==================================================================================== FSQ
FSQ_LEVELS = ([7, 5, 5], [8, 6], [5], [8, 5, 5, 5])
FSQ_KINDS = [(tuple(lv), pb) for lv in FSQ_LEVELS for pb in (True, False)]
# (G, B, T4): B * G * T4 tokens.  G = 1: 1, 255, 256, 257, 600; G = 3 has multiples of 3 only: 3, 255, 258 (across the 256-thread block), 600
FSQ_TOKENS = [(1, 1, 1), (1, 5, 51), (1, 1, 256), (1, 1, 257), (1, 3, 200), (3, 1, 1), (3, 5, 17), (3, 2, 43), (3, 4, 50)]
# (levels, prebound, C, G, B, T4): every kind with every token count, C = 1 and 70 alternating so that each count meets both
FSQ_CASES = [(lv, pb, (1, 70)[(i + j) % 2], G, B, T4) for i, (lv, pb) in enumerate(FSQ_KINDS) for j, (G, B, T4) in enumerate(FSQ_TOKENS)]
# decode: the same cases (their ids start at code 0 and wrap at the codebook size), and for every kind two cases that EACH enumerate the whole
# codebook -- prod(levels) is 175, 48, 5 and 1000, above the 600 tokens of the largest case for [8, 5, 5, 5]: G = 3 with C = 70, G = 1 with C = 1
FSQ_DECODE_FULL = [c for lv, pb in FSQ_KINDS for c in ((lv, pb, 70, 3, 1, -(-math.prod(lv) // 3)), (lv, pb, 1, 1, 2, -(-math.prod(lv) // 2)))]
FSQ_DECODE_CASES = FSQ_CASES + FSQ_DECODE_FULL
# fsq_bwd_param_kernel walks B * T4 points with stride 256: 1, 63, 255, 256, 257, 700 points with B = 1, and with a B > 1 wherever the count
# has a factor (B * T4 is a multiple of B; odd B where there is one, so that item boundaries fall inside a 256-point pass)
FSQ_BWD_POINTS = [(1, 1), (1, 63), (7, 9), (1, 255), (3, 85), (1, 256), (4, 64), (1, 257), (1, 700), (7, 100)]
FSQ_BWD_CASES = [(lv, pb, (70, 1)[(i + j) % 4 == 3], (1, 3)[(i + j) % 2], B, T4)
                 for i, (lv, pb) in enumerate(FSQ_KINDS) for j, (B, T4) in enumerate(FSQ_BWD_POINTS)]
FSQ_ITEM_CASES = [((7, 5, 5), True, 70, 3, 5, 37), ((8, 6), False, 70, 1, 5, 37), ((8, 5, 5, 5), True, 1, 3, 5, 37)]
FSQ_ITEM_LENS = lambda T4: [0, T4 // 2, T4, T4 + 5, -3]      # the last two are clamped on the device
NEAR_CAP = 0.005                 # at most 0.5 % of (token, level) pairs may lie nearer to a rounding boundary than their own bound
BWD_MARGIN = 1e-4


def fsq_id(s):
    lv, pb, C, G, B, T4 = s
    return f"L{'x'.join(map(str, lv))}-{'pre' if pb else 'raw'}-C{C}-G{G}-B{B}-T{T4}"


def fsq_constants(levels):
    """make_fsq_const (csrc/small_ops.hip), in its own fp32 arithmetic: half_l = (L - 1) * 1.001f / 2, offset, half_width, basis; the shift
    atanh(offset / half_l) in float64 of those fp32 values (what strict mode uses; the kernel's atanhf rounds it once)."""
    lv = np.asarray(levels)
    half_l = (lv - 1).astype(np.float32) * np.float32(1.001) / np.float32(2.0)
    offset = np.where(lv % 2 == 0, np.float32(0.5), np.float32(0.0)).astype(np.float32)
    shift = np.arctanh(offset.astype(np.float64) / half_l.astype(np.float64))
    basis = np.concatenate([[1], np.cumprod(lv[:-1])])
    t = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt)
    return dict(levels=t(lv, torch.int64), half_l=t(half_l, torch.float64), offset=t(offset, torch.float64), shift=t(shift, torch.float64),
                half_width=t(lv // 2, torch.int64), basis=t(basis, torch.int64))


def fsq_operands(case, draw=0):
    """fp32 operands of one case in the packed layouts: w_in (G, D, C), b_in (G, D), w_out (G, C, D), b_out (G, C); z, dout (B*G, C, T4)."""
    lv, pb, C, G, B, T4 = case
    D = len(lv)
    g = torch.Generator().manual_seed(sum(lv) * 1000003 + pb * 7919 + C * 131 + G * 17 + B * 5 + T4 + 1000 * draw)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(w_in=rn(G, D, C) * (1.5 / math.sqrt(C)), b_in=rn(G, D) * 0.3, w_out=rn(G, C, D) / math.sqrt(D), b_out=rn(G, C) * 0.1,
                z=rn(B * G, C, T4), dout=rn(B * G, C, T4))


def fsq_rows(z, B, G):
    """(B*G, C, T4) -> (G, B, T4, C): the layout of prequant"""
    return z.view(B, G, z.shape[1], z.shape[2]).permute(1, 0, 3, 2)


def fsq_prequant(op, case, dtype=torch.float64):
    """prequant = bound(bound?(W_in z + b_in)) in (G, B, T4, D) with its scale A (float64 only), bound(v) = tanh(v + shift) half_l - offset.
    Propagation: the Linear's error is tau * A_lin, A_lin = sum |w| |z| + |b|.  |d bound / dv| <= half_l, the sum v + shift rounds on
    |v| + |shift|, and tanhf's own rounding sits on half_l |tanh| + |offset| <= half_l + |offset|:
        A_bound(A_v) = half_l (A_v + |shift|) + half_l + |offset|,   applied twice when pre-bounded."""
    lv, pb, C, G, B, T4 = case
    k = fsq_constants(lv)
    hl, of, sh = (k[n].to(dtype) for n in ("half_l", "offset", "shift"))
    zr = fsq_rows(op["z"].to(dtype), B, G)
    w, b = op["w_in"].to(dtype), op["b_in"].to(dtype)
    v = torch.einsum("gbtc,gdc->gbtd", zr, w) + b[:, None, None, :]
    A = torch.einsum("gbtc,gdc->gbtd", zr.abs(), w.abs()) + b.abs()[:, None, None, :]
    for _ in range(2 if pb else 1):
        v = torch.tanh(v + sh) * hl - of
        A = hl * (A + sh.abs()) + hl + of.abs()
    return v, A


def fsq_prequant32(op, case):
    """The fp32 CPU reference (torch in float32, fp32 constants with atanh in fp32)."""
    lv, pb, C, G, B, T4 = case
    k = fsq_constants(lv)
    hl, of = k["half_l"].float(), k["offset"].float()
    sh = torch.atanh(of / hl)
    v = torch.einsum("gbtc,gdc->gbtd", fsq_rows(op["z"], B, G), op["w_in"]) + op["b_in"][:, None, None, :]
    for _ in range(2 if pb else 1):
        v = torch.tanh(v + sh) * hl - of
    return v


def fsq_digits(pre, levels):
    """rint (half to even) of the pre-quantised value plus half_width: the digit of every (token, level), int64"""
    return torch.round(pre.double()).to(torch.int64) + fsq_constants(levels)["half_width"]


def fsq_pack(digits, levels, B, G):
    """digits (G, B, T4, D) -> ids (B, G, T4) int32"""
    return (digits * fsq_constants(levels)["basis"]).sum(-1).permute(1, 0, 2).contiguous().to(torch.int32)


def fsq_unpack(ids, levels):
    """ids (B, G, T4) -> digits (G, B, T4, D)"""
    k = fsq_constants(levels)
    return ((ids.to(torch.int64).permute(1, 0, 2).unsqueeze(-1) // k["basis"]) % k["levels"])


def fsq_safe(pre64, A):
    """(token, level) pairs whose float64 pre-quantised value lies farther from an x.5 boundary than that element's own bound"""
    return (pre64 - torch.floor(pre64) - 0.5).abs() > tau("fsq prequant") * A


def fsq_decode_ids(case):
    """the codes 0, 1, 2, ... in token order, wrapping at the codebook size: ids (B, G, T4) int32.  A case of at least prod(levels) tokens
    (FSQ_DECODE_FULL) enumerates every code."""
    lv, pb, C, G, B, T4 = case
    return (torch.arange(B * G * T4, dtype=torch.int64) % math.prod(lv)).to(torch.int32).view(B, G, T4)


def fsq_decode_ref(op, case, ids, dtype=torch.float64):
    """z = W_out code + b_out, code = (digit - half_width) / half_width            A = sum |w| |code| + |b|        -> (B*G, C, T4)"""
    lv, pb, C, G, B, T4 = case
    k = fsq_constants(lv)
    hw = k["half_width"].to(dtype)
    code = (fsq_unpack(ids, lv).to(dtype) - hw) / hw                          # (G, B, T4, D)
    w, b = op["w_out"].to(dtype), op["b_out"].to(dtype)
    z = torch.einsum("gbtd,gcd->bgct", code, w) + b[None, :, :, None]
    A = torch.einsum("gbtd,gcd->bgct", code.abs(), w.abs()) + b.abs()[None, :, :, None]
    return z.reshape(B * G, C, T4), A.reshape(B * G, C, T4)


@functools.lru_cache(maxsize=None)
def fsq_bwd_operands(case):
    """The operands of a backward case: x is redrawn (deterministically, at most 20 times) until the float64 pre-quantised value keeps
    1e-4 from every rounding boundary -- nearer, the code and with it the whole straight-through gradient may legitimately differ."""
    for draw in range(20):
        op = fsq_operands(case, draw)
        pre, _ = fsq_prequant(op, case)
        if float((pre - torch.floor(pre) - 0.5).abs().min()) > BWD_MARGIN:
            return op
    raise AssertionError(f"{fsq_id(case)}: no input with a {BWD_MARGIN} rounding margin in 20 draws")


def fsq_backward_refs(op, case):
    """The straight-through backward (csrc/small_ops.hip, above fsq_bwd_point_kernel) in float64, x = op['z']:
         z3 = W_in x + b_in; [t0 = tanh(z3 + shift), zz = t0 half_l - offset, f0 = half_l (1 - t0^2)]; t1 = tanh(zz + shift);
         code = rint(t1 half_l - offset) / half_width; dcode = W_out^T dout; dz3 = dcode / half_width half_l (1 - t1^2) f0;
         dx = W_in^T dz3; dW_in = sum dz3 (x) x; db_in = sum dz3; dW_out = sum dout (x) code; db_out = sum dout.
    A: the same with absolute operands and 1 + t^2 for 1 - t^2.      -> name -> (ref, [(mode, A)])"""
    lv, pb, C, G, B, T4 = case
    k = fsq_constants(lv)
    hl, of, sh, hw = k["half_l"], k["offset"], k["shift"], k["half_width"].double()
    xr, dr = fsq_rows(op["z"].double(), B, G), fsq_rows(op["dout"].double(), B, G)               # (G, B, T4, C)
    w_in, b_in, w_out = op["w_in"].double(), op["b_in"].double(), op["w_out"].double()
    zz = torch.einsum("gbtc,gdc->gbtd", xr, w_in) + b_in[:, None, None, :]
    f0 = f0a = torch.ones_like(zz)
    if pb:
        t0 = torch.tanh(zz + sh)
        zz, f0, f0a = t0 * hl - of, hl * (1 - t0 * t0), hl * (1 + t0 * t0)
    t1 = torch.tanh(zz + sh)
    code = torch.round(t1 * hl - of) / hw
    dcode = torch.einsum("gbtc,gcd->gbtd", dr, w_out)
    dcode_a = torch.einsum("gbtc,gcd->gbtd", dr.abs(), w_out.abs())
    dz3 = dcode / hw * hl * (1 - t1 * t1) * f0
    dz3a = dcode_a / hw * hl * (1 + t1 * t1) * f0a
    back = lambda t: t.permute(1, 0, 3, 2).reshape(B * G, C, T4)
    return {
        "dx": (back(torch.einsum("gbtd,gdc->gbtc", dz3, w_in)), [("fsq dx", back(torch.einsum("gbtd,gdc->gbtc", dz3a, w_in.abs())))]),
        "dw_in": (torch.einsum("gbtd,gbtc->gdc", dz3, xr), [("fsq dparams", torch.einsum("gbtd,gbtc->gdc", dz3a, xr.abs()))]),
        "db_in": (dz3.sum((1, 2)), [("fsq dparams", dz3a.sum((1, 2)))]),
        "dw_out": (torch.einsum("gbtc,gbtd->gcd", dr, code), [("fsq dparams", torch.einsum("gbtc,gbtd->gcd", dr.abs(), code.abs()))]),
        "db_out": (dr.sum((1, 2)), [("fsq dparams", dr.abs().sum((1, 2)))]),
    }


def fsq_backward32(op, case):
    """The fp32 CPU reference: autograd through the straight-through forward in float32."""
    lv, pb, C, G, B, T4 = case
    k = fsq_constants(lv)
    hl, of, hw = k["half_l"].float(), k["offset"].float(), k["half_width"].float()
    sh = torch.atanh(of / hl)
    x, w_in, b_in, w_out, b_out = (op[n].detach().clone().requires_grad_() for n in ("z", "w_in", "b_in", "w_out", "b_out"))
    v = torch.einsum("gbtc,gdc->gbtd", fsq_rows(x, B, G), w_in) + b_in[:, None, None, :]
    for _ in range(2 if pb else 1):
        v = torch.tanh(v + sh) * hl - of
    code = (v + (torch.round(v) - v).detach()) / hw
    out = torch.einsum("gbtd,gcd->gbtc", code, w_out) + b_out[:, None, None, :]
    (out * fsq_rows(op["dout"], B, G)).sum().backward()
    return {"dx": x.grad, "dw_in": w_in.grad, "db_in": b_in.grad, "dw_out": w_out.grad, "db_out": b_out.grad}


# ==================================================================================== the reference ratios
def reference_ratios(progress=None):
    """mode -> largest max |y32 - ref64| / A of the fp32 CPU reference over the cases of both GPU modules, and the near-boundary statistics
    of the fp32 reference's ids: (pairs nearer than their bound, ids that differ outside them, pairs)."""
    got = {m: 0.0 for m in R}

    def take(refs, y32):
        for name, (ref, terms) in refs.items():
            if name in y32 and len(terms) == 1 and terms[0][0] in got:
                got[terms[0][0]] = max(got[terms[0][0]], err_over(y32[name], ref, [(1.0, terms[0][1])]))

    for shape in CX_CASES + [CX_LONG, (494, 1, 33), (CX_ITEMS[0], 1, CX_ITEMS[1])]:
        c = cx_case(shape)
        ws, out = cx_chain32(c["p"], c["x"], c["dy"])
        take(cx_forward_refs(c["p"], c["x"], ws), out)
        take(cx_backward_refs(c["p"], c["x"], c["dy"], ws, dgpre=ws["DGpre"], only=()), out)
        if progress:
            progress(cx_id(shape))
    near = wrong = pairs = 0
    for case in FSQ_CASES + FSQ_ITEM_CASES:
        op = fsq_operands(case)
        pre, A = fsq_prequant(op, case)
        pre32 = fsq_prequant32(op, case)
        got["fsq prequant"] = max(got["fsq prequant"], err_over(pre32, pre, [(1.0, A)]))
        safe = fsq_safe(pre, A)
        near += int((~safe).sum())
        pairs += safe.numel()
        wrong += int(((fsq_digits(pre32, case[0]) != fsq_digits(pre, case[0])) & safe).sum())
    for case in FSQ_DECODE_CASES + FSQ_ITEM_CASES:
        op = fsq_operands(case)
        ids = fsq_decode_ids(case)
        z, Az = fsq_decode_ref(op, case, ids)
        got["fsq decode"] = max(got["fsq decode"], err_over(fsq_decode_ref(op, case, ids, torch.float32)[0], z, [(1.0, Az)]))
    for case in FSQ_BWD_CASES:
        op = fsq_bwd_operands(case)
        take(fsq_backward_refs(op, case), fsq_backward32(op, case))
    return got, (near, wrong, pairs)
