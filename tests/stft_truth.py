"""The STFT front end and its backward, stated in float64, and the case matrix the GPU tests run (tests/test_gpu_stft_matrix.py,
tests/test_gpu_stft_bwd_matrix.py; tests/test_stft_truth_cpu.py checks this file itself without a GPU).  No tests in here.

The operation (utils/spectrogram.py:58-79): reflect-pad by (n_fft - hop) / 2, frames of n_fft samples every hop, periodic Hann of
win_length centred in n_fft, one-sided DFT, sqrt(re^2 + im^2 + 1e-9), Slaney mel basis, log(clamp(., 1e-5)).

Errors are measured in units of eps = 2^-24 (half an fp32 ulp, relative) of what an fp32 transform can resolve: the error of a bin
follows the energy of its FRAME (the L2 norm of the windowed samples), not the magnitude of the bin, so
    e_lin = max |y - mag64| / (eps (norm[b, t] + mag64[b, t, k]))
    e_mel = max |mel - mel64| / (eps sum_k basis[m, k] (norm[b, t] + mag64[b, t, k]))        over bands with at least one bin
stay of order 10 for any fp32 FFT on any signal (bin-centred tone with 160 dB of range included), where a per-element relative error is
meaningless in empty bins and a max-norm one hides every quiet bin behind the loudest."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
LOG_FLOOR = 1e-5                     # the clamp in front of the log


# ------------------------------------------------------------------------------------ the operation in float64
def window64(n_fft, win, window32=None):
    """the fp32 window of `win` samples the kernel is handed (the periodic Hann unless one is given), centred in n_fft, as float64"""
    w = torch.zeros(n_fft, dtype=torch.float64)
    off = (n_fft - win) // 2
    w[off:off + win] = (torch.hann_window(win, dtype=torch.float32) if window32 is None else window32).double()
    return w


def frames64(x, n_fft, win, hop, window32=None):
    """x (B, L) -> (windowed frames (B, T, n_fft), their L2 norms (B, T)), float64, T = L // hop"""
    pad = (n_fft - hop) // 2
    xp = F.pad(x.double()[:, None, :], (pad, pad), mode="reflect")[:, 0] if pad else x.double()
    fr = xp.unfold(1, n_fft, hop) * window64(n_fft, win, window32)
    return fr, fr.norm(dim=-1)


def mag64(frames):
    """(B, T, n_fft) -> (B, T, n_fft / 2 + 1)"""
    s = torch.fft.rfft(frames, dim=-1)
    return torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-9)


def mel64(mag, basis32):
    """mag (B, T, K), basis32 (M, K) float32 -> (B, M, T): basis32.double() @ mag; the caller takes log(clamp(., 1e-5))"""
    return torch.matmul(torch.as_tensor(basis32).double(), mag.transpose(1, 2))


def e_lin(y, mag, norm):
    """y (B, T, K) in any float type against mag64 / norm of the same clip"""
    return float(((y.double().cpu() - mag).abs() / (EPS * (norm[..., None] + mag))).max())


def mel_scale(mag, norm, basis32):
    """(B, M, T): sum_k basis[m, k] (norm[b, t] + mag64[b, t, k]); zero exactly for the bands without a bin"""
    b = torch.as_tensor(basis32).double()
    return torch.matmul(b, (norm[..., None] + mag).transpose(1, 2))


def e_mel(ylog, mag, norm, basis32):
    """ylog (B, M, T): a LOG-mel output.  It is taken back through exp in float64 (exact to 1e-16, and free of the asymmetry of the log
    where the error is not small against the value), compared with max(mel64, 1e-5), and relieved of what the log itself and the fp32
    constant 1e-5f may round: 2 ulp = 4 eps of |log| on the output is a relative 4 eps |log| on exp(output), the constant one more eps.
    What is left is measured in eps * mel_scale, over the bands that have a bin."""
    basis32 = torch.as_tensor(basis32)
    m = mel64(mag, basis32).clamp_min(LOG_FLOOR)
    d = ((ylog.double().cpu().exp() - m).abs() - EPS * (4.0 * m.log().abs() + 1.0) * m).clamp_min(0.0)
    has = (basis32 != 0).any(dim=1)
    return float((d[:, has] / (EPS * mel_scale(mag, norm, basis32)[:, has])).max())


# ------------------------------------------------------------------------------------ mel tables
Mel = namedtuple("Mel", "sr n_fft n_mels f_min f_max")     # f_max None = sr / 2 (0.0 in the C ABI)

PROD_24K = Mel(24000, 1024, 100, 0.0, 12000.0)
PROD_16K = Mel(16000, 1024, 80, 0.0, None)
MEL_EDGES = {                                               # id -> (table, the property it is in the matrix for)
    "48k_512_128": (Mel(48000, 512, 128, 0.0, None), dict(empty=13, nyquist=True)),
    "44k_2048_128": (Mel(44100, 2048, 128, 0.0, None), dict(chunks=314, passes=5, nyquist=True)),
    "8k_2048_128": (Mel(8000, 2048, 128, 0.0, None), dict(chunks=332, passes=6)),
    "24k_512_1": (Mel(24000, 512, 1, 0.0, None), dict(widest=255, chunks=32, passes=1)),
    "24k_1024_64": (Mel(24000, 1024, 64, 0.0, None), dict(empty=0)),
    "24k_1024_65": (Mel(24000, 1024, 65, 0.0, None), dict(empty=0)),
    "24k_1024_80_50_7600": (Mel(24000, 1024, 80, 50.0, 7600.0), dict(top_bin=324)),
    "prod_24k": (PROD_24K, dict(empty=0)),
    "prod_16k": (PROD_16K, dict(empty=0)),
}
GEOM_MEL = {512: Mel(24000, 512, 80, 0.0, None), 1024: PROD_24K, 2048: Mel(24000, 2048, 80, 0.0, None)}   # the table of a geometry case
MEL_CHUNK, MAX_MEL_PASSES = 8, 6                            # kMelChunk, kMaxMelPasses of csrc/stft_logmel.hip


def mel_basis(mel):
    from oracle import ref_cpu
    return torch.from_numpy(ref_cpu.slaney_mel_basis(mel.sr, mel.n_fft, mel.n_mels, mel.f_min, mel.f_max)).float()


def mel_properties(basis32):
    """what the kernel's plan derives from a basis: per band first bin .. last bin, cut into chunks of 8"""
    nz = torch.as_tensor(basis32) != 0
    cnt = []
    for row in nz:
        idx = torch.nonzero(row).flatten()
        cnt.append(int(idx[-1] - idx[0]) + 1 if idx.numel() else 0)
    chunks = sum(-(-c // MEL_CHUNK) for c in cnt)
    cols = torch.nonzero(nz.any(dim=0)).flatten()
    return dict(empty=sum(c == 0 for c in cnt), nyquist=bool(nz[:, -1].any()), chunks=chunks, passes=max(1, -(-chunks // 64)),
                widest=max(cnt), top_bin=int(cols[-1]))


def floor_lin():
    """e_floor of the linear output, from the kernel's operation count behind an exact re / im: the fp32 constant 1e-9f (1/2 ulp of it),
    the add that folds it in (1/2 ulp) and the 1-ulp v_sqrt; the square root halves what precedes it, the sum is bounded by 2 ulp = 4 eps."""
    return 4.0


def floor_mel(basis32):
    """e_floor of the mel output: floor_lin on every magnitude, plus the longest summation chain of the mel stage -- 8 fmas per chunk
    and one add per chunk of the widest band, 1/2 ulp = 1 eps each, of partial sums that never exceed the band's value (all terms >= 0).
    (The rounding of the log and of 1e-5f is taken out by e_mel itself.)"""
    return floor_lin() + MEL_CHUNK + -(-mel_properties(basis32)["widest"] // MEL_CHUNK)


# ------------------------------------------------------------------------------------ forward cases
Fwd = namedtuple("Fwd", "id n_fft hop win L B mel signal")


def _geometry():
    out = []
    for n in (512, 1024, 2048):
        hop, pad = n // 4, (n - n // 4) // 2
        out.append(Fwd(f"{n}-smallest", n, hop, n, max(pad + 1, hop), 2, GEOM_MEL[n], "noise"))
        out.append(Fwd(f"{n}-short-T1", n, hop, n, 200 * n // 512, 2, GEOM_MEL[n], "noise"))          # 200, 400, 800 < n_fft
        for T in (7, 8, 9, 31, 32, 33, 65):
            out.append(Fwd(f"{n}-T{T}", n, hop, n, T * hop, 2, GEOM_MEL[n], "noise"))
            out.append(Fwd(f"{n}-T{T}-tail", n, hop, n, T * hop + hop - 1, 2, GEOM_MEL[n], "noise"))
        out.append(Fwd(f"{n}-hop-is-n_fft", n, n, n, 3 * n, 2, GEOM_MEL[n], "noise"))
    out.append(Fwd("512-hop2", 512, 2, 512, 600, 2, GEOM_MEL[512], "noise"))
    for n, hop, win in ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)):                        # the MR-STFT resolutions
        out.append(Fwd(f"mrstft-{n}-{hop}-{win}", n, hop, win, 33 * hop + hop - 1, 2, GEOM_MEL[n], "noise"))
    out.append(Fwd("1024-odd-window-801", 1024, 256, 801, 33 * 256, 2, GEOM_MEL[1024], "noise"))
    return out


def _tables():
    return [Fwd(f"mel-{k}", m.n_fft, m.n_fft // 4, m.n_fft, 33 * (m.n_fft // 4), 2, m, "noise") for k, (m, _) in MEL_EDGES.items()]


def _signals():
    out = []
    for n in (1024, 512, 2048):
        kinds = ["zeros", "ones", "impulse3", "alternating"] + (["tone", "noise*1e-6", "noise*3e4"] if n == 1024 else [])
        out += [Fwd(f"signal-{n}-{s}", n, n // 4, n, 33 * (n // 4), 2, GEOM_MEL[n], s) for s in kinds]
    return out


GEOMETRY, TABLES, SIGNALS = _geometry(), _tables(), _signals()
FORWARD = GEOMETRY + TABLES + SIGNALS


def signal(case):
    """(B, L) float32, seeded by the case"""
    B, L, s = case.B, case.L, case.signal
    g = torch.Generator().manual_seed(sum(map(ord, case.id)) + case.L)
    noise = torch.randn(B, L, generator=g) * 0.3
    if s == "noise":
        return noise
    if s.startswith("noise*"):
        return noise * float(s[6:])
    if s == "zeros":
        return torch.zeros(B, L)
    if s == "ones":
        return torch.ones(B, L)
    if s == "impulse3":                                    # sample 3: also mirrored into the left reflection of frames 0 and 1
        x = torch.zeros(B, L)
        x[:, 3] = 1.0
        return x
    if s == "alternating":
        return (1.0 - 2.0 * (torch.arange(L) % 2).float()).expand(B, L).contiguous()
    if s == "tone":                                        # the bin nearest 1 kHz, exactly on the bin, + 1e-4 noise
        k = round(1000.0 * case.n_fft / case.mel.sr)
        t = torch.arange(L, dtype=torch.float64)
        return (torch.sin(2.0 * math.pi * k * t / case.n_fft).float() + noise * (1e-4 / 0.3)).contiguous()
    raise ValueError(s)


def truth(case, x):
    """-> dict(mag (B, T, K), norm (B, T), basis (M, K) float32), float64"""
    fr, norm = frames64(x, case.n_fft, case.win, case.hop)
    return dict(mag=mag64(fr), norm=norm, basis=mel_basis(case.mel))


def oracle32(case, x):
    """the fp32 oracle on the same input -> (log-mel (B, M, T), linear (B, T, K))"""
    from oracle import ref_cpu
    m = case.mel
    args = (m.sr, case.n_fft, case.win, case.hop, m.n_mels, m.f_min, m.f_max)
    return ref_cpu.stft_logmel(x, *args), ref_cpu.stft_logmel(x, *args, return_linear=True).transpose(1, 2)


# ------------------------------------------------------------------------------------ backward
Bwd = namedtuple("Bwd", "id n_fft hop win L B window", defaults=("hann",))


def _backward():
    out = []
    for n in (512, 1024, 2048):
        out.append(Bwd(f"{n}-short-T1", n, n // 4, n, 200 * n // 512, 2))
        # hop = n_fft / 2: the last n_fft / 4 - 1 samples lie in no frame and in no reflection that a frame reads
        out.append(Bwd(f"{n}-tail", n, n // 2, n, 5 * (n // 2) + n // 2 - 1, 2))
        out.append(Bwd(f"{n}-tail-quarter-hop", n, n // 4, n, 5 * (n // 4) + n // 4 - 1, 1))
        out.append(Bwd(f"{n}-hop-is-n_fft", n, n, n, 3 * n, 2))
    out += [Bwd(f"512-hop16-T{T}", 512, 16, 512, T * 16, 1) for T in (255, 256, 257)]
    out += [Bwd(f"512-hop128-L{L}", 512, 128, 512, L, 2) for L in (767, 768, 769)]
    out.append(Bwd("512-hop2", 512, 2, 512, 600, 1))
    out.append(Bwd("1024-B3", 1024, 256, 1024, 2000, 3))
    # The periodic Hann all but vanishes at both ends (w[n_fft - 1] = 4e-5 at 512, w[0] = 0), and with it every term that only the first or
    # last window position contributes -- the outermost mirror images of the overlap-add among them.  A window without small entries
    # (dmel_stft_grad_create takes any) gives those terms full weight; L = T hop, so that the last padded sample is read.
    out += [Bwd(f"{n}-full-window", n, n // 4, n, 6 * (n // 4), 2, "full") for n in (512, 1024)]
    return out


BACKWARD = _backward()


def first_untouched(case):
    """the first sample no frame reads, directly or through a reflection (>= L: there is none)"""
    pad = (case.n_fft - case.hop) // 2
    return (case.L // case.hop - 1) * case.hop + case.n_fft - pad


def backward_window(case):
    """the fp32 window of a backward case, (win,): None = the periodic Hann; "full" = seeded, every entry in [0.5, 1]"""
    if case.window == "hann":
        return None
    assert case.window == "full"
    return 0.5 + 0.5 * torch.rand(case.win, generator=torch.Generator().manual_seed(case.n_fft + 7))


def backward_inputs(case):
    """-> (x (B, L) f32, g (B, T, K) f32): g = d loss / d mag of  sum w mag + sum log(mag + 0.3)  at the float64 magnitudes, rounded to
    fp32 once -- the cotangent is an input the backward is handed, the same for every implementation"""
    gen = torch.Generator().manual_seed(case.n_fft + case.hop + case.L)
    x = torch.randn(case.B, case.L, generator=gen) * 0.3
    T, K = case.L // case.hop, case.n_fft // 2 + 1
    w = torch.randn(case.B, T, K, generator=gen)
    mag = mag64(frames64(x, case.n_fft, case.win, case.hop, backward_window(case))[0])
    return x, (w.double() + 1.0 / (mag + 0.3)).float()


def backward64(case, x, g):
    """-> (dy64 (B, L), scale (B, L)).  dy64: autograd through frames64 / mag64.  scale: the same gradient with the absolute value of
    every term taken -- sum over the frames t and window positions n that read sample j (reflections included) of
    |w[n]| sum_k |dre[t, k] cos(2 pi k n / N)| + |dim[t, k] sin(2 pi k n / N)|,  dre / dim = g re / mag, g im / mag."""
    n_fft, win, hop = case.n_fft, case.win, case.hop
    x64 = x.double().requires_grad_()
    w32 = backward_window(case)
    fr, _ = frames64(x64, n_fft, win, hop, w32)
    (mag64(fr) * g.double()).sum().backward()
    with torch.no_grad():
        s = torch.fft.rfft(fr.detach(), dim=-1)
        mag = torch.sqrt(s.real ** 2 + s.imag ** 2 + 1e-9)
        dre, dim = (g.double() * s.real / mag).abs(), (g.double() * s.imag / mag).abs()
        ang = 2.0 * math.pi * torch.outer(torch.arange(n_fft // 2 + 1, dtype=torch.float64), torch.arange(n_fft, dtype=torch.float64)) / n_fft
        sframe = (dre @ ang.cos().abs() + dim @ ang.sin().abs()) * window64(n_fft, win, w32).abs()       # (B, T, n_fft), every entry >= 0
    # overlap-add and the fold of the reflect padding are the adjoint of pad + unfold: let autograd apply it to the non-negative frames
    z = torch.zeros_like(x64, requires_grad=True)
    pad = (n_fft - hop) // 2
    zp = F.pad(z[:, None, :], (pad, pad), mode="reflect")[:, 0] if pad else z
    (zp.unfold(1, n_fft, hop) * sframe).sum().backward()
    return x64.grad, z.grad


def backward32(case, x, g):
    """fp32 autograd through the oracle's torch.stft restatement (the same call with the case's window where that is not the Hann)"""
    from oracle import ref_cpu
    x32 = x.clone().requires_grad_()
    w32 = backward_window(case)
    if w32 is None:
        mag = ref_cpu.stft_magnitude(x32, case.n_fft, case.win, case.hop)
    else:
        pad = (case.n_fft - case.hop) // 2
        spec = torch.view_as_real(torch.stft(F.pad(x32[:, None, :], (pad, pad), mode="reflect")[:, 0], case.n_fft, hop_length=case.hop,
                                             win_length=case.win, window=w32, center=False, onesided=True, return_complex=True))
        mag = torch.sqrt(spec.pow(2).sum(-1) + 1e-9)
    (mag.transpose(1, 2) * g).sum().backward()
    return x32.grad


def floor_bwd(case):
    """In units of eps * scale, behind an exact spectrum (what the forward GEMM adds to re / im is left to the 3 e_ref clause), from the
    arithmetic csrc/stft_bwd.hip actually runs:
      * spectrum step: sqrt, division and two products on every g re / mag, 1 eps each                                       -> 4
      * the transposed DFT is launch_conv at DMEL_PRECISION_FP32, the six-product bf16 split of csrc/conv_igemm.hip: the three
        dropped partial products are below 2^-21 |a b| (its header comment)                                                   -> 8
      * one fp32 accumulator per output walks K = n_fft + 2 channels in steps of 16, six MFMAs per step, and the overlap-add then adds
        at most ceil(n_fft / hop) frames for the sample and each of its two mirror images: m = 6 ceil((n_fft + 2) / 16) +
        3 ceil(n_fft / hop) roundings, each at most eps of a partial sum that never exceeds the sum of the absolute terms, i.e. `scale`.
        The worst case, m eps, is what no run comes near (512 .. 2066 here); with the roundings independent and zero-mean (Higham and
        Mary, "A new approach to probabilistic rounding error analysis", 2019) their sum has a standard deviation of at most
        eps scale sqrt(m / 3), and six of those are exceeded by one element in 5e8                                            -> 6 sqrt(m / 3)
    61 / 80 / 108 at n_fft 512 / 1024 / 2048 with hop = n_fft / 4.  Still above what a Hann-weighted outermost term weighs (w[n_fft - 1]
    ~ 1e-5): the two full-window cases are there for those."""
    m = 6 * -(-(case.n_fft + 2) // 16) + 3 * -(-case.n_fft // case.hop)
    return 4.0 + 8.0 + 6.0 * math.sqrt(m / 3.0)


MAXNORM_BWD = 2e-5                   # the floor of test_stft_magnitude_backward_matches_autograd, max |dy - dy64| / max |dy64|


def legal(n_fft, hop, L):
    pad = (n_fft - hop) // 2
    return (n_fft - hop) % 2 == 0 and 0 < hop <= n_fft and L > pad and L >= hop and 1 + (L + 2 * pad - n_fft) // hop == L // hop
