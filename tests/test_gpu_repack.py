"""The device-side weight re-pack (dmel_*_refresh: repack_kernel / repack_unit in csrc/train_ops.hip, weight_norm_fwd_kernel in
csrc/modules.hip) held to the host packer (pack_conv, csrc/conv.h), image by image.

Every trainable image is described ONCE, next to the image itself (WeightImage::src in csrc/modules.hip, filled in by the finalize
code of each module): affine views over named tensors.  Routes A and B below share that
description and differ in the EVALUATOR: the host accessor view_weight / view_bias under pack_conv against repack_unit on the device,
each with its own copy of the addressing and of the four roundings.  That is what this module proves: the two evaluators agree bit for
bit.  That the descriptions themselves are right is held by the float64 comparisons here and in test_gpu_parity.py, and by the recorded
image fingerprints of tests/test_host_asan.py.

From the second optimiser step on, every convolution of a training run reads images written by that kernel.  Each case here
reaches the same parameter values W2 by two routes:
  (A) rebuild: a fresh handle packed on the host from W2 (set_tensor + finalize);
  (B) refresh: a handle packed on the host from UNRELATED values W1, then re-packed ONCE on the device to W2.
W1 and W2 are independent draws, so a stale, skipped or mis-addressed image is an O(1) error; inputs are the same on both routes.

What is compared, and how:
  * determinism control: route A is built twice.  Outputs and input gradients of two rebuilds must be torch.equal (asserted), and
    then A and B must be torch.equal too -- at every forward precision (all four images w48 / w32h / w / w16 are read) and every
    training mode (the transposed, tap-reversed, phase-major backward images are read), switched on the refreshed handle WITHOUT
    another refresh;
  * parameter gradients come out of weight- / bias-gradient kernels that accumulate with atomics: two rebuilds are not always
    torch.equal in them (how many were is reported), so A and B are not compared with each other; each is compared with
    float64 autograd through oracle/ref_cpu.py at W2, under the bars the per-module tests of test_gpu_parity.py apply to a fresh
    handle.  In the bf16 training mode those fp32 bars do not apply; the bar is the one test_bf16_training_mode applies (10 % in
    the L2 sense) -- the sharp check of that mode is the bit-equality of outputs and input gradients above;
  * the discriminator's refresh folds weight norm in float, the host in double: images agree to rounding, not bitwise.  B is held
    to the float64 oracle under the bars of test_discriminator_forward / _backward, and |B - A| is bounded per element (DISC_TAU)."""
import ctypes as C

import pytest
import torch

from conftest import rel_err, report
from oracle import ref_cpu
from test_gpu_parity import assert_close_to_truth, cpu_sd, randomise

pytestmark = pytest.mark.gpu

DMEL_EMISSING = -3
PRECISIONS = ("fp32", "fp32_bf16x3", "fp32_f16x2", "fp32_mfma", "bf16")      # w48 (or the fused kernel / w32h), w48, w32h, w, w16
# (forward precision, train precision) of forward_train + backward: the training images are read as w48 (and w32h by the conditioned
# forward), as w, and as w16
TRAIN_MODES = (("fp32", "fp32"), ("fp32_mfma", "fp32"), ("fp32", "bf16"))
BF16_L2 = 0.1                    # test_bf16_training_mode's bar on a gradient of the bf16 training mode, relative L2 distance from fp32 / fp64

# Discriminator, per element: |B - A| <= DISC_TAU * A_scale, A_scale = the float64 discriminator on |x| with |g|, |v|, |bias|.
# The yardstick is route A's own rounding level, max |A - float64| / A_scale, measured on the MI355X over this module's cases:
# 7.5e-16 at (1, 80, 12), 2.1e-16 at (2, 80, 37) (max |B - A| / A_scale measured next to them: 3.0e-16 and 9.3e-17; A_scale of a six-layer
# stack without cancellation is ~1e9 times the logits).  DISC_TAU is 4x that level, rounded up -- the margin
# test_gpu_conv_matrix.py keeps between a measured maximum and its bound -- under that module's ceiling.
DISC_TAU = 3e-15
TAU_CEIL = 2.0 ** -16
assert DISC_TAU <= TAU_CEIL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def lib():
    from dmel_codec_amd import _lib
    return _lib.lib()


def last_error():
    return lib().dmel_last_error().decode(errors="replace")


class Findings:
    """Collects every failed comparison of a test before failing it: one run shows which images, precisions and quantities differ."""

    def __init__(self):
        self.bad = []

    def equal(self, what, a, b):
        if a.shape != b.shape or not torch.equal(a, b):
            n = int((a != b).sum()) if a.shape == b.shape else -1
            d = float((a.double() - b.double()).abs().max()) if a.shape == b.shape else float("nan")
            self.bad.append(f"{what}: not bit-equal ({n} of {a.numel()} elements, max |diff| {d:.3e}, max |value| {float(a.abs().max()):.3e})")

    def below(self, what, value, bound):
        if not value < bound:
            self.bad.append(f"{what}: {value:.3e} is not below {bound:.3e}")

    def done(self):
        assert not self.bad, f"{len(self.bad)} findings:\n" + "\n".join(self.bad)


def l2_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build_handle(m):
    with torch.cuda.device(m._device()):
        return m.native()


def refresh_to(m, redraw):
    """Route B: m holds W1.  Pack its handle on the host, redraw the parameters in place (W2), re-pack once on the device."""
    h, gen = build_handle(m), m._generation
    with torch.no_grad():
        redraw(m)
    assert build_handle(m) == h and m._generation == gen + 1, "the parameters were not re-packed on the device (handle rebuilt?)"
    return h, m._generation


def assert_not_repacked_since(m, state):
    assert (m._handle, m._generation) == state, "the handle was rebuilt or refreshed again: the comparison no longer tests ONE refresh"


def compare_routes(f, a, a2, b, pgrads_a, pgrads_a2):
    """a, a2: two rebuilds; b: the refreshed handle.  Dicts name -> tensor of outputs and input gradients (a, a2, b) and of parameter
    gradients.  Returns how many parameter gradients differ between the two rebuilds."""
    for k in a:
        # control: a rebuild is deterministic in every output and input gradient (no atomics on these paths) ...
        f.equal(f"CONTROL, two rebuilds: {k}", a[k], a2[k])
        # ... so the refreshed handle owes the same bits
        f.equal(f"refresh vs rebuild: {k}", b[k], a[k])
    # Parameter gradients are not compared with each other: the weight- and bias-gradient kernels accumulate with atomics, and a gradient
    # that comes out torch.equal from two rebuilds in one run (most WaveNet ones do) differs in the last bit in the next (measured: bias and
    # LayerNorm gradients equal between two rebuilds and 1 ulp off in the third handle).  The callers hold each route to float64.
    return sum(not torch.equal(pgrads_a[k], pgrads_a2[k]) for k in pgrads_a)


# ==================================================================================================== WaveNet
WAVENETS = {
    # fused whole-stack kernel at the default precision (T <= 96), layered kernels otherwise; 70 channels: no multiple of 16
    "encoder": (dict(input_channels=10, residual_channels=70, residual_layers=5, dilation_cycle=4), 6, 93),
    "encoder, layered": (dict(input_channels=10, residual_channels=70, residual_layers=3, dilation_cycle=4), 2, 130),
    # two-segment GATE recipe (dilated conv + condition), output projection; 48 channels: a multiple of 16, not of 32
    "decoder": (dict(input_channels=48, output_channels=20, residual_channels=48, residual_layers=4, dilation_cycle=4,
                     condition_channels=48), 3, 61),
    "no projections": (dict(residual_channels=64, residual_layers=3, dilation_cycle=2), 2, 130),
    # the gate's SECOND segment ends in a partial K step: 24 condition channels, no multiple of 16
    "ragged condition": (dict(input_channels=10, residual_channels=48, residual_layers=2, dilation_cycle=2, condition_channels=24), 2, 40),
    "real decoder widths": (dict(input_channels=560, output_channels=80, residual_channels=560, residual_layers=2, dilation_cycle=4,
                                 condition_channels=560), 2, 92),
}


def make_wavenet(cfg, seed, dev):
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    torch.manual_seed(seed)
    m = WaveNet(**cfg)
    randomise(m, seed)
    m = m.to(dev)
    m._want_train = True          # the training images are packed with the first handle: the one refresh has to rewrite them too
    return m


def wavenet_run(m, x, cond, lens, gy):
    """Everything a WaveNet handle computes: inference at the five precisions, plain and with ragged lengths, and forward_train + backward
    in the three training modes.  Returns (outputs and input gradients, parameter gradients), keyed by quantity and mode."""
    out, pg = {}, {}
    for prec in PRECISIONS:
        m.set_precision(prec)
        with torch.no_grad():
            out[f"forward [{prec}]"] = m(x, condition=cond)
            out[f"forward, ragged lengths [{prec}]"] = m(x, condition=cond, in_lengths=lens, out_lengths=lens)
    trained = m._trained_parameters()
    for prec, tprec in TRAIN_MODES:
        m.set_precision(prec)
        m.set_train_precision(tprec)
        tag = f"[{prec} / train {tprec}]"
        xd = x.clone().requires_grad_()
        cd = cond.clone().requires_grad_() if cond is not None else None
        y = m(xd, condition=cd)
        grads = torch.autograd.grad((y * gy).sum(), [xd] + ([cd] if cd is not None else []) + [p for _, p in trained])
        out[f"forward_train {tag}"] = y.detach()
        out[f"dx {tag}"] = grads[0]
        if cd is not None:
            out[f"d condition {tag}"] = grads[1]
        for (k, _), g in zip(trained, grads[1 + (cd is not None):]):
            pg[f"d {k} {tag}"] = g.clone()
    m.set_precision("fp32")
    m.set_train_precision("fp32")
    return out, pg


@pytest.mark.parametrize("name", list(WAVENETS))
def test_wavenet_refresh_equals_rebuild(dev, name):
    """dmel_wavenet_refresh: every forward image (GATE / RESSKIP paired row maps, one and two segments, the fused kernel's table) and every
    training image (pre_lin, out_lin, and the transposed pre_dx with reversed taps, pre_dc, out_dz, in_dx, skip_dx, out_dx), in all four
    number formats."""
    cfg, N, T = WAVENETS[name]
    seed = 100 + T
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cfg.get("input_channels") or cfg["residual_channels"], T, generator=g)
    cond = torch.randn(N, cfg["condition_channels"], T, generator=g) if cfg.get("condition_channels") else None
    gy = torch.randn(N, cfg.get("output_channels") or cfg["residual_channels"], T, generator=g).to(dev)
    lens = torch.tensor(([T, 0, T // 2 + 1, 1, T - 1, T // 3])[:N], device=dev)          # ragged, with an empty item

    a, a2 = make_wavenet(cfg, seed + 2, dev), make_wavenet(cfg, seed + 2, dev)             # W2, through the host, twice
    b = make_wavenet(cfg, seed + 1, dev)                                                   # W1 ...
    state = refresh_to(b, lambda m: randomise(m, seed + 2))                                # ... re-packed to W2
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert not any(torch.equal(p, q) for p, q in zip(make_wavenet(cfg, seed + 1, dev).parameters(), b.parameters()))

    xd, cd = x.to(dev), cond.to(dev) if cond is not None else None
    out_a, pg_a = wavenet_run(a, xd, cd, lens, gy)
    out_a2, pg_a2 = wavenet_run(a2, xd, cd, lens, gy)
    out_b, pg_b = wavenet_run(b, xd, cd, lens, gy)
    assert_not_repacked_since(b, state)

    f = Findings()
    loose = compare_routes(f, out_a, out_a2, out_b, pg_a, pg_a2)
    # float64 autograd through the oracle at W2
    sd64 = {k: v.double().requires_grad_() for k, v in cpu_sd(a).items()}
    x64 = x.double().requires_grad_()
    c64 = cond.double().requires_grad_() if cond is not None else None
    y64 = ref_cpu.wavenet_forward(sd64, "", x64, cfg["residual_layers"], cfg["dilation_cycle"] or 0, c64)
    (y64 * gy.cpu().double()).sum().backward()
    for route, out, pg in (("rebuild", out_a, pg_a), ("refresh", out_b, pg_b)):
        for prec, tprec in TRAIN_MODES:
            tag = f"[{prec} / train {tprec}]"
            if tprec == "fp32":          # bars of test_wavenet_training_forward_backward
                f.below(f"{route}: forward_train {tag} vs float64", rel_err(out[f"forward_train {tag}"], y64), 2e-5)
                f.below(f"{route}: dx {tag} vs float64", rel_err(out[f"dx {tag}"], x64.grad), 2e-5)
                if cond is not None:
                    f.below(f"{route}: d condition {tag} vs float64", rel_err(out[f"d condition {tag}"], c64.grad), 2e-5)
            for k, _ in a._trained_parameters():
                if tprec == "fp32":
                    f.below(f"{route}: d {k} {tag} vs float64", rel_err(pg[f"d {k} {tag}"], sd64[k].grad), 2e-5)
                else:
                    f.below(f"{route}: d {k} {tag} vs float64, L2", l2_err(pg[f"d {k} {tag}"], sd64[k].grad), BF16_L2)
    report(f"[repack] wavenet '{name}': {len(out_a)} outputs / input gradients bit-equal between refresh and rebuild; "
           f"{loose} of {len(pg_a)} parameter gradients differ between two rebuilds (atomics)")
    f.done()


def f32_from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def edge_weight_rows():
    """Rows of weight values at the edges of the three roundings (bf16 RNE, bf16 truncation split, fp16 pieces of 64 w), one class per row:
    a row's output then has its class's own scale, and a wrong piece is not hidden under a larger term."""
    below_max = torch.nextafter(torch.tensor(1023.5), torch.tensor(0.0)).item()      # largest w with 64 w < 65504
    assert below_max * 64 < 65504 and below_max == 1023.5 - 2.0 ** -14
    rows = {
        "zeros": [0.0, -0.0],
        # bf16 RNE ties: low half exactly 0x8000 under an even (round down) and an odd (round up) upper half, both signs; and their neighbours
        "bf16 ties": f32_from_bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
                                    0x3EFF8000, 0xBEFE8000]).tolist(),
        # exactly a bf16 value: second and third piece zero; and two pieces exact, third zero
        "bf16 exact": f32_from_bits([0x3F800000, 0xBF000000, 0x3E990000, 0xBE990000, 0x3F7F0000]).tolist() + [1.0 + 2.0 ** -15, -(0.5 + 2.0 ** -14)],
        # 64 w is an fp16 subnormal (below 2^-14): the smallest one, a tie that rounds to zero, one that rounds up to the smallest, the largest
        "fp16 subnormal": [2.0 ** -30, -2.0 ** -30, 2.0 ** -31, 1.5 * 2.0 ** -31, -3.0 * 2.0 ** -31, 2.0 ** -22, 1.25 * 2.0 ** -23,
                           (2.0 ** -14 - 2.0 ** -24) / 64, -(2.0 ** -14 - 2.0 ** -24) / 64],
        # low fp16 piece zero (64 w exact in fp16) or subnormal ((64 w - hi) 2^11 below 2^-14)
        "fp16 low piece": [0.5, -0.25, 2.0 ** -9, 2.0 ** -9 + 2.0 ** -32, -(2.0 ** -9 + 2.0 ** -32), 2.0 ** -9 + 3 * 2.0 ** -32,
                           2.0 ** -7 + 2.0 ** -30, 2.0 ** -12 + 2.0 ** -33],
        "fp16 range": [below_max, -below_max, 1023.0, -512.25],
    }
    for k, v in rows.items():
        t = torch.tensor(v, dtype=torch.float64)
        assert torch.isfinite(t).all() and torch.equal(t.float().double(), t), k          # every value is exactly an fp32 number
        assert float(t.abs().max()) * 64 < 65504, k
    return rows


def test_refresh_at_the_edges_of_the_three_roundings(dev):
    """The rounding code of the four images is written twice, on the host (conv.h) and on the device (repack_unit).  One small plain
    WaveNet whose last convolution (skip_projection: its rows ARE the output) carries one class of edge values per row, with a band of
    the small classes in the first gated convolution as well; no NaN or Inf, and 64 |w| stays below 65504."""
    cfg = dict(residual_channels=32, residual_layers=2, dilation_cycle=2)
    N, T = 2, 40
    rows = edge_weight_rows()

    def redraw(m):
        randomise(m, 72)
        w = m.skip_projection.conv.weight               # (C, C, 1)
        for r, vals in enumerate(rows.values()):
            for rr in (r, r + 16):                      # both 16-row halves of the 32-row tile
                w[rr, :, 0] = torch.tensor([vals[(c + rr) % len(vals)] for c in range(w.shape[1])])
                m.skip_projection.conv.bias[rr] = 0.0
        band = [v for k in ("zeros", "bf16 ties", "bf16 exact", "fp16 subnormal", "fp16 low piece") for v in rows[k]]
        cw = m.residual_layers[0].conv_layer.conv.weight     # (2C, C, 3)
        cw.view(-1)[200:200 + 20 * len(band)] = torch.tensor(band * 20)

    a = make_wavenet(cfg, 71, dev)
    with torch.no_grad():
        redraw(a)
    b = make_wavenet(cfg, 71, dev)
    state = refresh_to(b, redraw)
    w = b.skip_projection.conv.weight.detach().cpu()
    assert torch.equal(w[0, :2, 0].view(torch.int32), torch.tensor([0.0, -0.0]).view(torch.int32))      # the sign of zero arrived
    x = torch.randn(N, 32, T, generator=torch.Generator().manual_seed(9)).to(dev)
    f = Findings()
    for prec in PRECISIONS:
        a.set_precision(prec)
        b.set_precision(prec)
        with torch.no_grad():
            ya, yb = a(x), b(x)
        assert torch.isfinite(ya).all()
        # rows keep their class's own scale: +-0 weights and no bias give zeros, the fp16-subnormal row (|w| < 2^-20) stays tiny
        assert float(ya[:, 0].abs().max()) == 0 and 0 < float(ya[:, 3].abs().max()) < 1e-3 < float(ya[:, 1].abs().max())
        f.equal(f"edge values, forward [{prec}]", yb, ya)
    assert_not_repacked_since(b, state)
    f.done()


# ==================================================================================================== quantiser
def make_quantizer(levels, prebound, G, seed, dev, Cg=70):
    from dmel_codec_amd.models.modules.dowmsample_fsq import DownsampleFiniteScalarQuantize
    torch.manual_seed(seed)
    q = DownsampleFiniteScalarQuantize(input_dim=Cg * G, n_codebooks=1, n_groups=G, levels=levels, downsample_factor=[2, 2], is_dmel=True,
                                       fsq_prebound=prebound)
    with torch.no_grad():
        redraw_quantizer(q, seed)
    q = q.to(dev)
    q._want_train = True
    return q


def redraw_quantizer(q, seed):
    randomise(q, seed, scale=1.5)
    g = torch.Generator().manual_seed(seed + 5000)
    for name, p in q.named_parameters():
        if name.endswith("gamma"):
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)          # O(0.3): the ConvNeXt branches matter


def quantizer_run(q, z, gz):
    out, pg = {}, {}
    with torch.no_grad():
        ids = q.encode(z)
        out["encode"], out["decode"] = ids, q.decode(ids)
    names = [k for k, _ in q.named_parameters()]
    for tprec in ("fp32", "bf16"):
        q.set_train_precision(tprec)
        zd = z.clone().requires_grad_()
        res = q(zd)
        grads = torch.autograd.grad((res.z * gz).sum(), [zd] + list(q.parameters()))
        out[f"z [train {tprec}]"], out[f"ids [train {tprec}]"], out[f"latents [train {tprec}]"] = res.z.detach(), res.codes, res.latents.detach()
        out[f"dz [train {tprec}]"] = grads[0]
        for k, g in zip(names, grads[1:]):
            pg[f"d {k} [train {tprec}]"] = g.clone()
    q.set_train_precision("fp32")
    return out, pg


@pytest.mark.parametrize("levels,prebound,G,T,B", [([7, 5, 5], True, 3, 93, 2), ([7, 5, 5], False, 2, 64, 3), ([8, 6], True, 2, 47, 2),
                                                   ([8, 6], False, 3, 52, 2)])
def test_quantizer_refresh_equals_rebuild(dev, levels, prebound, G, T, B):
    """dmel_quantizer_refresh: the two-segment `down`, the phase-major `up` with one bias per channel shared by the phases (bias_mod), the
    ConvNeXt pointwise pairs and their transposes pw1T / pw2T, down_dx (phase-major) and up_dx (two segments), and the parameter buffers
    that are plain copies (depthwise, LayerNorm, gamma, FSQ projections)."""
    quantizer_refresh_case(dev, levels, prebound, G, T, B, 70)


# dmel_quantizer_create accepts any channel count per group (it only asks input_dim % n_groups == 0), but with ONE channel the ConvNeXt
# LayerNorm is degenerate: the normalised value is identically 0, every gradient through it is exactly 0 in float64, and the relative
# bars below divide by that 0 (measured on the commit before the descriptions were unified: it fails there too, for that reason alone).
# Cg = 3 is the smallest odd count with a LayerNorm that normalises something, and no multiple of 16: the phase-major `up` / `down_dx`
# images hold 2 x 3 real rows in 2 x 32 packed ones.  T = 5: the two stride-2 stages admit 4 at the least, plus one (the trailing column
# is dropped on the way down and zero-padded on the way up).
@pytest.mark.parametrize("Cg", [3])
def test_quantizer_refresh_equals_rebuild_odd_group_width(dev, Cg):
    """The phase-major view (ps / pC, bias_mod) with padded rows at the smallest shapes: one item, five frames."""
    quantizer_refresh_case(dev, [7, 5, 5], True, 2, 5, 1, Cg)


def quantizer_refresh_case(dev, levels, prebound, G, T, B, Cg):
    seed = 300 + 10 * G + len(levels) + T
    a, a2 = make_quantizer(levels, prebound, G, seed + 2, dev, Cg), make_quantizer(levels, prebound, G, seed + 2, dev, Cg)
    b = make_quantizer(levels, prebound, G, seed + 1, dev, Cg)
    state = refresh_to(b, lambda q: redraw_quantizer(q, seed + 2))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    # as in test_quantizer_training_forward_backward: an input that keeps a 1e-4 margin to every quantisation boundary in the float64
    # oracle (at W2), so that ids must be EQUAL to the oracle's
    gen = torch.Generator().manual_seed(1000 * T + G)
    for attempt in range(20):
        z = torch.randn(B * G, Cg, T, generator=gen)
        sd64 = {k: v.double().requires_grad_() for k, v in cpu_sd(a).items()}
        z64 = z.double().requires_grad_()
        zq64, ids64, lat64 = ref_cpu.quantizer_forward(sd64, "", z64, G, levels, (2, 2), prebound)
        _, pre64 = ref_cpu.quantizer_encode({k: v.detach() for k, v in sd64.items()}, "", z.double(), G, levels, (2, 2), prebound,
                                            return_prequant=True)
        if float((pre64 - torch.floor(pre64) - 0.5).abs().min()) > 1e-4:
            break
    else:
        raise AssertionError("no input with a 1e-4 rounding margin in 20 draws")
    gz = torch.randn(B, Cg * G, T, generator=gen)
    (zq64 * gz.double()).sum().backward()
    zd, gzd = z.to(dev), gz.to(dev)
    out_a, pg_a = quantizer_run(a, zd, gzd)
    out_a2, pg_a2 = quantizer_run(a2, zd, gzd)
    out_b, pg_b = quantizer_run(b, zd, gzd)
    assert_not_repacked_since(b, state)
    f = Findings()
    loose = compare_routes(f, out_a, out_a2, out_b, pg_a, pg_a2)
    for route, out, pg in (("rebuild", out_a, pg_a), ("refresh", out_b, pg_b)):
        # bars of test_quantizer_training_forward_backward
        f.equal(f"{route}: ids vs float64 oracle", out["ids [train fp32]"].cpu(), ids64.cpu().to(out["ids [train fp32]"].dtype))
        f.below(f"{route}: latents vs float64", rel_err(out["latents [train fp32]"].reshape(lat64.shape), lat64), 2e-5)
        f.below(f"{route}: z vs float64", rel_err(out["z [train fp32]"], zq64), 5e-5)
        f.below(f"{route}: dz vs float64", rel_err(out["dz [train fp32]"], z64.grad), 1e-4)
        for k, _ in a.named_parameters():
            f.below(f"{route}: d {k} [train fp32] vs float64", rel_err(pg[f"d {k} [train fp32]"], sd64[k].grad), 2e-4)
    report(f"[repack] quantizer levels {levels} G {G} Cg {Cg}: {len(out_a)} outputs / input gradients bit-equal between refresh and rebuild; "
           f"{loose} of {len(pg_a)} parameter gradients differ between two rebuilds (atomics)")
    f.done()


# ==================================================================================================== discriminator
def discriminator_sd(seed):
    """ref_cpu.seeded_discriminator_sd with g drawn from [0.5, 1.5): independent of v's norm, so the fold cannot pass for the identity."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (cin, cout, kw) in enumerate(ref_cpu.DISC_CONVS):
        p = f"blocks.{2 * i}."
        sd[p + "bias"] = torch.randn(cout, generator=gen) * 0.1
        sd[p + "parametrizations.weight.original0"] = torch.rand(cout, 1, 1, 1, generator=gen) + 0.5
        sd[p + "parametrizations.weight.original1"] = torch.randn(cout, cin, 3, kw, generator=gen) / (cin * 3 * kw) ** 0.5
    return sd


def make_discriminator(sd, dev):
    from dmel_codec_amd.models.modules.discriminator import Discriminator
    d = Discriminator()
    d.load_state_dict(sd)
    d = d.to(dev)
    d._want_train = True
    return d


def load_in_place(m, sd):
    for k, p in m.named_parameters():
        p.copy_(sd[k])


def discriminator_run(d, x, dy):
    out, pg = {}, {}
    with torch.no_grad():
        out["forward"] = d(x)
    names = [k for k, _ in d.named_parameters()]
    for tprec in ("fp32", "bf16"):
        d.set_train_precision(tprec)
        xd = x.clone().requires_grad_()
        y = d(xd)
        grads = torch.autograd.grad((y * dy).sum(), [xd] + list(d.parameters()))
        out[f"forward_train [train {tprec}]"], out[f"dx [train {tprec}]"] = y.detach(), grads[0]
        for k, g in zip(names, grads[1:]):
            pg[f"d {k} [train {tprec}]"] = g.clone()
    d.set_train_precision("fp32")
    return out, pg


def discriminator_truth(sd, x, dy):
    """float32 and float64 oracle outputs, float64 gradients, and A_scale (the float64 discriminator on |x| with |g|, |v|, |bias|)."""
    sd64 = {k: v.double().requires_grad_() for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    y64 = ref_cpu.discriminator_forward(sd64, "", x64)
    (y64 * dy.double()).sum().backward()
    y32 = ref_cpu.discriminator_forward(sd, "", x)
    scale = ref_cpu.discriminator_forward({k: v.double().abs() for k, v in sd.items()}, "", x.double().abs())
    return sd64, x64, y64.detach(), y32, scale


def check_discriminator_route(f, route, out, pg, names, sd64, x64, y64, y32):
    assert_close_to_truth(out["forward"], y32, y64, f"discriminator logits after {route}")          # test_discriminator_forward
    # bars of test_discriminator_backward
    f.below(f"{route}: forward_train vs float64", rel_err(out["forward_train [train fp32]"], y64), 1e-4)
    f.below(f"{route}: dx vs float64", rel_err(out["dx [train fp32]"], x64.grad), 1e-4)
    f.below(f"{route}: forward_train [train bf16] vs float64, L2", l2_err(out["forward_train [train bf16]"], y64), BF16_L2)
    f.below(f"{route}: dx [train bf16] vs float64, L2", l2_err(out["dx [train bf16]"], x64.grad), BF16_L2)
    for k in names:
        f.below(f"{route}: d {k} vs float64", rel_err(pg[f"d {k} [train fp32]"], sd64[k].grad), 2e-4)
        f.below(f"{route}: d {k} [train bf16] vs float64, L2", l2_err(pg[f"d {k} [train bf16]"], sd64[k].grad), BF16_L2)


def per_element(y, ref, scale):
    return float(((y.detach().double().cpu() - ref.detach().double().cpu()).abs() / scale.clamp_min(1e-300)).max())


# (1, 80, 12): the width falls to 6, 3, 2 -- below the nine taps of the strided layers; (2, 80, 37): ragged widths 37 -> 19 -> 10 -> 5
@pytest.mark.parametrize("B,H,W", [(1, 80, 12), (2, 80, 37)])
def test_discriminator_refresh_matches_oracle_and_rebuild(dev, B, H, W):
    """dmel_discriminator_refresh: the weight-norm fold on the device, three row-taps per layer, two strided K segments of the stride-2
    layers forward, and backward images with reversed taps (stride 1) or negative tap stride per output phase (stride 2)."""
    w1, w2 = ref_cpu.seeded_discriminator_sd(900 + W), discriminator_sd(901 + W)
    g = torch.Generator().manual_seed(W)
    x = torch.randn(B, H, W, generator=g)
    a = make_discriminator(w2, dev)
    b = make_discriminator(w1, dev)
    state = refresh_to(b, lambda d: load_in_place(d, w2))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    with torch.no_grad():
        dy = torch.randn(a(x.to(dev)).shape, generator=g)
    out_a, pg_a = discriminator_run(a, x.to(dev), dy.to(dev))
    out_b, pg_b = discriminator_run(b, x.to(dev), dy.to(dev))
    assert_not_repacked_since(b, state)
    sd64, x64, y64, y32, scale = discriminator_truth(w2, x, dy)
    names = [k for k, _ in a.named_parameters()]
    f = Findings()
    check_discriminator_route(f, "refresh", out_b, pg_b, names, sd64, x64, y64, y32)
    check_discriminator_route(f, "rebuild", out_a, pg_a, names, sd64, x64, y64, y32)
    for k in ("forward", "forward_train [train fp32]"):
        level, diff = per_element(out_a[k], y64, scale), per_element(out_b[k], out_a[k], scale)
        report(f"[repack] discriminator ({B}, {H}, {W}) {k}: max |refresh - rebuild| / A_scale = {diff:.3e}; the rebuild's own "
               f"max |rebuild - float64| / A_scale = {level:.3e}  (DISC_TAU {DISC_TAU:.1e}, ceiling 2^-16 = {TAU_CEIL:.2e})")
        f.below(f"refresh vs rebuild, per element: {k}", diff, DISC_TAU)
    for k in ("forward_train [train bf16]", "dx [train fp32]", "dx [train bf16]"):          # on record only
        report(f"[repack] discriminator ({B}, {H}, {W}) {k}: refresh vs rebuild, max|diff| / max|value| = {rel_err(out_b[k], out_a[k]):.3e}")
    f.done()


# ==================================================================================================== launch machinery
def tiny_wavenet(seed, dev):
    return make_wavenet(dict(residual_channels=16, residual_layers=1, dilation_cycle=1), seed, dev)


def test_refresh_after_the_job_table_cache_evicted_its_table(dev):
    """RepackBatchState keeps the device copies of 64 job tables per thread; the 65th distinct table evicts the oldest (after a stream
    sync).  More than 64 distinct WaveNets are refreshed on one thread and stream, then the first one again, to new values: its table
    has to be uploaded anew, and the result must equal a rebuild.  All handles stay alive: their addresses, hence tables, are distinct."""
    x = torch.randn(2, 16, 24, generator=torch.Generator().manual_seed(1)).to(dev)
    nets = [tiny_wavenet(1000 + i, dev) for i in range(70)]
    for i, m in enumerate(nets):
        refresh_to(m, lambda mm: randomise(mm, 2000 + i))
    assert len({m._handle for m in nets}) == len(nets)
    first = nets[0]
    state = refresh_to(first, lambda mm: randomise(mm, 3000))
    fresh = tiny_wavenet(3000, dev)
    f = Findings()
    with torch.no_grad():
        f.equal("first handle, refreshed again after eviction", first(x), fresh(x))
        # the others still hold what their own refresh wrote
        for i in (1, 5, 64, 69):
            f.equal(f"handle {i} after the eviction", nets[i](x), tiny_wavenet(2000 + i, dev)(x))
    xd = x.clone().requires_grad_()
    xf = x.clone().requires_grad_()
    first(xd).sum().backward()
    fresh(xf).sum().backward()
    f.equal("first handle, dx", xd.grad, xf.grad)
    assert_not_repacked_since(first, state)
    f.done()


def test_refresh_on_a_second_stream(dev):
    """The job table cache is keyed by stream as well: the same handle refreshed on a non-default stream uploads its own table there.
    Refresh and forward both run under that stream."""
    cfg = dict(input_channels=10, residual_channels=48, residual_layers=3, dilation_cycle=2)
    x = torch.randn(3, 10, 130, generator=torch.Generator().manual_seed(2)).to(dev)
    m = make_wavenet(cfg, 41, dev)
    refresh_to(m, lambda mm: randomise(mm, 42))          # default stream first: a cached table for that stream exists
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        state = refresh_to(m, lambda mm: randomise(mm, 43))
        with torch.no_grad():
            y = m(x)
        xd = x.clone().requires_grad_()
        m(xd).sum().backward()
    side.synchronize()
    assert_not_repacked_since(m, state)
    fresh = make_wavenet(cfg, 43, dev)
    with torch.no_grad():
        assert torch.equal(y, fresh(x))
    xf = x.clone().requires_grad_()
    fresh(xf).sum().backward()
    assert torch.equal(xd.grad, xf.grad)


def call_refresh(m, tensors, leave_out=None):
    """dmel_*_refresh through the C ABI with chosen keys: `tensors` key -> device tensor, minus `leave_out`."""
    from dmel_codec_amd import _lib
    items = [(k, v) for k, v in tensors.items() if k != leave_out]
    keys = (C.c_char_p * len(items))(*[k.encode() for k, _ in items])
    ptrs = (C.c_void_p * len(items))(*[v.data_ptr() for _, v in items])
    with torch.cuda.device(m._device()):
        return getattr(lib(), m._refresh_symbol)(m._handle, len(items), keys, ptrs, _lib.stream_ptr())


def refused_then_complete(m, tensors, leave_out, forward):
    """A refresh with one required key left out is refused as a whole: DMEL_EMISSING, the key by name, the handle untouched.  The complete
    refresh that follows works.  `tensors` are NOT the module's parameters: the mirror sees no change and never refreshes by itself."""
    build_handle(m)
    y0 = forward(m)
    state = (m._handle, m._generation)
    assert leave_out in tensors
    rc = call_refresh(m, tensors, leave_out)
    assert rc == DMEL_EMISSING, (rc, last_error())
    assert leave_out in last_error(), last_error()
    torch.cuda.synchronize()
    y1 = forward(m)
    assert (m._handle, m._generation) == state
    assert torch.equal(y1, y0), (f"a refused refresh changed the handle: {int((y1 != y0).sum())} of {y0.numel()} outputs differ, "
                                 f"max |diff| {float((y1 - y0).abs().max()):.3e}")
    rc = call_refresh(m, tensors)
    assert rc == 0, (rc, last_error())
    y2 = forward(m)
    assert (m._handle, m._generation) == state
    assert not torch.equal(y2, y0)
    return y2


def test_refused_wavenet_refresh_leaves_the_handle_unchanged(dev):
    cfg = dict(input_channels=10, residual_channels=48, residual_layers=3, dilation_cycle=2)
    x = torch.randn(3, 10, 130, generator=torch.Generator().manual_seed(3)).to(dev)
    m, target = make_wavenet(cfg, 51, dev), make_wavenet(cfg, 52, dev)
    tensors = {k: target.state_dict()[k].detach().clone() for k, _ in m._native_state_refs()}

    def forward(mm):
        with torch.no_grad():
            return mm(x)

    y2 = refused_then_complete(m, tensors, "skip_projection.conv.bias", forward)
    assert torch.equal(y2, forward(target))
    xd, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    m(xd).sum().backward()
    target(xt).sum().backward()
    assert torch.equal(xd.grad, xt.grad)


def test_refused_quantizer_refresh_leaves_the_handle_unchanged(dev):
    G, levels = 2, [7, 5, 5]
    z = torch.randn(2 * G, 70, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    q, target = make_quantizer(levels, True, G, 61, dev), make_quantizer(levels, True, G, 62, dev)
    tensors = {k: target.state_dict()[k].detach().clone() for k, _ in q._native_state_refs()}

    def forward(qq):
        with torch.no_grad():
            res = qq(z)
            return torch.cat([res.z.reshape(-1), res.latents.reshape(-1), qq.decode(res.codes).reshape(-1)])

    # the last key the refresh looks at: every buffer copy and every re-pack of the blocks in front of it used to be done by then
    y2 = refused_then_complete(q, tensors, f"residual_fsq.rvqs.{G - 1}.project_out.bias", forward)
    assert torch.equal(y2, forward(target))
    with torch.no_grad():
        assert torch.equal(q(z).codes, target(z).codes)
    # an early key as well
    q2 = make_quantizer(levels, True, G, 61, dev)
    refused_then_complete(q2, tensors, "upsample.0.1.gamma", forward)


def test_refused_discriminator_refresh_leaves_the_handle_unchanged(dev):
    B, H, W = 2, 80, 37
    w2 = discriminator_sd(72)
    x = torch.randn(B, H, W, generator=torch.Generator().manual_seed(5))
    d, target = make_discriminator(ref_cpu.seeded_discriminator_sd(71), dev), make_discriminator(w2, dev)
    tensors = {k: target.state_dict()[k].detach().clone() for k, _ in d._native_state_refs()}
    assert len(tensors) == 18

    def forward(dd):
        with torch.no_grad():
            return dd(x.to(dev))

    # the last layer's bias: the five layers in front of it used to be flushed by the time it was missed
    y2 = refused_then_complete(d, tensors, "blocks.10.bias", forward)
    # equal to a rebuild as far as the float fold allows: the oracle's bar, and the per-element bound of the refresh test
    y64 = ref_cpu.discriminator_forward({k: v.double() for k, v in w2.items()}, "", x.double())
    scale = ref_cpu.discriminator_forward({k: v.double().abs() for k, v in w2.items()}, "", x.double().abs())
    assert_close_to_truth(y2, ref_cpu.discriminator_forward(w2, "", x), y64, "discriminator logits after a refused, then a complete refresh")
    assert per_element(y2, forward(target), scale) < DISC_TAU


# ==================================================================================================== launch counts
def kernel_launches(fn):
    """Names of the device kernels launched while fn runs (the library keeps no profile record for the re-pack: the profiler's trace)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_refresh_launch_counts(dev):
    """One refresh is ONE repack launch for a WaveNet, one (next to its plain copies) for the quantiser, and one weight-norm fold launch
    plus one repack launch for each of the discriminator's six layers."""
    m = make_wavenet(WAVENETS["decoder"][0], 81, dev)
    q = make_quantizer([7, 5, 5], True, 2, 82, dev)
    d = make_discriminator(ref_cpu.seeded_discriminator_sd(83), dev)
    w2 = discriminator_sd(84)
    counts = {}
    for name, mod, redraw in (("wavenet", m, lambda mm: randomise(mm, 91)), ("quantizer", q, lambda qq: redraw_quantizer(qq, 92)),
                              ("discriminator", d, lambda dd: load_in_place(dd, w2))):
        refresh_to(mod, redraw)                      # the first refresh uploads the job tables; the counted one finds them cached
        with torch.no_grad():
            redraw(mod)
        h, gen = mod._handle, mod._generation
        names = kernel_launches(lambda: build_handle(mod))
        assert (mod._handle, mod._generation) == (h, gen + 1)
        counts[name] = (sum("repack_kernel" in k for k in names), sum("weight_norm_fwd_kernel" in k for k in names))
        report(f"[repack] {name}: one refresh launched {counts[name][0]} repack and {counts[name][1]} fold kernels ({len(names)} device kernels in all)")
    assert counts == {"wavenet": (1, 0), "quantizer": (1, 0), "discriminator": (6, 6)}, counts
