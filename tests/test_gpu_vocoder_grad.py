"""Input gradient through the frozen BigVGAN (dmel_bigvgan_forward_train / dmel_bigvgan_backward_input) on the GPU: every new kernel
against float64 autograd on the CPU, the whole generator against float64 autograd through oracle.ref_cpu.bigvgan_forward, and the
multi-resolution STFT loss back-propagated through the vocoder to the mel.

Bars: single ops rel_err < 2e-5 (the bar test_gpu_train.py puts on conv1d_dilated's gradients); whole networks
e_gpu < max(1e-4, 3 * e_ref) with e_ref the fp32 oracle's own distance from float64 (the project's gradient criterion; 1.5 * e_ref
for the generator alone, where every recorded case stays under e_ref).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, report
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    import dmel_codec_amd.torch_ops  # noqa: F401
    return torch.ops.dmel_hip


def cpu_sd(module):
    return {k: v.detach().cpu().float() for k, v in module.state_dict().items()}


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def randomise(module, seed, scale=1.0):
    """O(1) weights so every term of the arithmetic matters (the recipe of test_gpu_parity.py)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.split(".")[-1]
            if leaf in ("alpha", "beta"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif leaf == "gamma":
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
            elif leaf == "weight_g":
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.ndim >= 2:
                p.copy_(torch.randn(p.shape, generator=g) * (scale / p[0].numel() ** 0.5))
            elif leaf == "weight":
                p.copy_(1.0 + torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)


# ------------------------------------------------------------------------------------ single ops
CONVT_CASES = [(8, 40, 24, 37), (2, 16, 8, 101), (4, 70, 33, 5)]                      # the cases of the forward's op test
CONVT_CASES += [(u, ci, co, T) for (u, ci, co) in ((8, 512, 256), (8, 256, 128), (2, 128, 64), (2, 64, 32)) for T in (1, 7, 94)]


@pytest.mark.parametrize("stride,Ci,Co,T", CONVT_CASES)
def test_conv_transpose1d_input_gradient(dev, ops, stride, Ci, Co, T):
    g = torch.Generator().manual_seed(1000 * stride + Ci + T)
    w, b = torch.randn(Ci, Co, 2 * stride, generator=g) / (Ci * 2) ** 0.5, torch.randn(Co, generator=g) * 0.1
    x = torch.randn(2, Ci, T, generator=g)
    dy = torch.randn(2, Co, T * stride, generator=g)
    x64 = x.double().requires_grad_()
    (F.conv_transpose1d(x64, w.double(), b.double(), stride=stride, padding=stride // 2) * dy.double()).sum().backward()
    xd = x.to(dev).requires_grad_()
    y = ops.conv_transpose1d(xd, w.to(dev), b.to(dev), stride)
    assert y.grad_fn is not None
    (y * dy.to(dev)).sum().backward()
    e = rel_err(xd.grad, x64.grad)
    report(f"conv_transpose1d dgrad stride {stride} {Ci}->{Co} T {T}: gpu-vs-fp64 {e:.2e}")
    assert xd.grad.shape == x.shape and e < 2e-5, e


def test_conv_transpose1d_weight_gradient_is_refused(dev, ops):
    w = torch.randn(16, 8, 4, device=dev, requires_grad=True)
    x = torch.randn(1, 16, 9, device=dev, requires_grad=True)
    y = ops.conv_transpose1d(x, w, None, 2)             # the forward itself behaves as before
    with pytest.raises(NotImplementedError, match="frozen"):
        y.sum().backward()
    wp = torch.randn(1, 8, 7, device=dev, requires_grad=True)
    yp = ops.conv_post(torch.randn(1, 8, 50, device=dev, requires_grad=True), wp, 0.0, "tanh")
    with pytest.raises(NotImplementedError, match="frozen"):
        yp.sum().backward()


@pytest.mark.parametrize("act", ["none", "tanh", "clamp"])
def test_conv_post_input_gradient(dev, ops, act):
    # seed 12: in float64 no pre-activation of the clamp case lies within 7e-3 of +-1 (asserted below at 1e-3; most seeds have one closer)
    g = torch.Generator().manual_seed(12)
    w, x = torch.randn(1, 32, 7, generator=g) * 0.05, torch.randn(3, 32, 500, generator=g)
    scale = 4.0 if act == "clamp" else 1.0             # as in the forward's op test: pushes part of the samples past the clamp
    bias = 0.3 * scale
    dy = torch.randn(3, 1, 500, generator=g)
    fn = {"none": lambda v: v, "tanh": torch.tanh, "clamp": lambda v: v.clamp(-1, 1)}[act]
    x64 = (x.double() * scale).requires_grad_()
    pre = F.conv1d(x64, w.double(), torch.tensor([bias], dtype=torch.float64), padding=3)
    if act == "clamp":
        # the derivative AT +-1 is a convention, not arithmetic: keep every sample away from it, and have both kinds of sample
        assert float((pre.detach().abs() - 1).abs().min()) > 1e-3
        assert bool((pre.detach().abs() > 1).any()) and bool((pre.detach().abs() < 1).any())
    (fn(pre) * dy.double()).sum().backward()
    xd = (x.to(dev) * scale).requires_grad_()
    y = ops.conv_post(xd, w.to(dev), bias, act)
    (y * dy.to(dev)).sum().backward()
    e = rel_err(xd.grad, x64.grad)
    report(f"conv_post dgrad {act}: gpu-vs-fp64 {e:.2e}")
    assert e < 2e-5, e


def test_parameter_free_activation_backward(dev, ops, golden):
    """dx of the dx-only kernel is the full backward's dx bit for bit; with the additive input it is dx + r in fp32."""
    gd = golden("train_grads_activation1d")
    x, dy = gd.ins["x"].to(dev), gd.ins["dy"].to(dev)
    a, b = gd.sd["act.alpha"].to(dev), gd.sd["act.beta"].to(dev)
    up, dn = gd.sd["upsample.filter"], gd.sd["downsample.lowpass.filter"]
    for beta in (b, None):
        dx_full, _, _ = ops.aa_snake_backward(x, dy, a, beta, up, dn, True)
        dx = ops.aa_snake_backward_input(x, dy, None, a, beta, up, dn, True)
        assert torch.equal(dx, dx_full)
        r = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        dxr = ops.aa_snake_backward_input(x, dy, r, a, beta, up, dn, True)
        assert torch.equal(dxr.cpu(), dx_full.cpu() + r.cpu())
    assert rel_err(ops.aa_snake_backward_input(x, dy, None, a, b, up, dn, True), gd.outs["d_x"]) < 2e-5


# ------------------------------------------------------------------------------------ whole vocoder
def scale_conv_post(m, k=0.05):
    """As committed, the fixtures and the random base model saturate the output non-linearity (12-80 % of samples beyond 0.99), where
    the input gradient is mostly the derivative of a flat tanh / clamp: shrink conv_post on both sides of the comparison."""
    with torch.no_grad():
        cp = m.conv_post
        (cp.weight_g if hasattr(cp, "weight_g") else cp.weight).mul_(k)
        if getattr(cp, "bias", None) is not None:
            cp.bias.mul_(k)


def build_model(name, golden):
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.bigvgan.env import AttrDict
    from dmel_codec_amd.configs import bigvgan_h
    if name == "base":
        h = bigvgan_h("base_24k_100band", num_mels=80)
        torch.manual_seed(11)
        m = BigVGAN(h)
        randomise(m, 12, scale=0.7)
        mel = torch.randn(2, 80, 12)
    else:
        gd = golden(name)
        h = AttrDict(dict(gd.meta["h"]))
        m = BigVGAN(h)
        if name.endswith("nowm"):
            m.remove_weight_norm()
        m.load_state_dict(gd.sd)
        mel = gd.ins["mel"].clone()
    scale_conv_post(m)
    return m, h, mel


def oracle_grads(sd, h, mel, w):
    """(audio64, d mel in float64, d mel by fp32 autograd through the same oracle)."""
    m64 = mel.double().requires_grad_()
    y64 = ref_cpu.bigvgan_forward(to64(sd), dict(h), m64)
    assert float(y64.detach().abs().max()) < 0.9, "the reference saturates its output non-linearity: the comparison would show nothing"
    (y64 * w.double()).sum().backward()
    m32 = mel.clone().requires_grad_()
    (ref_cpu.bigvgan_forward(sd, dict(h), m32) * w).sum().backward()
    return y64.detach(), m64.grad, m32.grad


MODELS = ["bigvgan_tiny", "bigvgan_tiny_snake_nowm", "bigvgan_tiny_ampblock2", "base"]


@pytest.mark.parametrize("name", MODELS)
def test_vocoder_input_gradient(dev, golden, name):
    m, h, mel = build_model(name, golden)
    sd = cpu_sd(m)
    g = torch.Generator().manual_seed(77)
    up = 1
    for u in h.upsample_rates:
        up *= u
    w = torch.randn(mel.shape[0], 1, mel.shape[2] * up, generator=g)
    y64, g64, g32 = oracle_grads(sd, h, mel, w)
    m = m.to(dev)
    grads, audios = {}, {}
    for streams in (3, 1):
        m.set_streams(streams)
        with torch.no_grad():
            y_inf = m(mel.to(dev))
        assert m(mel.to(dev)).grad_fn is None                       # a mel that does not require grad: the inference path
        md = mel.to(dev).requires_grad_()
        y = m(md)
        assert y.grad_fn is not None
        assert torch.equal(y.detach(), y_inf), f"{name}: training forward and inference forward differ ({streams} streams)"
        (y * w.to(dev)).sum().backward()
        grads[streams], audios[streams] = md.grad.clone(), y.detach()
    assert torch.equal(audios[1], audios[3]) and torch.equal(grads[1], grads[3]), f"{name}: one stream and three give different bits"
    assert rel_err(audios[3], y64) < TOL
    e_gpu, e_ref = rel_err(grads[3], g64), rel_err(g32, g64)
    report(f"[vocoder input grad] {name}: gpu-vs-fp64 {e_gpu:.2e}, oracle-fp32-vs-fp64 {e_ref:.2e}, |y|max {float(y64.abs().max()):.2f}")
    # every recorded case has e_gpu < e_ref (4.1e-6 / 4.3e-6, 2.7e-6 / 3.1e-6, 1.8e-6 / 2.2e-6, 4.5e-5 / 5.0e-5), so the relief factor of
    # the project's gradient criterion is 1.5 here instead of 3, as in the forward's assert_close_to_truth
    assert e_gpu < max(TOL, 1.5 * e_ref), (e_gpu, e_ref)
    assert all(p.grad is None for p in m.parameters())              # frozen: parameters never receive a gradient


def test_two_forwards_before_one_backward(dev, golden):
    m, h, mel = build_model("bigvgan_tiny", golden)
    m = m.to(dev)
    g = torch.Generator().manual_seed(5)
    mel_a, mel_b = mel.to(dev), (mel + 0.3 * torch.randn(mel.shape, generator=g)).to(dev)
    w = torch.randn(mel.shape[0], 1, mel.shape[2] * 8, generator=g).to(dev)

    def alone(x):
        x = x.clone().requires_grad_()
        (m(x) * w).sum().backward()
        return x.grad

    ga, gb = alone(mel_a), alone(mel_b)
    xa, xb = mel_a.clone().requires_grad_(), mel_b.clone().requires_grad_()
    ya, yb = m(xa), m(xb)                     # both saved workspaces must survive until the single backward
    ((ya * w).sum() + (yb * w).sum()).backward()
    assert torch.equal(xa.grad, ga) and torch.equal(xb.grad, gb)
    # a retained graph can be back-propagated twice: the backward leaves the saved activations alone
    x = mel_a.clone().requires_grad_()
    y = m(x)
    (y * w).sum().backward(retain_graph=True)
    first = x.grad.clone()
    x.grad = None
    (y * w).sum().backward()
    assert torch.equal(x.grad, first) and torch.equal(first, ga)


def test_mrstft_lengths_shorter_than_a_hop(dev):
    """Items shorter than the hop of a resolution count no frame there: that resolution contributes zero, not nan."""
    from dmel_codec_amd.utils.mrstft import MultiResolutionSTFTLoss
    g = torch.Generator().manual_seed(2)
    pred = (torch.randn(2, 6000, generator=g) * 0.1).to(dev).requires_grad_()
    target = (torch.randn(2, 6000, generator=g) * 0.1).to(dev)
    sc, mag = MultiResolutionSTFTLoss()(pred, target, lengths=torch.tensor([100, 60], device=dev))      # hops 120, 240, 50
    (sc + mag).backward()
    assert bool(torch.isfinite(sc)) and bool(torch.isfinite(mag)) and bool(torch.isfinite(pred.grad).all())
    assert float(sc) > 0 and bool((pred.grad[:, 100:] == 0).all())


def test_vocoder_input_gradient_ragged_shape(dev, golden):
    """B = 3, T = 7: no tile of any launch is full."""
    m, h, _ = build_model("bigvgan_tiny", golden)
    g = torch.Generator().manual_seed(9)
    mel = torch.randn(3, h.num_mels, 7, generator=g)
    w = torch.randn(3, 1, 7 * 8, generator=g)
    y64, g64, g32 = oracle_grads(cpu_sd(m), h, mel, w)
    m = m.to(dev)
    md = mel.to(dev).requires_grad_()
    y = m(md)
    (y * w.to(dev)).sum().backward()
    e_gpu, e_ref = rel_err(md.grad, g64), rel_err(g32, g64)
    report(f"[vocoder input grad] bigvgan_tiny B 3 T 7: gpu-vs-fp64 {e_gpu:.2e}, oracle-fp32-vs-fp64 {e_ref:.2e}")
    assert rel_err(y, y64) < TOL and e_gpu < max(TOL, 1.5 * e_ref), (e_gpu, e_ref)


# ------------------------------------------------------------------------------------ waveform loss through the vocoder
RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def masked_mrstft64(pred, target, lengths):
    """float64 restatement of MultiResolutionSTFTLoss.forward(pred, target, lengths): samples at or behind lengths[b] zeroed on both
    sides, frame t of a resolution with hop h counted only if t < lengths[b] // h, both norms and the mean over counted entries."""
    keep = (torch.arange(pred.shape[1])[None, :] < lengths[:, None]).to(pred.dtype)
    pred, target = pred * keep, target * keep
    sc, mag = 0.0, 0.0
    for n_fft, hop, win in RES:
        sp, st = ref_cpu.stft_magnitude(pred, n_fft, win, hop), ref_cpu.stft_magnitude(target, n_fft, win, hop)     # (B, K, T)
        cnt = (torch.arange(sp.shape[2])[None, :] < (lengths // hop)[:, None])[:, None, :].expand_as(sp)
        sc = sc + torch.linalg.norm((st - sp)[cnt]) / torch.linalg.norm(st[cnt])
        mag = mag + (st[cnt].log() - sp[cnt].log()).abs().mean()
    return sc / len(RES), mag / len(RES)


def waveform_model(golden):
    """bigvgan_tiny (20 mels, x8) on 800 frames: 6400 samples, enough for every resolution of the loss."""
    m, h, _ = build_model("bigvgan_tiny", golden)
    g = torch.Generator().manual_seed(31)
    mel = torch.randn(2, h.num_mels, 800, generator=g)
    return m, h, mel, g


def test_mrstft_loss_through_the_vocoder(dev, golden):
    from dmel_codec_amd.utils.mrstft import MultiResolutionSTFTLoss
    m, h, mel, g = waveform_model(golden)
    sd = cpu_sd(m)
    with torch.no_grad():
        clean = ref_cpu.bigvgan_forward(sd, dict(h), mel + 0.2 * torch.randn(mel.shape, generator=g))[:, 0]
    target = clean + 0.01 * torch.randn(clean.shape, generator=g)

    def chain(dtype):
        x = mel.detach().clone().to(dtype).requires_grad_()
        s = to64(sd) if dtype == torch.float64 else sd
        y = ref_cpu.bigvgan_forward(s, dict(h), x)
        if dtype == torch.float64:
            assert float(y.detach().abs().max()) < 0.9
        sc, mag = ref_cpu.mrstft_loss(y[:, 0], target.to(dtype))
        (sc + mag).backward()
        return float((sc + mag).detach()), x.grad

    l64, g64 = chain(torch.float64)
    _, g32 = chain(torch.float32)
    m = m.to(dev)
    loss = MultiResolutionSTFTLoss()
    md = mel.to(dev).requires_grad_()
    sc, mag = loss(m(md), target.to(dev)[:, None, :])
    (sc + mag).backward()
    e_gpu, e_ref = rel_err(md.grad, g64), rel_err(g32, g64)
    report(f"[mrstft through vocoder] loss gpu {float(sc + mag):.6f} fp64 {l64:.6f}; d mel gpu-vs-fp64 {e_gpu:.2e}, oracle-fp32-vs-fp64 {e_ref:.2e}")
    assert abs(float(sc + mag) - l64) < 1e-4 * abs(l64)
    assert e_gpu < max(TOL, 3.0 * e_ref), (e_gpu, e_ref)
    # a dozen Adam steps on the mel itself lower the loss (the shape of test_mrstft_loss_trains_a_waveform)
    x = mel.to(dev).clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=2e-2)
    first = None
    for _ in range(12):
        opt.zero_grad()
        a, b = loss(m(x), target.to(dev)[:, None, :])
        (a + b).backward()
        opt.step()
        first = first if first is not None else float(a + b)
    report(f"[mrstft through vocoder] 12 Adam steps on the mel: loss {first:.4f} -> {float(a + b):.4f}")
    assert float(a + b) < first


def test_mrstft_lengths_on_a_right_padded_batch(dev, golden):
    from dmel_codec_amd.utils.mrstft import MultiResolutionSTFTLoss
    m, h, mel, g = waveform_model(golden)
    L = mel.shape[2] * 8
    lengths = torch.tensor([L, L // 2])
    mel[1, :, 400:] = 0.0                                    # the collated batch: item 1 is half as long, right-padded
    sd = cpu_sd(m)
    with torch.no_grad():
        target = ref_cpu.bigvgan_forward(sd, dict(h), mel + 0.2 * torch.randn(mel.shape, generator=g))[:, 0]
        target = target + 0.01 * torch.randn(target.shape, generator=g)
    target[1, L // 2:] = 0.0                                 # right-padding zeros: |S| of empty frames is sqrt(1e-9)
    x64 = mel.double().requires_grad_()
    y64 = ref_cpu.bigvgan_forward(to64(sd), dict(h), x64)
    assert float(y64.detach().abs().max()) < 0.9
    sc64, mag64 = masked_mrstft64(y64[:, 0], target.double(), lengths)
    (sc64 + mag64).backward()
    x32 = mel.clone().requires_grad_()
    sc32, mag32 = masked_mrstft64(ref_cpu.bigvgan_forward(sd, dict(h), x32)[:, 0], target, lengths)
    (sc32 + mag32).backward()
    m = m.to(dev)
    loss = MultiResolutionSTFTLoss()

    def run(tgt):
        x = mel.to(dev).requires_grad_()
        sc, mag = loss(m(x), tgt.to(dev)[:, None, :], lengths=lengths.to(dev))
        (sc + mag).backward()
        return float(sc + mag), x.grad

    l_gpu, g_gpu = run(target)
    assert torch.isfinite(torch.tensor(l_gpu)) and bool(torch.isfinite(g_gpu).all())
    e_gpu, e_ref = rel_err(g_gpu, x64.grad), rel_err(x32.grad, x64.grad)
    report(f"[mrstft lengths] loss gpu {l_gpu:.6f} fp64 {float(sc64 + mag64):.6f}; d mel gpu-vs-fp64 {e_gpu:.2e}, oracle-fp32-vs-fp64 {e_ref:.2e}")
    assert abs(l_gpu - float(sc64 + mag64)) < 1e-4 * abs(float(sc64 + mag64))
    assert e_gpu < max(TOL, 3.0 * e_ref), (e_gpu, e_ref)
    # what the padding holds does not matter
    other = target.clone()
    other[1, L // 2:] = torch.randn(L - L // 2, generator=g)
    l_other, g_other = run(other)
    assert l_other == l_gpu and torch.equal(g_other, g_gpu)
    # lengths=None is the unmasked loss
    a0, b0 = loss(m(mel.to(dev)), target.to(dev)[:, None, :])
    a1, b1 = loss(m(mel.to(dev)), target.to(dev)[:, None, :], lengths=None)
    assert float(a0) == float(a1) and float(b0) == float(b1)


# ------------------------------------------------------------------------------------ training step with the waveform loss
def test_training_step_with_mrstft_loss(dev):
    """One VQGAN.training_step with weight_mrstft = 0.5 on the codec of test_full_training_step_matches_cpu_reference_loop, now with a
    small 80-mel x256 vocoder: logged losses against the same statements executed on the CPU in float64, the decoder WaveNet's
    gradients of the generator loss (read before any optimiser step, from generator_forward and the loss by hand) against float64
    autograd, and no gradient on the vocoder."""
    from functools import partial
    from dmel_codec_amd.configs import bigvgan_h, build_codec, oracle_cfg
    from dmel_codec_amd.utils.schedule import get_cosine_schedule_with_warmup_lr_lambda
    W = 0.5
    opt = partial(torch.optim.AdamW, lr=2e-3, betas=(0.8, 0.99), eps=1e-5)
    sched = partial(torch.optim.lr_scheduler.LambdaLR,
                    lr_lambda=partial(get_cosine_schedule_with_warmup_lr_lambda, num_warmup_steps=1, num_training_steps=10, final_lr_ratio=0.1))
    torch.manual_seed(4321)
    codec = build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=2, discriminator=True, optimizer=opt, lr_scheduler=sched,
                        vocoder=dict(bigvgan_h("base_24k_100band", num_mels=80, upsample_initial_channel=64)), weight_mrstft=W)
    randomise(codec.encoder, 4322); randomise(codec.quantizer, 4323, scale=1.5); randomise(codec.decoder, 4324)
    randomise(codec.vocoder, 4325, scale=0.7)
    scale_conv_post(codec.vocoder)
    with torch.no_grad():
        codec.quality_projection.weight.normal_(0, 0.3)
        codec.quality_projection.bias.normal_(0, 0.1)
        for m in codec.quantizer.modules():
            if hasattr(m, "gamma"):
                m.gamma.normal_(0, 0.3)
    codec.discriminator.load_state_dict(ref_cpu.seeded_discriminator_sd(31337))
    cfg = oracle_cfg(codec)
    h = dict(codec.vocoder.h)
    full_sd = cpu_sd(codec)
    gen = torch.Generator().manual_seed(5)
    L, hop = 8000, 256
    audio, lens, noise = torch.randn(2, 1, L, generator=gen) * 0.2, torch.tensor([L, 5555]), torch.randn(2, 560, L // hop, generator=gen)

    def leaves(dtype):
        gsd = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in full_sd.items()
               if not k.startswith(("discriminator.", "vocoder.")) and "diffusion_projection" not in k and v.is_floating_point()}
        dsd = {k[len("discriminator."):]: v.detach().clone().to(dtype).requires_grad_() for k, v in full_sd.items() if k.startswith("discriminator.")}
        voc = {k[len("vocoder."):]: v.to(dtype) for k, v in full_sd.items() if k.startswith("vocoder.")}
        return gsd, dsd, voc

    def avg(x, m):
        return (x * m).sum() / m.expand_as(x).sum()

    def generator_losses(gsd, dsd, voc, gen_mel, gt, mask, dmask):
        dist = (gen_mel - gt).abs()
        loss_mel = (avg(dist[:, :40], mask) * 0.6 + avg(dist[:, 40:70], mask) * 0.3 + avg(dist[:, 70:], mask) * 0.1) * 0.5 + avg(dist, mask) * 0.5
        loss_adv = avg((ref_cpu.discriminator_forward(dsd, "", gen_mel) - 1) ** 2, dmask)
        wav = ref_cpu.bigvgan_forward(voc, h, gen_mel)
        if gen_mel.dtype == torch.float64:
            assert float(wav.detach().abs().max()) < 0.9, "the reference vocoder saturates its output non-linearity"
        n = gen_mel.shape[2] * hop
        sc, mag = masked_mrstft64(wav[:, 0], audio[:, 0, :n].to(gen_mel.dtype), (lens // hop) * hop)
        return loss_mel, loss_adv, sc + mag

    def reference(dtype, d_step):
        """The statements of training_step on leaves of `dtype`; d_step=False: the generator loss alone, for its gradients."""
        gsd, dsd, voc = leaves(dtype)
        _, gen_mel, gt = ref_cpu.vqgan_generator_loss(gsd, cfg, audio, lens, noise)
        mask = (torch.arange(gt.shape[2])[None, :] < (lens // hop)[:, None])[:, None, :].to(dtype)
        real = ref_cpu.discriminator_forward(dsd, "", gt)
        dmask = F.interpolate(mask, size=(real.shape[2],), mode="nearest")
        loss_d = None
        if d_step:
            od = opt(list(dsd.values()))
            sd_ = sched(od)                                    # the scheduler sets the learning rate of this first step
            fake = ref_cpu.discriminator_forward(dsd, "", gen_mel.detach())
            loss_d = avg((real - 1) ** 2, dmask) + avg(fake ** 2, dmask)
            loss_d.backward()
            torch.nn.utils.clip_grad_norm_(list(dsd.values()), 1000.0)
            od.step(); od.zero_grad(); sd_.step()
        loss_mel, loss_adv, loss_mr = generator_losses(gsd, dsd, voc, gen_mel, gt, mask, dmask)
        loss = loss_mel + loss_adv + W * loss_mr
        loss.backward()
        grads = {k: v.grad for k, v in gsd.items() if k.startswith("decoder.")}
        return dict(d=loss_d, mel=loss_mel, adv=loss_adv, mr=loss_mr, g=loss), grads

    _, g64 = reference(torch.float64, d_step=False)
    _, g32 = reference(torch.float32, d_step=False)
    logs64, _ = reference(torch.float64, d_step=True)

    codec = codec.to(dev)
    a_d, l_d, n_d = audio.to(dev), lens.to(dev), noise.to(dev)
    # ---- gradients of the generator loss, before any optimiser step
    gen_mel, gt, mask = codec.generator_forward(a_d, l_d, noise=n_d)
    dmask = F.interpolate(mask, size=(codec.discriminator(gt).shape[2],), mode="nearest")
    loss = (codec.mel_loss(gen_mel, gt, mask) + avg((codec.discriminator(gen_mel) - 1) ** 2, dmask)
            + W * codec.mrstft_loss(gen_mel, a_d, l_d))
    loss.backward()
    worst = (0.0, 0.0, "")
    for k, ref in g64.items():
        got = dict(codec.named_parameters())[k].grad
        if ref is None or float(ref.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        e_gpu, e_ref = rel_err(got, ref), rel_err(g32[k], ref)
        if e_gpu / max(TOL, 3.0 * e_ref) > worst[0] / max(TOL, 3.0 * worst[1]) or not worst[2]:
            worst = (e_gpu, e_ref, k)
        assert e_gpu < max(TOL, 3.0 * e_ref), (k, e_gpu, e_ref)
    report(f"[training step + mrstft] decoder gradients, closest to the bar: {worst[2]} gpu-vs-fp64 {worst[0]:.2e}, fp32-autograd-vs-fp64 {worst[1]:.2e}")
    assert all(p.grad is None for p in codec.vocoder.parameters())
    for p in codec.parameters():
        p.grad = None
    # ---- the step itself
    logs = codec.training_step({"audios": a_d, "audio_lengths": l_d}, 0, noise=n_d)
    for name, key in (("train/discriminator/loss", "d"), ("train/generator/loss_mel", "mel"), ("train/generator/loss_adv", "adv"),
                      ("train/generator/loss_mrstft", "mr"), ("train/generator/loss", "g")):
        ref = float(logs64[key].detach())
        report(f"[training step + mrstft] {name}: gpu {logs[name]:.6f}, fp64 loop {ref:.6f}")
        assert abs(logs[name] - ref) < 1e-4 * abs(ref), (name, logs[name], ref)
    assert all(p.grad is None for p in codec.vocoder.parameters())
