"""Multi-resolution STFT loss on the MI355X.  BASELINE.json's north_star lists it next to the BigVGAN decode side; the reference has
NO such loss (its generator loss is band-weighted mel L1 + LSGAN, codec_lit_modules.py:246-274) -- so there is nothing in the
reference to be on par with: PARITY UNPINNED BY THE REFERENCE.  The definition is the standard one (Parallel WaveGAN): per resolution
    spectral convergence  || |S(y)| - |S(x)| ||_F / || |S(y)| ||_F     +     mean | log|S(y)| - log|S(x)| |
averaged over the resolutions, with the reference's own STFT framing (utils/spectrogram.py:58-76) at each resolution, and it is
checked against a torch.stft restatement in oracle/ref_cpu.py.  The magnitudes come from the fused STFT kernel
(torch.ops.dmel_hip.stft_magnitude, one launch per signal and resolution, mel stage skipped).

Differentiable with respect to `pred` (round 3): torch.ops.dmel_hip.stft_magnitude has a native backward (dmel_stft_magnitude_backward_f32:
the windowed DFT and its transpose as GEMMs on the library's convolution kernel, overlap-add with the reflect padding folded back), so
the loss can train whatever produces the waveform.  In the reference's own training_step the vocoder between the trained networks
and a waveform is frozen (codec_lit_modules.py:68-72) and nothing differentiates through it; here BigVGAN.forward has an input
gradient (dmel_bigvgan_backward_input: d loss / d mel through the frozen generator), so the loss reaches the decoder that produced
the mel: VQGAN(weight_mrstft > 0) adds it to the generator step.  The vocoder's own weights stay frozen (fine-tuning it is not built).

`lengths` (samples per item of a right-padded batch): samples at or behind lengths[b] are zeroed in BOTH signals before the STFT, a
frame t of a resolution with hop h counts only if t < lengths[b] // h, both norms of the spectral-convergence term and the mean of the
log term run over counted entries only, and masked-out magnitudes are replaced before the log -- loss and gradient do not depend on
what the padding holds and stay finite on its zeros."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from .. import torch_ops  # noqa: F401  (registers torch.ops.dmel_hip.*)


class MultiResolutionSTFTLoss(nn.Module):
    def __init__(self, fft_sizes: Sequence[int] = (1024, 2048, 512), hop_sizes: Sequence[int] = (120, 240, 50),
                 win_lengths: Sequence[int] = (600, 1200, 240)):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.resolutions = list(zip(fft_sizes, hop_sizes, win_lengths))

    def forward(self, pred: torch.Tensor, target: torch.Tensor, lengths: Optional[torch.Tensor] = None):
        """pred / target: (B, L) or (B, 1, L) on the GPU -> (spectral convergence, log-magnitude L1), each averaged over resolutions.
        Gradients flow to `pred` (the target's magnitudes are constants).  lengths: (B,) valid samples per item, or None."""
        if pred.ndim == 3:
            pred, target = pred[:, 0], target[:, 0]
        if lengths is not None:
            lengths = lengths.reshape(-1).to(device=pred.device, dtype=torch.int64)
            if lengths.numel() != pred.shape[0]:
                raise ValueError("lengths do not match the batch")
            keep = torch.arange(pred.shape[1], device=pred.device)[None, :] < lengths[:, None]
            pred, target = pred * keep, target * keep
        sc_total, mag_total = 0.0, 0.0
        for n_fft, hop, win in self.resolutions:
            sp = torch.ops.dmel_hip.stft_magnitude(pred, n_fft, win, hop)
            with torch.no_grad():
                st = torch.ops.dmel_hip.stft_magnitude(target, n_fft, win, hop)
            if lengths is not None:
                counted = (torch.arange(sp.shape[1], device=sp.device)[None, :] < (lengths // hop)[:, None])[:, :, None]
                one = torch.ones((), dtype=sp.dtype, device=sp.device)
                sp, st = torch.where(counted, sp, one), torch.where(counted, st, one)      # masked entries: |S| := 1 on both sides
                # a resolution none of whose frames counts (every item shorter than its hop) contributes 0, not 0 / 0
                n = (counted.sum() * sp.shape[2]).clamp_min(1)
                ref = torch.linalg.norm(torch.where(counted, st, torch.zeros_like(one))).clamp_min(torch.finfo(sp.dtype).tiny)
                sc_total = sc_total + torch.linalg.norm(st - sp) / ref
                mag_total = mag_total + (st.log() - sp.log()).abs().sum() / n
                continue
            sc_total = sc_total + torch.linalg.norm(st - sp) / torch.linalg.norm(st)
            mag_total = mag_total + (st.log() - sp.log()).abs().mean()
        n = len(self.resolutions)
        return sc_total / n, mag_total / n
