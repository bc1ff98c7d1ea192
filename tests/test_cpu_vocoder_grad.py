"""Input gradient through the frozen BigVGAN, the parts that need no GPU: the new C-ABI symbols are declared, exported and bound; calls
that cannot run (NULL, bad shape, handle not enabled) return the library's argument error with a message naming the entry point; the
Python surface has the new arguments."""
import ctypes as C
import inspect
import os
import re

import pytest

from dmel_codec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dmel_bigvgan_enable_input_grad", "dmel_bigvgan_train_workspace_bytes", "dmel_bigvgan_forward_train",
               "dmel_bigvgan_backward_input", "dmel_conv_transpose1d_backward_data", "dmel_conv_post_backward_f32",
               "dmel_aa_snake_backward_input_f32"]
DMEL_EINVAL = -1


def last_error() -> str:
    return _lib.lib().dmel_last_error().decode()


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_symbol_is_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "dmel_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmel_hip.h"
    assert name in _lib.PROTOTYPES
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes == _lib.PROTOTYPES[name][1] and fn.restype == _lib.PROTOTYPES[name][0]


def test_abi_version_is_unchanged():
    assert _lib.lib().dmel_abi_version() == 2


def tiny_handle():
    cfg = _lib.BigVGANConfig()
    cfg.num_mels, cfg.upsample_initial_channel, cfg.num_upsamples, cfg.num_kernels = 20, 32, 2, 2
    for i, u in enumerate((4, 2)):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, 2 * u
    for j, k in enumerate((3, 5)):
        cfg.resblock_kernel_sizes[j] = k
        for l, d in enumerate((1, 3, 5)):
            cfg.resblock_dilations[j][l] = d
    cfg.snake_logscale, cfg.activation_snake, cfg.use_tanh_at_final, cfg.use_bias_at_final, cfg.resblock_type = 1, 0, 1, 1, 1
    h = C.c_void_p()
    _lib.check(_lib.lib().dmel_bigvgan_create(C.byref(h), C.byref(cfg)), "bigvgan_create")
    return h.value


def test_vocoder_training_entry_points_refuse_loudly():
    L = _lib.lib()
    buf = (C.c_float * 64)()                 # a host address: the calls below must return before touching any of their pointers
    p = C.addressof(buf)
    h = tiny_handle()
    try:
        for name in ("dmel_bigvgan_forward_train", "dmel_bigvgan_backward_input"):
            fn = getattr(L, name)
            short = name[len("dmel_"):]
            assert fn(None, p, p, 1, 4, p, 256, None) == DMEL_EINVAL and short in last_error()
            assert fn(h, None, p, 1, 4, p, 256, None) == DMEL_EINVAL and short in last_error()
            assert fn(h, p, p, 1, 4, None, 0, None) == DMEL_EINVAL and short in last_error()
            # a handle that never went through dmel_bigvgan_enable_input_grad
            assert fn(h, p, p, 1, 4, p, 256, None) == DMEL_EINVAL
            assert short in last_error() and "enable_input_grad" in last_error()
        assert L.dmel_bigvgan_enable_input_grad(None, 1) == DMEL_EINVAL and "bigvgan_enable_input_grad" in last_error()
        assert L.dmel_bigvgan_enable_input_grad(h, 1) != 0 and "bigvgan_enable_input_grad" in last_error()      # not finalized
        assert L.dmel_bigvgan_train_workspace_bytes(None, 1, 4) == 0
        assert L.dmel_bigvgan_train_workspace_bytes(h, 0, 4) == 0 and L.dmel_bigvgan_train_workspace_bytes(h, 1, 0) == 0
        # the saved activations: more than the inference workspace, and linear in the batch
        n1, n2 = L.dmel_bigvgan_train_workspace_bytes(h, 1, 16), L.dmel_bigvgan_train_workspace_bytes(h, 2, 16)
        assert n1 > L.dmel_bigvgan_workspace_bytes(h, 1, 16) and n1 < n2 <= 2 * n1
    finally:
        L.dmel_bigvgan_destroy(h)


def test_single_op_backward_entry_points_refuse_loudly():
    L = _lib.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.dmel_conv_transpose1d_backward_data(None, p, p, 1, 4, None) == DMEL_EINVAL and "conv_transpose1d_backward_data" in last_error()
    assert L.dmel_conv_transpose1d_backward_data(p, None, p, 1, 4, None) == DMEL_EINVAL and "conv_transpose1d_backward_data" in last_error()
    assert L.dmel_conv_transpose1d_backward_data(p, p, p, 0, 4, None) == DMEL_EINVAL and "bad shape" in last_error()
    assert L.dmel_conv_transpose1d_backward_data(p, p, p, 1, 0, None) == DMEL_EINVAL and "bad shape" in last_error()
    assert L.dmel_conv_post_backward_f32(p, None, p, 2, p, 1, 4, 7, 16, None) == DMEL_EINVAL and "conv_post_backward" in last_error()
    assert L.dmel_conv_post_backward_f32(None, p, p, 2, p, 1, 4, 7, 16, None) == DMEL_EINVAL and "conv_post_backward" in last_error()   # tanh needs y
    assert L.dmel_conv_post_backward_f32(p, p, p, 1, p, 1, 4, 7, 16, None) == DMEL_EINVAL and "act must be" in last_error()
    assert L.dmel_conv_post_backward_f32(p, p, p, 2, p, 1, 4, 6, 16, None) == DMEL_EINVAL and "conv_post_backward: bad shape" in last_error()
    assert L.dmel_conv_post_backward_f32(p, p, p, 2, p, 0, 4, 7, 16, None) == DMEL_EINVAL and "conv_post_backward: bad shape" in last_error()
    assert L.dmel_conv_post_backward_f32(p, p, p, 2, p, 1, 4096, 7, 16, None) == DMEL_EINVAL and "too large" in last_error()
    assert L.dmel_aa_snake_backward_input_f32(None, p, None, p, p, None, p, p, 1, 1, 4, 16, None) == DMEL_EINVAL
    assert "aa_snake_backward_input" in last_error()
    assert L.dmel_aa_snake_backward_input_f32(p, p, None, p, p, None, p, p, 1, 1, 0, 16, None) == DMEL_EINVAL and "bad shape" in last_error()


def test_python_surface():
    from dmel_codec_amd.models.codec_lit_modules import VQGAN
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.utils.mrstft import MultiResolutionSTFTLoss
    sig = inspect.signature(VQGAN.__init__)
    assert "weight_mrstft" in sig.parameters and sig.parameters["weight_mrstft"].default == 0.0
    sig = inspect.signature(MultiResolutionSTFTLoss.forward)
    assert "lengths" in sig.parameters and sig.parameters["lengths"].default is None
    assert callable(getattr(BigVGAN, "enable_input_grad"))
    assert "NEVER receive a gradient" in BigVGAN.forward.__doc__
    import torch
    import dmel_codec_amd.torch_ops  # noqa: F401
    for op in ("bigvgan_forward_train", "bigvgan_backward_input", "conv_transpose1d_backward", "conv_post_backward", "aa_snake_backward_input"):
        assert hasattr(torch.ops.dmel_hip, op)


def test_weight_mrstft_needs_a_matching_vocoder():
    from dmel_codec_amd.configs import build_codec
    small = dict(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, residual_channels=8)
    voc = dict(num_mels=80, upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=32, resblock="1",
               resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]], activation="snakebeta", snake_logscale=True)
    with pytest.raises(ValueError, match="needs a vocoder"):
        build_codec(vocoder=None, weight_mrstft=0.5, **small)
    with pytest.raises(ValueError, match="does not match"):
        build_codec(vocoder=voc, hop_length=128, weight_mrstft=0.5, **small)            # x256 vocoder, hop 128
    with pytest.raises(ValueError, match="does not match"):
        build_codec(vocoder=dict(voc, sampling_rate=22050), weight_mrstft=0.5, **small)  # 22.05 kHz vocoder, 24 kHz mel
    codec = build_codec(vocoder=voc, weight_mrstft=0.5, **small)
    assert codec.weight_mrstft == 0.5 and codec.mrstft is not None
    assert all(not p.requires_grad for p in codec.vocoder.parameters())
    assert build_codec(vocoder=voc, **small).mrstft is None
