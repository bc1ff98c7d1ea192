"""CPU-side checks of the boundary: the C-ABI library builds, loads without a GPU, exports every symbol
include/dmel_hip.h declares, fails loudly (no fallback), and its host-side logic matches the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import ref_cpu


@pytest.fixture(scope="module")
def L():
    from dmel_codec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from dmel_codec_amd.build import build
        build(verbose=False)
    return _lib.lib()


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "dmel_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dmel_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(L):
    from dmel_codec_amd import _lib
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/dmel_hip.h but not exported by libdmel_hip.so"
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    assert L.dmel_abi_version() == 2


def test_errors_are_loud_not_fallbacks(L):
    from dmel_codec_amd import _lib
    h = C.c_void_p()
    rc = L.dmel_stft_plan_create(C.byref(h), 44100, 4096, 4096, 1024, 128, 0.0, 0.0, None)
    assert rc == -2 and b"n_fft" in L.dmel_last_error()
    with pytest.raises(RuntimeError, match="n_fft"):
        _lib.check(rc, "stft_plan_create")
    lv = (C.c_int * 3)(7, 5, 5)
    fs = (C.c_int * 2)(2, 3)
    assert L.dmel_quantizer_create(C.byref(h), 700, 10, lv, 3, fs, 2, 1) == -2
    assert L.dmel_quantizer_create(C.byref(h), 701, 10, lv, 3, fs, 2, 1) == -1
    # CPU tensors are refused by the mirror modules (there is no CPU path)
    from dmel_codec_amd.utils.spectrogram import LogMelSpectrogram
    with pytest.raises(RuntimeError, match="GPU"):
        LogMelSpectrogram(sample_rate=24000, n_fft=1024, win_length=1024, hop_length=256, n_mels=100)(torch.zeros(1, 4000))


def test_missing_weights_are_reported(L):
    h = C.c_void_p()
    assert L.dmel_wavenet_create(C.byref(h), 10, 0, 70, 2, 4, 0) == 0
    rc = L.dmel_wavenet_finalize(h)
    assert rc == -3 and b"missing state-dict tensor 'input_projection.conv." in L.dmel_last_error()
    w = torch.zeros(70, 11, 1)
    shape = (C.c_int64 * 3)(70, 11, 1)
    assert L.dmel_wavenet_set_tensor(h, b"input_projection.conv.weight", w.data_ptr(), shape, 3) == 0
    bshape = (C.c_int64 * 1)(70)
    assert L.dmel_wavenet_set_tensor(h, b"input_projection.conv.bias", w.data_ptr(), bshape, 1) == 0
    assert L.dmel_wavenet_finalize(h) == -3 and b"shape" in L.dmel_last_error()
    L.dmel_wavenet_destroy(h)


def test_mel_basis_matches_oracle(L):
    for sr, n_mels, fmax in ((24000, 100, 12000.0), (16000, 80, None), (24000, 80, None), (44100, 128, None)):
        out = torch.empty(n_mels, 513)
        assert L.dmel_mel_basis_host(sr, 1024, n_mels, 0.0, fmax or 0.0, out.data_ptr()) == 0
        ref = ref_cpu.slaney_mel_basis(sr, 1024, n_mels, 0.0, fmax)
        assert np.allclose(out.numpy(), ref, rtol=0, atol=1e-9)
        assert np.array_equal(out.numpy() != 0, ref != 0)


def test_mirror_state_dict_layout():
    """Key names are part of the drop-in contract."""
    from dmel_codec_amd.configs import build_codec
    m = build_codec(n_mels=80, dmel_groups=8, encoder_layers=2, decoder_layers=2)
    sd = m.state_dict()
    for k, shape in {
        "encoder.input_projection.conv.weight": (70, 10, 1),
        "encoder.residual_layers.1.conv_layer.conv.weight": (140, 70, 3),
        "encoder.residual_layers.0.output_projection.conv.bias": (140,),
        "encoder.skip_projection.conv.weight": (70, 70, 1),
        "quantizer.residual_fsq.rvqs.7.project_in.weight": (3, 70),
        "quantizer.residual_fsq.rvqs.0.project_out.bias": (70,),
        "quantizer.downsample.0.0.weight": (70, 70, 2),
        "quantizer.downsample.1.1.dwconv.weight": (70, 1, 7),
        "quantizer.downsample.0.1.pwconv1.weight": (280, 70),
        "quantizer.upsample.1.0.weight": (70, 70, 2),
        "quantizer.upsample.0.1.gamma": (70,),
        "decoder.residual_layers.0.condition_projection.conv.weight": (1120, 560, 1),
        "decoder.residual_layers.1.diffusion_projection.linear.weight": (560, 560),
        "decoder.output_projection.conv.weight": (80, 560, 1),
        "quality_projection.weight": (560, 1),
        "vocoder.conv_pre.weight_g": (512, 1, 1),
        "vocoder.conv_pre.weight_v": (512, 80, 7),
        "vocoder.ups.0.0.weight_v": (512, 256, 16),
        "vocoder.resblocks.0.convs1.2.weight_v": (256, 256, 3),
        "vocoder.resblocks.11.activations.5.act.beta": (32,),
        "vocoder.resblocks.3.activations.0.upsample.filter": (1, 1, 12),
        "vocoder.resblocks.3.activations.0.downsample.lowpass.filter": (1, 1, 12),
        "vocoder.activation_post.act.alpha": (32,),
        "vocoder.conv_post.weight_v": (1, 32, 7),
    }.items():
        assert k in sd, k
        assert tuple(sd[k].shape) == shape, (k, tuple(sd[k].shape))
    assert "decoder.input_projection.conv.weight" not in sd      # 560 == 560: wavenet.py:152-156


def test_mirror_state_dicts_equal_reference_modules():
    """The mirror modules carry the reference modules' state dicts: same names, same shapes, with and without weight norm.  The
    reference's layout is stored as data (tests/golden/state_dict_shapes.json, written by oracle/gen_golden_shapes.py from the reference's
    own classes built with the same arguments)."""
    import json
    from dmel_codec_amd.configs import BIGVGAN, bigvgan_h
    from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN
    from dmel_codec_amd.models.modules.firefly import ConvNeXtBlock
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_shapes.json")) as f:
        ref = json.load(f)

    def same(m, sd):
        got = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert got == sd, (set(got) ^ set(sd)) or [k for k in got if got[k] != sd[k]]

    assert ref["wavenet_enc"]["args"] == [10, None, 70, 20, 4] and ref["wavenet_cond"]["args"] == [64, 20, 64, 3, 4, False, 64]
    same(WaveNet(10, None, 70, 20, 4), ref["wavenet_enc"]["state_dict"])
    same(WaveNet(64, 20, 64, 3, 4, False, 64), ref["wavenet_cond"]["state_dict"])
    assert ref["convnext"]["args"] == [70]
    same(ConvNeXtBlock(70), ref["convnext"]["state_dict"])
    for name in ('base_24k_100band',):
        assert name in BIGVGAN
        r = ref["bigvgan_" + name]
        m = BigVGAN(bigvgan_h(name))
        same(m, r["state_dict"])
        m.remove_weight_norm()
        same(m, r["state_dict_without_weight_norm"])


def test_yaml_config_builds_the_codec():
    """The reference's config schema (`_target_`, `_partial_`, `${a.b}`, `defaults[1:]` merge of train_codec.py:12-23)
    builds the MI355X codec; `_target_` strings keep the REFERENCE's dotted paths."""
    import functools
    from dmel_codec_amd import config_loader
    from dmel_codec_amd.models.codec_lit_modules import VQGAN
    path = os.path.join(ROOT, "dmel_codec_amd", "config", "codec", "dMel_mi355x.yaml")
    cfg = config_loader.load_config(path)
    assert cfg["concat_channels_dim"] == 700 and cfg["model"]["decoder"]["residual_channels"] == 700
    assert cfg["model"]["vocoder"]["h_path"].endswith("base_24k_100band.json")
    m = config_loader.build_codec_from_config(path, overrides={"model": {"encoder": {"residual_layers": 2},
                                                                         "decoder": {"residual_layers": 2}}},
                                              load_vocoder_ckpt=False)
    assert isinstance(m, VQGAN) and m.dmel_groups == 10 and m.vocoder.h.upsample_rates == [8, 8, 2, 2]
    assert isinstance(m.optimizer_builder, functools.partial) and m.optimizer_builder.keywords["lr"] == 1e-4
    lam = m.lr_scheduler_builder.keywords["lr_lambda"]
    assert abs(lam(50) - 0.5) < 1e-12
    with pytest.raises(ValueError, match="concat_channels_dim"):
        config_loader.resolve({"concat_channels_dim": "???", "model": {"x": "${concat_channels_dim}"}})


def test_alias_package_serves_reference_paths():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dmel_codec.models.modules.wavenet import WaveNet\n"
            "from dmel_codec.utils.spectrogram import LogMelSpectrogram\n"
            "from dmel_codec.models.lit_modules import VQGAN\n"
            "from dmel_codec.models.modules.bigvgan.bigvgan import BigVGAN\n"
            "from dmel_codec.models.modules.bigvgan.alias_free_activation.torch.act import Activation1d\n"
            "import dmel_codec_amd.models.modules.wavenet as w\n"
            "assert WaveNet is w.WaveNet\nprint('ok')\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-1500:]


def test_reference_yaml_instantiates():
    """The reference's own example config (config/codec/dMel_example.yaml, stored as data in tests/golden/) builds the codec once the
    author-local vocoder paths are overridden."""
    from dmel_codec_amd import config_loader
    h = os.path.join(ROOT, "dmel_codec_amd", "config", "bigvgan", "base_24k_100band.json")
    m = config_loader.build_codec_from_config(os.path.join(ROOT, "tests", "golden", "dMel_example.yaml"),
                                              overrides={"model": {"vocoder": {"h_path": h, "ckpt_path": None}}},
                                              load_vocoder_ckpt=False)
    assert len(m.encoder.residual_layers) == 8 and m.quantizer.levels == [8, 6] and m.dmel_groups == 10
    assert m.decoder.condition_channels == 700 and m.encode_mel_transform.n_mels == 100


def test_precision_api_validation():
    """set_precision is host-side state until a handle exists: argument checking needs no GPU."""
    import pytest
    from dmel_codec_amd.configs import build_codec
    codec = build_codec(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, vocoder=None)
    for ok in ("fp32", "bf16", "fp32_mfma", torch.bfloat16, torch.float32, 0, 1, 2):
        codec.decoder.set_precision(ok)
    with pytest.raises(ValueError):
        codec.decoder.set_precision("fp16")
    with pytest.raises(NotImplementedError):
        codec.quantizer.set_precision("bf16")          # ids are the interchange format: the quantizer has no bf16 mode
    codec.quantizer.set_precision("fp32")
    codec.set_decode_precision("bf16")
    assert codec.decoder._precision == 1 and codec.encoder._precision == 0


def test_precision_entry_points_reject_bad_arguments(L):
    assert L.dmel_conv_set_precision(None, 0) < 0 and b"PRECISION" in L.dmel_last_error()
    assert L.dmel_wavenet_set_precision(None, 1) < 0
    assert L.dmel_bigvgan_set_precision(None, 1) < 0


def test_handle_cache_is_tied_to_the_tensor_not_to_its_address():
    """torch_ops caches packed-weight handles per weight tensor.  The key must be the tensor OBJECT and its version, never data_ptr():
    the allocator hands a freed weight's address to the next tensor of that shape, and a fresh tensor starts at version 0 again."""
    import gc
    from dmel_codec_amd.torch_ops import _TensorKeyedCache
    destroyed = []
    cache = _TensorKeyedCache(3, destroy=destroyed.append)
    w, b = torch.zeros(4, 4, 3), torch.zeros(4)
    assert cache.get(w, 1, b) is None
    cache.put(w, 1, "h1", b)
    assert cache.get(w, 1, b) == "h1"
    assert cache.get(w, 2, b) is None                                   # another dilation: its own entry
    assert cache.get(w, 1, None, any_other=True) == "h1"                # backward does not care which bias the handle was built with
    assert cache.get(w, 1, torch.zeros(4)) is None and destroyed == ["h1"]    # a different bias object: stale, destroyed, rebuilt by the caller
    cache.put(w, 1, "h2", b)
    w.add_(1.0)                                                         # in-place update (an optimiser step): version moves
    assert cache.get(w, 1, b) is None and destroyed == ["h1", "h2"]
    cache.put(w, 1, "h3", b)
    b.mul_(2.0)
    assert cache.get(w, 1, b) is None and destroyed[-1] == "h3"
    # the tensor dies: its handle is destroyed, and a NEW tensor (same shape, version 0, quite possibly the same address / id) misses
    cache.put(w, 1, "h4", b)
    del w
    gc.collect()
    assert destroyed[-1] == "h4" and len(cache.entries) == 0
    w2 = torch.zeros(4, 4, 3)
    assert cache.get(w2, 1, b) is None
    # least recently used goes first, one at a time
    ts = [torch.zeros(2) for _ in range(4)]
    for i, t in enumerate(ts[:3]):
        cache.put(t, 0, f"t{i}")
    assert cache.get(ts[0], 0) == "t0"                                  # touch 0: 1 is now the oldest
    cache.put(ts[3], 0, "t3")
    assert destroyed[-1] == "t1" and cache.get(ts[0], 0) == "t0" and cache.get(ts[2], 0) == "t2" and cache.get(ts[3], 0) == "t3"


def test_copies_of_a_mirror_never_share_its_native_handle():
    """copy.deepcopy (what dmel_codec_amd.pipeline.CodecLanes makes its lanes with) and pickling of a mirror module: the copy carries no
    handle, no plan and no workspace of the original -- a handle is an address inside the library; copied by value, the copy's first
    native() would free the original's."""
    import copy
    import pickle
    from dmel_codec_amd.models.modules.wavenet import WaveNet
    from dmel_codec_amd.utils.spectrogram import LogMelSpectrogram
    m = WaveNet(input_channels=10, output_channels=10, residual_channels=16, residual_layers=2, dilation_cycle=2)
    m._handle, m._handle_versions = 0xDEAD0000, ("stale",)      # pretend a handle exists (never dereferenced: reset below)
    m._ws.buf = torch.zeros(4)
    try:
        for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
            assert c._handle is None and c._handle_versions is None and c._ws is not m._ws and c._ws.buf is None
            assert len(c._train_calls) == 0 and c._grad_sink is None
            assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), c.state_dict().values()))
        assert m._handle == 0xDEAD0000
    finally:
        m._handle = None      # or __del__ would hand the fake address to the library
    s = LogMelSpectrogram(sample_rate=24000, n_fft=1024, win_length=1024, hop_length=256, n_mels=80)
    s.spectrogram._plan = 0xBEEF0000
    try:
        assert copy.deepcopy(s).spectrogram._plan is None
    finally:
        s.spectrogram._plan = None


def test_lanes_refuse_a_cpu_codec():
    """dmel_codec_amd.pipeline.CodecLanes has no CPU form either: a codec that is not on a GPU raises (it would otherwise copy the codec
    and fail later, inside the first native call)."""
    from dmel_codec_amd.configs import build_codec
    from dmel_codec_amd.pipeline import CodecLanes
    codec = build_codec(n_mels=80, dmel_groups=8, encoder_layers=1, decoder_layers=1, vocoder=None)
    with pytest.raises(RuntimeError, match="CUDA"):
        CodecLanes(codec, 2)
    with pytest.raises(ValueError):
        CodecLanes(codec, 0)


def test_env_switches_are_the_documented_ones():
    """The DMEL_* names that csrc/ passes to getenv are exactly the rows of the environment-variable table of DESIGN.md, and the six files
    that used to carry A/B variants define no compile-time -D switch: a new knob has to be written down, with the test that uses it."""
    import glob
    csrc = os.path.join(ROOT, "dmel_codec_amd", "csrc")
    read = set()
    for path in glob.glob(os.path.join(csrc, "*")):
        read |= set(re.findall(r'getenv\(\s*"(DMEL_[A-Z0-9_]+)"', open(path).read()))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("### Environment variables read by the library"):]
    table = table[:table.index("\n## ")]
    documented = set(re.findall(r"^\| `(DMEL_[A-Z0-9_]+)` \|", table, flags=re.M))
    assert read and read == documented, (sorted(read - documented), sorted(documented - read))
    for name in ("conv_igemm.hip", "conv_pc.hip", "conv_bwd.hip", "aa_snake.hip", "conv_snake.hip", "modules.hip"):
        assert "#ifndef DMEL_" not in open(os.path.join(csrc, name)).read(), name


def test_conv_matrix_reaches_every_kernel_branch():
    """tests/test_gpu_conv_matrix.py claims to cover every tile / operand split / halo class of the forward kernel and every branch of
    launch_wgrad_any and launch_bgrad (csrc/conv_bwd.hip).  Its branch predicates are a Python mirror of lines of conv_bwd.hip: those
    lines must still read as transcribed, and the parametrisation must reach every branch at least twice."""
    import collections
    import test_gpu_conv_matrix as m
    src = open(os.path.join(ROOT, "dmel_codec_amd", "csrc", "conv_bwd.hip")).read()
    for line in m.WGRAD_PREDICATE_SOURCE:
        assert line in src, f"conv_bwd.hip no longer contains `{line}`: update the mirror in test_gpu_conv_matrix.py"
    wg = collections.Counter(m.wgrad_branch(k, dil, T) for (Cout, Cin, k, dil, T, B) in m.WGRAD_CASES)
    bg = collections.Counter(m.bgrad_branch(Cout, B, T) for (Cout, Cin, k, dil, T, B) in m.WGRAD_CASES)
    assert set(wg) == set(m.WGRAD_BRANCHES) and min(wg.values()) >= 2, wg
    assert set(bg) == set(m.BGRAD_BRANCHES) and min(bg.values()) >= 2, bg
    # boundaries on both sides: T = 32 | 33 (ipc), 255 | 256 (split), a B that is not a multiple of ipc, > 1024 channels for db
    Ts = {T for (_, _, _, _, T, _) in m.WGRAD_CASES}
    assert {32, 33, 255, 256} <= Ts
    assert any(T <= 32 and B % (64 // T) for (_, _, _, _, T, B) in m.WGRAD_CASES)
    assert any(Cout > 1024 for (Cout, *_rest) in m.WGRAD_CASES)
    assert {1, 17, 64, 65, 130} <= {c for (Cout, Cin, *_rest) in m.WGRAD_CASES for c in (Cout, Cin)}
    # the grouped path with one K slice and with many (slices = max(1, min(ceil(1024 / (tm tn groups)), ceil(B ceil(T / 64) / 8))))
    slices = set()
    for (Cout, Cin, k, dil, T, B) in m.WGRAD_CASES:
        if m.wgrad_branch(k, dil, T) == "grouped":
            tiles = ((Cout + 63) // 64) * ((Cin + 63) // 64) * (k // 3)
            slices.add(max(1, min((1024 + tiles - 1) // tiles, (B * ((T + 63) // 64) + 7) // 8)))
    assert 1 in slices and max(slices) >= 8, slices
    # forward: every halo class, the edges of each, and the ragged channel / length / batch sets the module promises
    halos = {(k - 1) * dil for (_, _, k, dil, _, _) in m.FWD_SHAPES}
    assert {0, 16, 64} <= halos and any(0 < h < 16 for h in halos) and any(16 < h < 64 for h in halos)
    assert {m.halo_class(k, dil) for (_, _, k, dil, _, _) in m.FWD_SHAPES} == {0, 16, 64}
    assert {1, 31, 33, 100, 129, 257, 300} <= {s[0] for s in m.FWD_SHAPES}
    assert {8, 17, 24, 130} <= {s[1] for s in m.FWD_SHAPES}
    Tf = {s[4] for s in m.FWD_SHAPES}
    assert {1, 2, 31, 32, 33, 95, 96, 97, 127, 128, 129, 255, 256, 257} <= Tf and max(Tf) >= 3000
    assert any(T < (k - 1) * dil for (_, _, k, dil, T, _) in m.FWD_SHAPES)
    assert {1, 3} <= {s[5] for s in m.FWD_SHAPES}
    assert set(m.NPS) == {1, 2, 3} and list(m.TILES) == list(range(8))
    assert all(t <= m.TAU_CEIL for t in m.TAU.values()) and m.TAU_CEIL == 2.0 ** -16


# the lines of csrc/ that tests/test_gpu_wavenet_one_launch_matrix.py transcribes (its eligible(), MAX_T, MAX_STREAM_L, SUBSTEP), per file
ONE_LAUNCH_PREDICATE_SOURCE = {
    "modules.hip": (
        "if (C > 32 && C <= 80 && !m->Ccond && !m->has_out && (!m->has_in || m->Cin <= 16) && (m->cycle == 0 || m->cycle <= 4)) {",
        "if (m->fused.ok && T <= 96 && m->precision == DMEL_PRECISION_FP32 && !(e && e[0] == '0') && !conv_fp32_mfma_forced())",
        "if (m->Ccond || cond || !m->fused.ok || m->L > kStreamMaxL || m->precision != DMEL_PRECISION_FP32 || conv_fp32_mfma_forced()) {",
        "if (m->fused.ok && L <= kStreamMaxL && m->precision == DMEL_PRECISION_FP32 && !(e && e[0] == '0') && !conv_fp32_mfma_forced())",
    ),
    "ops.h": ("constexpr int kStreamMaxL = 32;",),
    "wavenet_fused.hip": ("constexpr int kFT = 96;", "constexpr int kFH = 8;"),
    "wavenet_stream.hip": ("constexpr int kST = 96;", "constexpr int kSH = 8;"),
}


def test_one_launch_matrix_mirrors_the_dispatch_of_the_wavenet_kernels():
    """tests/test_gpu_wavenet_one_launch_matrix.py places its cases by a Python mirror of the conditions under which dmel_wavenet_forward and
    the streaming entries take the one-launch kernels.  The lines it transcribes must still read as transcribed, and the mirror must say
    what they say at every edge."""
    import test_gpu_wavenet_one_launch_matrix as m
    for name, lines in ONE_LAUNCH_PREDICATE_SOURCE.items():
        src = open(os.path.join(ROOT, "dmel_codec_amd", "csrc", name)).read()
        for line in lines:
            assert line in src, (f"{name} no longer contains `{line}`: update eligible() / MAX_T / MAX_STREAM_L / SUBSTEP and the case tables of "
                                 "test_gpu_wavenet_one_launch_matrix.py")
    assert (m.MAX_T, m.MAX_STREAM_L, m.SUBSTEP) == (96, 32, 96)

    def ok(C, has_in, Cin, Ccond, has_out, cycle):          # the first line, term for term
        return C > 32 and C <= 80 and not Ccond and not has_out and (not has_in or Cin <= 16) and (cycle == 0 or cycle <= 4)

    for C in (1, 32, 33, 80, 81, 512):
        for Cin in (None, 1, 16, 17, 80):
            for Ccond in (None, 0, 8):
                for has_out in (False, True):
                    for cycle in (0, 1, 4, 5):
                        assert m.eligible(C, Cin, Ccond, has_out, cycle) == ok(C, Cin is not None, Cin or C, Ccond or 0, has_out, cycle)


def test_conv_matrix_guards_catch_missing_and_stray_stores():
    """The guarded buffers of tests/test_gpu_conv_matrix.py (device-agnostic, exercised here on host tensors): an output element that
    is never stored, a store past either end of an output and a write into an input's NaN band each fail the check."""
    import test_gpu_conv_matrix as m
    cpu = torch.device("cpu")
    y = m.Out((2, 3, 5), cpu)
    with pytest.raises(AssertionError, match="never written"):
        y.check()
    y.t.copy_(torch.arange(30.0).view(2, 3, 5))
    y.t[1, 2, 4] = float("nan")
    with pytest.raises(AssertionError, match="never written"):
        y.check()
    y.t[1, 2, 4] = 1.0
    assert torch.equal(y.check(), y.t)
    for at in (m.GUARD - 1, m.GUARD + 30, 0, -1):          # just before, just after, and at both far ends
        y.base[at] = 0.0
        with pytest.raises(AssertionError, match="guard"):
            y.check()
        y.base.view(torch.int32)[at] = m.SENTINEL
    y.check()
    y.t[0, 0, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        y.check()
    x = m.In(torch.randn(3, 7), cpu)
    assert torch.isnan(x.base[:m.GUARD]).all() and torch.isnan(x.base[-m.GUARD:]).all() and not torch.isnan(x.t).any()
    x.check()
    x.base[m.GUARD + 21] = 0.0
    with pytest.raises(AssertionError, match="input"):
        x.check()
    # the per-element bound: an error that the global max would hide is caught in the small output it sits in
    ref = torch.tensor([1e3, 1e-3], dtype=torch.float64)
    A = ref.abs()
    assert m.ratio(ref.float(), ref, A) < 1e-7
    bad = ref.float().clone()
    bad[1] *= 1.0 + 1e-4
    assert m.ratio(bad, ref, A) > m.TAU_CEIL
    from conftest import rel_err
    assert rel_err(bad, ref) < 1e-9
