"""BigVGAN-only benchmark (BASELINE.json configs[3]: the 112-122 M parameter v2 vocoders, batch 16, 94 mel frames).

    python tools/bench_vocoder.py [--config v2_44k_128band_512x] [--batch 16] [--frames 94]
Prints one JSON line: audio-seconds per second, ms per forward, algorithmic conv TFLOP/s (serialised profiled pass).

    python tools/bench_vocoder.py --backward [--config base_24k_100band] [--batch 32] [--frames 94] [--steps 20]
The input gradient through the frozen generator: dmel_bigvgan_forward, _forward_train and _backward_input in ms (median over --steps
calls after warm-up, hipEvents), the library's launches of each, dmel_bigvgan_train_workspace_bytes, and the aa_snake backward kernels
alone at the last stage's shape."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_codec_amd import _lib
from dmel_codec_amd.configs import BIGVGAN, bigvgan_h
from dmel_codec_amd.models.modules.bigvgan.bigvgan import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="v2_44k_128band_512x", choices=sorted(BIGVGAN))
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--frames", type=int, default=94)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--backward", action="store_true")
ap.add_argument("--streams", type=int, default=3, choices=(1, 3))
args = ap.parse_args()
if args.backward and "--config" not in sys.argv:
    args.config = "base_24k_100band"
if args.backward and "--batch" not in sys.argv:
    args.batch = 32
if args.backward and "--steps" not in sys.argv:
    args.steps = 20
dev = torch.device("cuda:0")
h = bigvgan_h(args.config)
torch.manual_seed(0)
m = BigVGAN(h)
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for name, p in m.named_parameters():
        if name.endswith("weight_v"):
            p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
        elif name.endswith("weight_g"):
            p.fill_(1.0)
m = m.to(dev)
mel = torch.randn(args.batch, h.num_mels, args.frames, device=dev)


def backward_bench():
    import statistics
    import dmel_codec_amd.torch_ops  # noqa: F401
    ops, L = torch.ops.dmel_hip, _lib.lib()
    m.set_streams(args.streams)
    m.enable_input_grad()
    hd, up = m.native(), m._total_up()
    B, T = args.batch, args.frames
    ws_inf = torch.empty(L.dmel_bigvgan_workspace_bytes(hd, B, T), dtype=torch.uint8, device=dev)
    nbytes = L.dmel_bigvgan_train_workspace_bytes(hd, B, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dy = torch.randn(B, 1, T * up, device=dev)
    families = ("conv_igemm", "aa_snake", "aa_snake_bwd", "small")

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(max(args.steps, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        _lib.prof_reset(); _lib.prof_enable(True)
        fn(); torch.cuda.synchronize()
        _lib.prof_enable(False)
        fam = {k: _lib.prof_read(k) for k in families}
        return round(statistics.median(ms), 3), {k: v["launches"] for k, v in fam.items() if v["launches"]}, {k: round(v["ms"], 3) for k, v in fam.items() if v["launches"]}

    out = {"config": args.config, "batch": B, "frames": T, "streams": args.streams, "train_workspace_bytes": nbytes,
           "inference_workspace_bytes": ws_inf.numel()}
    for name, fn in (("forward", lambda: ops.bigvgan_forward(hd, mel, up, ws_inf)),
                     ("forward_train", lambda: ops.bigvgan_forward_train(hd, mel, up, ws)),
                     ("backward_input", lambda: ops.bigvgan_backward_input(hd, dy, h.num_mels, up, ws))):
        ms, launches, fam_ms = timed(fn)
        out[name] = {"ms": ms, "launches": launches, "launches_total": sum(launches.values()), "serialised_family_ms": fam_ms}
    out["forward_train"]["launches_total"] += 1          # + the device-to-device copy of the audio into the workspace
    out["backward_over_forward"] = round(out["backward_input"]["ms"] / out["forward"]["ms"], 2)
    # the activation backward alone, at the last stage's shape: with parameter gradients (dmel_aa_snake_backward_f32) and dx only
    ch, Tf = h.upsample_initial_channel >> len(h.upsample_rates), T * up
    x, g = torch.randn(B, ch, Tf, device=dev), torch.randn(B, ch, Tf, device=dev)
    a, b, taps = torch.randn(ch, device=dev) * 0.3, torch.randn(ch, device=dev) * 0.3, m.activation_post.upsample.filter
    out["aa_snake_backward_ms"] = timed(lambda: ops.aa_snake_backward(x, g, a, b, taps, taps, True))[0]
    out["aa_snake_backward_input_ms"] = timed(lambda: ops.aa_snake_backward_input(x, g, None, a, b, taps, taps, True))[0]
    out["aa_snake_forward_ms"] = timed(lambda: ops.aa_snake(x, a, b, taps, taps, True))[0]
    print(json.dumps(out))


if args.backward:
    backward_bench()
    sys.exit(0)
for _ in range(2):
    y = m(mel)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    y = m(mel)
torch.cuda.synchronize()
el = (time.perf_counter() - t0) / args.steps
m.set_streams(1)
m(mel); torch.cuda.synchronize()
_lib.prof_reset(); _lib.prof_enable(True)
for _ in range(args.steps):
    m(mel)
torch.cuda.synchronize()
_lib.prof_enable(False)
conv, snake = _lib.prof_read("conv_igemm"), _lib.prof_read("aa_snake")
sr = {"base_24k_100band": 24000, "v2_24k_100band_256x": 24000, "v2_44k_128band_512x": 44100}[args.config]
print(json.dumps({"config": args.config, "params_M": round(sum(p.numel() for p in m.parameters()) / 1e6, 2),
                  "batch": args.batch, "frames": args.frames, "samples_out": y.shape[-1], "ms_per_forward": round(el * 1e3, 2),
                  "audio_sec_per_sec": round(args.batch * y.shape[-1] / sr / el, 1),
                  "conv_TFLOPs": round(conv["flops"] / conv["ms"] / 1e9, 1), "conv_ms": round(conv["ms"] / args.steps, 2),
                  "conv_gflop": round(conv["flops"] / args.steps / 1e9, 1),
                  "snake_ms": round(snake["ms"] / args.steps, 2), "snake_GBs": round(snake["bytes"] / snake["ms"] / 1e6, 1)}))
