"""Micro-benchmark of the one-launch forms of the vocoder's head activations and tail against the separate launches (GPU only).

  python tools/bench_snake_fused.py                      separate and one-launch forms of the library of the tree take turns
  python tools/bench_snake_fused.py --parent-lib P.so    the separate launches come from another build (the parent commit's library)

Heads: three dmel_aa_snake_f32 launches of one tensor against one dmel_aa_snake3_forward, on the four BigVGAN-base stage shapes at batch 32.
Tail: dmel_aa_snake_f32 + dmel_conv_post_f32 against dmel_snake_post_forward on the output shape.  --rounds alternating rounds of --iters
launches each; prints median [min .. max] per form, whether the outputs are torch.equal, and whether the one-launch form's max lies below
the separate form's min.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_codec_amd import _lib
from oracle import ref_cpu

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--batch", type=int, default=32)
args = ap.parse_args()

new = _lib.lib()
old = new
if args.parent_lib:
    old = C.CDLL(os.path.abspath(args.parent_lib))
    for name in ("dmel_aa_snake_f32", "dmel_conv_post_f32"):
        fn = getattr(old, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
dev = torch.device("cuda:0")
taps = ref_cpu.aa_filter12().view(-1).contiguous()
tp = taps.data_ptr()
B = args.batch


def timed(forms):
    """forms: name -> callable; alternating rounds; us per call"""
    # one untimed round of the same length: the first round on freshly allocated tensors is slow for every form (first touch of the
    # outputs, clocks), and three launches did not absorb that on the 96 MB shapes
    for f in forms.values():
        for _ in range(args.iters):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) / args.iters * 1e3)
    return us


def show(what, us, nbytes, equal):
    for k, v in us.items():
        med = statistics.median(v)
        print(f"{what}  {k:9s} {med:7.1f} us [{min(v):.1f} .. {max(v):.1f}]  {nbytes[k] / med / 1e3:7.1f} GB/s", flush=True)
    sep, one_ = us["separate"], us["one"]
    print(f"{what}  outputs torch.equal: {equal}   one-launch max below separate min: {max(one_) < min(sep)}"
          f"   separate / one (medians): {statistics.median(sep) / statistics.median(one_):.2f}x", flush=True)


for (C_, T) in [(256, 736), (128, 5888), (64, 11776), (32, 23552)]:
    g = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(B, C_, T, device=dev, generator=g)
    al = [torch.randn(C_, device=dev, generator=g) * 0.3 for _ in range(3)]
    be = [torch.randn(C_, device=dev, generator=g) * 0.3 for _ in range(3)]
    ys = [torch.empty_like(x) for _ in range(3)]
    y3 = [torch.empty_like(x) for _ in range(3)]
    st = _lib.stream_ptr()

    def separate():
        for k in range(3):
            rc = old.dmel_aa_snake_f32(x.data_ptr(), ys[k].data_ptr(), al[k].data_ptr(), be[k].data_ptr(), tp, tp, 1, B, C_, T, st)
            assert rc == 0

    def one():
        rc = new.dmel_aa_snake3_forward(x.data_ptr(), y3[0].data_ptr(), y3[1].data_ptr(), y3[2].data_ptr(), al[0].data_ptr(), be[0].data_ptr(),
                                        al[1].data_ptr(), be[1].data_ptr(), al[2].data_ptr(), be[2].data_ptr(), tp, tp, 1, B, C_, T, st)
        assert rc == 0

    us = timed({"separate": separate, "one": one})
    n = 4.0 * B * C_ * T
    show(f"heads C={C_:4d} T={T:6d}", us, {"separate": 6 * n, "one": 4 * n}, all(torch.equal(a, b) for a, b in zip(ys, y3)))
    del x, ys, y3

C_, T = 32, 23552
g = torch.Generator(device=dev).manual_seed(9)
x = torch.randn(B, C_, T, device=dev, generator=g)
al, be = torch.randn(C_, device=dev, generator=g) * 0.3, torch.randn(C_, device=dev, generator=g) * 0.3
w = torch.randn(C_, 7, device=dev, generator=g) * 0.03
ua = torch.empty_like(x)
y2, y1 = torch.empty(B, 1, T, device=dev), torch.empty(B, 1, T, device=dev)
st = _lib.stream_ptr()


def separate():
    assert old.dmel_aa_snake_f32(x.data_ptr(), ua.data_ptr(), al.data_ptr(), be.data_ptr(), tp, tp, 1, B, C_, T, st) == 0
    assert old.dmel_conv_post_f32(ua.data_ptr(), w.data_ptr(), 0.0, 2, y2.data_ptr(), B, C_, 7, T, st) == 0


def one():
    assert new.dmel_snake_post_forward(x.data_ptr(), al.data_ptr(), be.data_ptr(), tp, tp, 1, w.data_ptr(), 0.0, 2, y1.data_ptr(), B, C_, 7, T, st) == 0


us = timed({"separate": separate, "one": one})
n = 4.0 * B * T
show(f"tail  C={C_:4d} T={T:6d}", us, {"separate": n * (3 * C_ + 1), "one": n * (C_ + 1)}, torch.equal(y1, y2))
