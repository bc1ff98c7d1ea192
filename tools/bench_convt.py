"""Micro-benchmark of the transposed convolution (dmel_conv_transpose1d_forward) on the four BigVGAN up-sampler shapes of the bench
configuration (GPU only).

  python tools/bench_convt.py                                  the library of the tree
  python tools/bench_convt.py --lib A.so --lib B.so            A/B: the libraries take turns, --rounds times each per shape, on the same seeded
                                                               tensors; prints the median with [min .. max] and whether the outputs are torch.equal
  --odd                                                        also T + 1 of every shape
  --iters N                                                    launches per timing (default 20; 1 for a counter pass under rocprofv3 --pmc)
  --precision P                                                DMEL_PRECISION_* of the handles (default 3, the fp16 split the vocoder runs at)
  --stage N                                                    only stage N (1 .. 4)
DMEL_UPSTAGE_ONE_LAUNCH=0 in the environment times the two-launch path of the same library.
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmel_codec_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", default=[])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--odd", action="store_true")
ap.add_argument("--precision", type=int, default=3)
ap.add_argument("--stage", type=int, default=0)
args = ap.parse_args()

NAMES = ["dmel_conv_transpose1d_create", "dmel_conv_transpose1d_destroy", "dmel_conv_transpose1d_set_precision", "dmel_conv_transpose1d_forward"]


def load(path):
    if path is None:
        return _lib.lib()
    dll = C.CDLL(os.path.abspath(path))
    for n in NAMES:
        fn = getattr(dll, n)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[n]
    return dll


names = args.lib or [None]
libs = [load(p) for p in names]
dev = torch.device("cuda:0")
# (B, Cin, Cout, T, u): v2_24k_100band_256x at 92 frames, batch 32
shapes = [(32, 512, 256, 92, 8), (32, 256, 128, 736, 8), (32, 128, 64, 5888, 2), (32, 64, 32, 11776, 2)]
if args.stage:
    shapes = shapes[args.stage - 1:args.stage]
if args.odd:
    shapes += [(B, Ci, Co, T + 1, u) for (B, Ci, Co, T, u) in shapes]
for (B, Ci, Co, T, u) in shapes:
    g = torch.Generator().manual_seed(T)
    w = (torch.randn(Ci, Co, 2 * u, generator=g) / math.sqrt(2 * Ci)).contiguous()
    bias = (torch.randn(Co, generator=g) * 0.1).contiguous()
    x = torch.randn(B, Ci, T, generator=g).to(dev)
    st = _lib.stream_ptr()
    hs = []
    for dll in libs:
        h = C.c_void_p()
        assert dll.dmel_conv_transpose1d_create(C.byref(h), w.data_ptr(), bias.data_ptr(), Ci, Co, 2 * u, u) == 0
        assert dll.dmel_conv_transpose1d_set_precision(h, args.precision) == 0
        hs.append(h)
    ys = [torch.empty(B, Co, T * u, device=dev) for _ in libs]

    def run(i):
        rc = libs[i].dmel_conv_transpose1d_forward(hs[i], x.data_ptr(), ys[i].data_ptr(), B, T, st)
        assert rc == 0, (names[i], rc)

    for i in range(len(libs)):
        for _ in range(3):
            run(i)
    us = [[] for _ in libs]
    for _ in range(args.rounds):
        for i in range(len(libs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            us[i].append(e0.elapsed_time(e1) / args.iters * 1e3)
    flop = 2.0 * B * T * (Co * u) * (2 * Ci)           # two taps per output sample
    byts = 4.0 * B * T * (Ci + Co * u)
    for i, name in enumerate(names):
        med = statistics.median(us[i])
        print(f"Cin={Ci:4d} Cout={Co:4d} T={T:6d} u={u}  {med:7.1f} us  {flop / med / 1e6:6.1f} TFLOP/s  {byts / med / 1e3:7.1f} GB/s"
              f"  [{min(us[i]):.1f} .. {max(us[i]):.1f}]" + (f"  {name}" if args.lib else ""), flush=True)
    for i in range(1, len(libs)):
        print(f"           outputs of {names[i]} torch.equal to {names[0]}: {torch.equal(ys[i], ys[0])}", flush=True)
    for dll, h in zip(libs, hs):
        dll.dmel_conv_transpose1d_destroy(h)
