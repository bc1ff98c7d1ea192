"""Micro-benchmark of the anti-aliased snake kernel on the BigVGAN-base stage shapes (GPU only).

  python tools/bench_snake.py                                  the library of the tree
  python tools/bench_snake.py --lib A.so --lib B.so            A/B: the libraries take turns, --rounds times each per shape, on the same seeded
                                                               tensors; prints every round, the medians, and whether the outputs are torch.equal
  --odd                                                        also T + 1 of every shape (rows off the 16-byte boundary: the dword path)
  --iters N                                                    launches per timing (default 20; 1 for a counter pass under rocprofv3 --pmc)
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
ap.add_argument("--lib", action="append", default=[])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--odd", action="store_true")
args = ap.parse_args()


def snake_fn(path):
    if path is None:
        return _lib.lib().dmel_aa_snake_f32
    fn = C.CDLL(os.path.abspath(path)).dmel_aa_snake_f32
    fn.restype, fn.argtypes = _lib.PROTOTYPES["dmel_aa_snake_f32"]
    return fn


names = args.lib or [None]
fns = [snake_fn(p) for p in names]
dev = torch.device("cuda:0")
taps = ref_cpu.aa_filter12().view(-1).contiguous()
shapes = [(32, 256, 736), (32, 128, 5888), (32, 64, 11776), (32, 32, 23552)]
if args.odd:
    shapes += [(B, C_, T + 1) for (B, C_, T) in shapes]
for (B, C_, T) in shapes:
    g = torch.Generator(device=dev).manual_seed(T)
    x = torch.randn(B, C_, T, device=dev, generator=g)
    al, be = torch.randn(C_, device=dev, generator=g) * 0.3, torch.randn(C_, device=dev, generator=g) * 0.3
    st = _lib.stream_ptr()
    ys = [torch.empty_like(x) for _ in fns]

    def run(i):
        rc = fns[i](x.data_ptr(), ys[i].data_ptr(), al.data_ptr(), be.data_ptr(), taps.data_ptr(), taps.data_ptr(), 1, B, C_, T, st)
        assert rc == 0, (names[i], rc)

    for i in range(len(fns)):
        for _ in range(3):
            run(i)
    us = [[] for _ in fns]
    for _ in range(args.rounds):
        for i in range(len(fns)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            us[i].append(e0.elapsed_time(e1) / args.iters * 1e3)
    for i, name in enumerate(names):
        med = statistics.median(us[i])
        print(f"C={C_:4d} T={T:6d}  {med:7.1f} us  {8.0 * B * C_ * T / med / 1e3:7.1f} GB/s"
              + (f"  [{min(us[i]):.1f} .. {max(us[i]):.1f}]  {name}" if args.lib else ""), flush=True)
    for i in range(1, len(fns)):
        print(f"           outputs of {names[i]} torch.equal to {names[0]}: {torch.equal(ys[i], ys[0])}", flush=True)
