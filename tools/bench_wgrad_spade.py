"""Times single weight-gradient calls (cgan_conv2d_nhwc_bwd_weight with bias gradient and workspace: zero fill, main kernel,
channel sum where it is separate, split reduce) of the SPADE gamma|beta layers at the batch slices the joint train step
runs them at, plus the two 160^2 layers that meet the column-walking kernel's preconditions without being SPADE layers.
bf16, 2 warm-up and 5 event-timed calls per shape: median [min .. max] in us.

usage: [CGAN_LIB=other/libcgan_hip.so] python tools/bench_wgrad_spade.py [--tile K] [--only SUBSTR]
  --tile K: development build with cgan_debug_set_wgrad_tile3x3(K) (0 never tiled, 2 tiled wherever one applies, 3 the
  column-walking kernel on every shape that meets its preconditions); without it the product build and its own plan."""
import argparse
import ctypes
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from climategan_amd import _lib, ops  # noqa: E402

SHAPES = [(20, 640, 128, 80), (12, 640, 128, 80), (20, 640, 128, 40), (12, 640, 128, 40), (32, 320, 128, 160),
          (32, 320, 128, 80), (32, 160, 128, 320), (32, 160, 128, 160), (64, 160, 64, 64), (64, 160, 128, 32), (32, 160, 64, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=-1)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if args.tile >= 0:
        _lib.load_dev().cgan_debug_set_wgrad_tile3x3(ctypes.c_int(args.tile))
    for n, hw, ci, co in SHAPES:
        name = "n%d %d^2 c%d->c%d" % (n, hw, ci, co)
        if args.only not in name:
            continue
        x = ops.NHWC((torch.rand(n, hw, hw, ci, device="cuda") - 0.5).to(torch.bfloat16), ci)
        dy = ops.NHWC((torch.rand(n, hw, hw, co, device="cuda") - 0.5).to(torch.bfloat16), co)
        for _ in range(2):
            ops.conv2d_bwd_weight(x, dy, (co, ci, 3, 3), pad=1)
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.conv2d_bwd_weight(x, dy, (co, ci, 3, 3), pad=1)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        print("%s: med %.0f [%.0f .. %.0f] us" % (name, ts[2], ts[0], ts[4]), flush=True)
        del x, dy


if __name__ == "__main__":
    main()
