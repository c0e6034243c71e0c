"""Time the loaders' default transform pipeline (defaults.yaml:43-67: hflip, resize 640 keeping the aspect ratio, crop 600,
resize {default 640, d 160, s 160}, Normalize; tasks d s m p, train mode) on synthetic sources of mixed sizes around
1200 x 1800, for batch sizes 1, 4 and 32.  Prints one JSON line.

    python tools/bench_data_transforms.py [--window-ms 400] [--warmup 3] [--repeats 5] [--batches 1,4,32]

Per batch size, in ms per sample (median of ``--repeats`` event-timed windows, each of as many runs as fill about
``--window-ms`` of device time -- a window of a few milliseconds measures the clock and the scheduler --, the two variants
alternating; the spread is the min and max of those windows):
  fused   ``transforms.compile_transforms``: the draws and plans on the host, one launch per task for the whole batch
  torch   the yardstick: the reference's algorithm step by step with torch ops on the same GPU, sample by sample
          (``torch.flip``, ``F.interpolate``, slicing, ``F.interpolate``, the normalisation, ``torch.stack``), same draws
``fused_gbps``: the bytes the fused launches must move -- each output once, and the rectangle of each source the final crop
looks at once -- over the fused time; ``share_of_stream_rate``: against the 5.5 TB/s the repository's streaming kernels
reach.  ``share_of_train_step``: against one train step's time per sample (564 ms / 64, README).
Before anything is timed the two variants run on the same draws and must agree -- d, m, s in every element, x within the
4e-6 of tests/test_gpu_data_transforms.py -- or the tool exits with status 1 and prints no timing.
"""
import argparse
import json
import math
import random
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from climategan_amd import transforms as T  # noqa: E402
from climategan_amd.config import Opts  # noqa: E402

SIZES = [(1200, 1800), (1080, 1920), (1800, 1200), (1365, 2048), (1024, 1024), (1200, 1600)]
STREAM_TBPS = 5.5
TRAIN_STEP_MS_PER_SAMPLE = 564.0 / 64
ITEMS = [{"name": "hflip", "ignore": "val", "p": 0.5},
         {"name": "resize", "ignore": False, "new_size": 640, "keep_aspect_ratio": True},
         {"name": "crop", "ignore": False, "center": "val", "height": 600, "width": 600},
         {"name": "resize", "ignore": False, "new_size": {"default": 640, "d": 160, "s": 160}}]


def make_samples(n):
    g = torch.Generator(device="cuda").manual_seed(0)
    out = []
    for k in range(n):
        h, w = SIZES[k % len(SIZES)]
        out.append({"x": torch.rand((1, 3, h, w), device="cuda", generator=g),
                    "m": (torch.rand((1, 1, h, w), device="cuda", generator=g) > 0.5).float(),
                    "d": torch.rand((1, 1, h, w), device="cuda", generator=g) * 7,
                    "s": torch.randint(0, 11, (1, 1, h, w), device="cuda", generator=g).float()})
    return out


def torch_pipeline(samples, draws):
    """The reference's transforms, restated with torch ops on the device (the per-sample algorithm, then the collate)"""
    outs = {k: [] for k in samples[0]}
    for s in samples:
        d = dict(s)
        if not (draws.rand() > 0.5):
            d = {k: torch.flip(v, [3]) for k, v in d.items()}
        h, w = d["x"].shape[-2:]
        size = (640, int(640 * w / h)) if h < w else (int(640 * h / w), 640)
        d = {k: F.interpolate(v, size=size, **T.interpolation(k)) for k, v in d.items()}
        top, left = draws.randint(0, size[0] - 600), draws.randint(0, size[1] - 600)
        d = {k: v[:, :, top:top + 600, left:left + 600] for k, v in d.items()}
        d = {k: F.interpolate(v, size=(160, 160) if k in "ds" else (640, 640), **T.interpolation(k)) for k, v in d.items()}
        d["x"] = (d["x"] - 0.5) / 0.5
        for k, v in d.items():
            outs[k].append(v.squeeze(0))
    return {k: torch.stack(v) for k, v in outs.items()}


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def source_extent(plan):
    """(rows, cols) of the source rectangle a plan looks at: its corners walked down through the maps and stages (the
    maps are monotone; one pixel more per resampling stage for the bilinear neighbour)"""
    rows, cols = [0, plan.h - 1], [0, plan.w - 1]
    for k in range(len(plan.stages), -1, -1):
        r0, c0, step = plan.maps[k]
        rows, cols = [r0 + r for r in rows], [c0 + step * c for c in cols]
        if k:
            in_h, in_w, out_h, out_w = plan.stages[k - 1]
            rows = [min(int(r * in_h / out_h), in_h - 1) for r in rows]
            cols = [min(int(c * in_w / out_w), in_w - 1) for c in cols]
    return abs(rows[1] - rows[0]) + 1 + len(plan.stages), abs(cols[1] - cols[0]) + 1 + len(plan.stages)


def fused_bytes(batch, samples):
    """output bytes + the bytes of the source rectangles the plans look at (one draw of the crops)"""
    total = 0
    for s in samples:
        plans, _ = batch.plan_sample(s)
        for task, p in plans.items():
            rows, cols = source_extent(p)
            c, e = s[task].shape[1], s[task].element_size()
            total += c * e * rows * cols + c * e * p.h * p.w
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,4,32")
    args = ap.parse_args()
    np.random.seed(0)       # the timed crops and flips come from the global generators: two builds time the same windows
    random.seed(0)
    opts = Opts({"tasks": ["d", "s", "m", "p"], "data": {"transforms": ITEMS}})
    draws = T.PipelineDraws()
    batch = T.compile_transforms(opts, "train", "r", draws=draws)
    result = {"what": "default loader transforms, tasks d s m p, train, sources around 1200x1800", "window_ms": args.window_ms,
              "repeats": args.repeats, "batches": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        samples = make_samples(n)
        np.random.seed(1)
        a = batch(samples)
        np.random.seed(1)
        b = torch_pipeline(samples, draws)
        agree = {k: float((a[k].float() - b[k].float()).abs().max()) for k in a}       # same draws: the two must agree
        if any(v > (4e-6 if k == "x" else 0.0) for k, v in agree.items()):
            sys.exit("bench_data_transforms: the fused and the torch variant disagree at batch %d (max |diff| %s): "
                     "nothing timed" % (n, agree))
        variants = {"fused": lambda: batch(samples), "torch": lambda: torch_pipeline(samples, draws)}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        iters = {k: max(20, math.ceil(args.window_ms / window_ms(fn, 20))) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(window_ms(fn, iters[k]) / n)
        med = {k: statistics.median(v) for k, v in times.items()}
        nbytes = fused_bytes(batch, samples)
        result["batches"][str(n)] = {
            "fused_ms_per_sample": med["fused"], "fused_min_max": [min(times["fused"]), max(times["fused"])],
            "torch_ms_per_sample": med["torch"], "torch_min_max": [min(times["torch"]), max(times["torch"])],
            "runs_per_window": iters, "torch_over_fused": med["torch"] / med["fused"], "fused_samples_per_s": 1e3 / med["fused"],
            "fused_bytes_per_sample": nbytes / n, "fused_gbps": nbytes / n / (med["fused"] * 1e6),
            "share_of_stream_rate": nbytes / n / (med["fused"] * 1e6) / (STREAM_TBPS * 1e3),
            "fused_share_of_train_step": med["fused"] / TRAIN_STEP_MS_PER_SAMPLE,
            "torch_share_of_train_step": med["torch"] / TRAIN_STEP_MS_PER_SAMPLE, "max_abs_diff_fused_vs_torch": agree}
        del samples, a, b
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
