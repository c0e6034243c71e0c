"""Time the masker evaluation at 640^2 with device events: (a) the metric stage alone (one ``eval_metrics.masker_eval``
call per batch: six launches + one device-to-host copy) and (b) the full loop of ``python -m climategan_amd.eval_masker``
per batch (prepare_batch, G.mask, masker_eval), for batch sizes 1, 16 and 64.  Prints one JSON line.

    python tools/bench_eval_masker.py [--iters 10] [--warmup 3] [--dtype bf16|fp16|split24] [--batches 1,16,64]

``metric_gbps`` = the bytes the metric kernels must move at least (inputs once, the edge masks, the column-distance map
and the squared distances of the edge pixels written and read once) over the metric stage's time.  The Masker has the
default configuration with torch's default weights: the mask values do not matter for the timing, the edge pixel count
(reported) does.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from climategan_amd import eval_metrics as em  # noqa: E402
from climategan_amd.apply_events import prepare_batch  # noqa: E402
from climategan_amd.config import default_opts  # noqa: E402
from climategan_amd.trainer import Trainer  # noqa: E402

LAUNCHES = 6          # csrc/masker_eval.hip: counts, finish, columns, rows, variance, final


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=("fp16", "bf16", "split24"))
    ap.add_argument("--batches", default="1,16,64")
    args = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    o = default_opts()
    o.tasks = ["m"]
    T = Trainer(o, device="cuda").setup(inference=True)
    T.G.set_compute_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}.get(args.dtype, args.dtype))
    yy, xx = np.mgrid[0:640, 0:640]
    result = {"what": "eval_masker metric stage and full loop, 640x640", "dtype": args.dtype, "launches_per_batch": LAUNCHES,
              "batches": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        imgs = [rng.integers(0, 256, size=(720, 960, 3)).astype(np.uint8) for _ in range(n)]
        lab = np.zeros((n, 640, 640), np.int64)
        for i in range(n):
            r = rng.uniform(100, 250)
            lab[i][(yy - rng.uniform(200, 440)) ** 2 + (xx - rng.uniform(200, 440)) ** 2 < r * r] = 1
            lab[i][:, :80] = 2
        label = torch.from_numpy(lab).to(torch.uint8).cuda()
        # the metric stage on a blob mask offset from the label (a trained Masker's kind of output) and on uniform noise
        # (the worst case: about half the pixels are prediction edges)
        blob = np.zeros((n, 640, 640), np.float32)
        for i in range(n):
            r = rng.uniform(100, 250)
            blob[i] = 1.0 / (1.0 + np.exp(-(r * r - (yy - rng.uniform(200, 440)) ** 2 - (xx - rng.uniform(200, 440)) ** 2)
                                          / 2000.0))
        mask = torch.from_numpy(blob).cuda()
        noise = torch.rand((n, 640, 640), device="cuda")
        r = em.masker_eval(mask, label, bin_value=0.5)
        pe_px = int(r["pred_edge_pixels"].sum())
        metric_ms = timed(lambda: em.masker_eval(mask, label, bin_value=0.5), args.iters, args.warmup)
        noise_ms = timed(lambda: em.masker_eval(noise, label, bin_value=0.5), args.iters, args.warmup)

        def full():
            with torch.no_grad():
                m = T.G.mask(x=prepare_batch(imgs))[:, 0].float().contiguous()
            em.masker_eval(m, label, bin_value=0.5)

        full_ms = timed(full, max(1, args.iters // 2), 1)
        npix = n * 640 * 640
        nbytes = npix * (4 + 1) + npix * 2 + npix * 1 + npix * 4 * 2 + npix * 1 + pe_px * 4 * 2 + npix * 1
        result["batches"][str(n)] = {
            "metric_ms_per_image": metric_ms / n, "full_ms_per_image": full_ms / n, "metric_images_per_s": 1e3 * n / metric_ms,
            "full_images_per_s": 1e3 * n / full_ms, "metric_share_of_full": metric_ms / full_ms,
            "metric_noise_ms_per_image": noise_ms / n, "pred_edge_pixels_per_image": pe_px / n, "metric_bytes": nbytes, "metric_gbps": nbytes / (metric_ms * 1e6)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
