"""Time the loaders' decode + default transform pipeline from RAW sources (sim domain: Unity depth code, RGBA segmentation
image, uint8 mask, uint8 image without known min / max; sizes around 1200 x 1800) for batch sizes 1, 4 and 32.  Prints one
JSON line.

    python tools/bench_data_decode.py [--window-ms 300] [--warmup 3] [--repeats 5] [--batches 1,4,32] [--normalize]

Per batch size, in ms per sample (median of ``--repeats`` event-timed windows, the variants alternating; the spread is the
min and max of those windows, as in tools/bench_data_transforms.py):
  raw     ``RawSource``s through ``compile_transforms``: the decode inside the one gather per task (plus two min / max
          launches for x, and for d with ``--normalize``)
  torch   what one does without the raw kinds: the same device arrays decoded step by step with torch ops (tensor_loader's
          algorithm restated; the palette lookup as eleven masked updates in class order), then ``compile_transforms`` on the
          decoded tensors
  host    for the record, one run, wall clock: the numpy decode of tensor_loader restated (the palette lookup vectorised --
          the reference's per-pixel Python loop takes minutes per image) and the upload of the fp32 results
``uploaded_bytes_per_sample``: the raw arrays against the decoded fp32 tensors.  ``share_of_train_step``: against one train
step's time per sample (564 ms / 64, README).  Before anything is timed ``raw`` and ``torch`` run on the same draws and must
agree -- d, m, s in every element, x within the 4e-6 of tests/test_gpu_data_transforms.py -- or the tool exits with status 1
and prints no timing.
"""
import argparse
import json
import math
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_data_transforms import ITEMS, SIZES, TRAIN_STEP_MS_PER_SAMPLE, window_ms  # noqa: E402
from climategan_amd import data  # noqa: E402
from climategan_amd import transforms as T  # noqa: E402
from climategan_amd.config import Opts  # noqa: E402

FAR = 1000.0


def make_arrays(n):
    """per sample {task: raw uint8 device array}"""
    g = torch.Generator(device="cuda").manual_seed(0)
    cols = torch.tensor(list(data.classes_dict["s"].values()), dtype=torch.uint8, device="cuda")
    out = []
    for k in range(n):
        h, w = SIZES[k % len(SIZES)]
        u8 = lambda *shape, hi=256: torch.randint(0, hi, shape, device="cuda", generator=g, dtype=torch.uint8)   # noqa: E731
        d = torch.cat([u8(h, w, 2, hi=248), u8(h, w, 1, hi=255)], dim=2)          # never code 0: 1 / depth stays finite
        s = cols[u8(h, w, hi=11).long()]
        noisy = u8(h, w) > 127
        s[noisy] = s[noisy] ^ (u8(h, w, 4, hi=64)[noisy])
        out.append({"x": 10 + u8(h, w, 3, hi=240), "m": u8(h, w, hi=2) * 255, "d": d, "s": s})
    return out


def raw_samples(arrays, normalize):
    pal = data.nearest_palette("s")
    return [{"x": T.RawSource(a["x"], "x"), "m": T.RawSource(a["m"], "mask"),
             "d": T.RawSource(a["d"], "unity_d", far=FAR, normalize=normalize),
             "s": T.RawSource(a["s"], "palette_s", palette=pal)} for a in arrays]


def torch_decode(a, normalize):
    """tensor_loader, restated with torch ops on the device"""
    x = a["x"].float()
    x = x - x.min()
    x = (x / x.max()).permute(2, 0, 1).unsqueeze(0)
    m = a["m"].float()
    if m.max() > 127:
        m = (m > 127).float()
    r, g, b = (a["d"][:, :, k].float() for k in range(3))
    code = ((247 - r) / 8).int() * (256 * 31) + ((247 - g) / 8).int() * 256 + (255 - b).int()
    # the divisor as a device tensor: torch's GPU division by a Python scalar multiplies by its reciprocal, which is not the
    # reference's (CPU) IEEE division and differs from it by an ulp
    d = 1 / (code.float() / torch.tensor(256 * 31 * 31 - 1.0, device=r.device) * FAR)
    if normalize:
        d = d - d.min()
        d = d / d.max()
    px = a["s"].int()
    best = torch.full(px.shape[:2], 1 << 30, dtype=torch.int32, device=px.device)
    s = torch.zeros(px.shape[:2], dtype=torch.float32, device=px.device)
    for cls, col in data.classes_dict["s"].items():
        dist = ((px - torch.tensor(col, dtype=torch.int32, device=px.device)) ** 2).sum(-1, dtype=torch.int32)
        closer = dist < best
        best = torch.where(closer, dist, best)
        s = torch.where(closer, float(cls), s)
    return {"x": x, "m": m[None, None], "d": d[None, None], "s": s[None, None]}


def host_decode(a, normalize):
    """tensor_loader in numpy on the host, then the upload"""
    x = a["x"].astype(np.float32)
    x -= x.min()
    x /= x.max()
    m = a["m"].astype(np.float32)
    if m.max() > 127:
        m = (m > 127).astype(np.float32)
    t = a["d"].astype(np.float32)
    code = ((247 - t[..., 0]) / 8).astype(np.int32) * (256 * 31) + ((247 - t[..., 1]) / 8).astype(np.int32) * 256 \
        + (255 - t[..., 2]).astype(np.int32)
    d = 1 / (code.astype(np.float32) / np.float32(256 * 31 * 31 - 1) * np.float32(FAR))
    if normalize:
        d = d - d.min()
        d = d / d.max()
    cols = np.array(list(data.classes_dict["s"].values()), np.int32)
    px = a["s"].astype(np.int32)
    dist = np.stack([((px - c) ** 2).sum(-1) for c in cols])
    s = dist.argmin(0).astype(np.float32)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
            {"x": np.moveaxis(x, 2, 0)[None], "m": m[None, None], "d": d[None, None], "s": s[None, None]}.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,4,32")
    ap.add_argument("--normalize", action="store_true", help="min-max normalise d (train.pseudo.tasks holds d)")
    args = ap.parse_args()
    np.random.seed(0)       # the timed crops and flips come from the global generators: two builds time the same windows
    random.seed(0)
    opts = Opts({"tasks": ["d", "s", "m", "p"], "data": {"transforms": ITEMS}})
    batch = T.compile_transforms(opts, "train", "s", draws=T.PipelineDraws())
    result = {"what": "decode + default loader transforms from raw sim-domain sources around 1200x1800, tasks d s m x",
              "normalize_d": args.normalize, "window_ms": args.window_ms, "repeats": args.repeats, "batches": {}}
    for n in [int(b) for b in args.batches.split(",")]:
        arrays = make_arrays(n)
        raws = raw_samples(arrays, args.normalize)
        variants = {"raw": lambda: batch(raws),
                    "torch": lambda: batch([torch_decode(a, args.normalize) for a in arrays])}
        np.random.seed(1)
        a = variants["raw"]()
        np.random.seed(1)
        b = variants["torch"]()
        agree = {k: float((a[k].float() - b[k].float()).abs().max()) for k in a}
        if any(not v <= (4e-6 if k == "x" else 0.0) for k, v in agree.items()):
            sys.exit("bench_data_decode: the raw and the torch variant disagree at batch %d (max |diff| %s): nothing timed"
                     % (n, agree))
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        iters = {k: max(5, math.ceil(args.window_ms / window_ms(fn, 5))) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(window_ms(fn, iters[k]) / n)
        med = {k: statistics.median(v) for k, v in times.items()}
        host_arrays = [{k: v.cpu().numpy() for k, v in s.items()} for s in arrays[:min(n, 2)]]
        t0 = time.perf_counter()
        decoded = [host_decode(s, args.normalize) for s in host_arrays]
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3 / len(host_arrays)
        raw_bytes = sum(v.numel() * v.element_size() for s in arrays for v in s.values()) / n
        fp32_bytes = sum(v.numel() * v.element_size() for s in decoded for v in s.values()) / len(decoded)
        spread = max(max(times[k]) - min(times[k]) for k in times)
        result["batches"][str(n)] = {
            "raw_ms_per_sample": med["raw"], "raw_min_max": [min(times["raw"]), max(times["raw"])],
            "torch_ms_per_sample": med["torch"], "torch_min_max": [min(times["torch"]), max(times["torch"])],
            "host_decode_upload_ms_per_sample": host_ms, "runs_per_window": iters,
            "torch_over_raw": med["torch"] / med["raw"], "raw_not_slower_within_spread": med["raw"] <= med["torch"] + spread,
            "uploaded_bytes_per_sample": {"raw": raw_bytes, "decoded_fp32": fp32_bytes},
            "raw_share_of_train_step": med["raw"] / TRAIN_STEP_MS_PER_SAMPLE,
            "torch_share_of_train_step": med["torch"] / TRAIN_STEP_MS_PER_SAMPLE, "max_abs_diff_raw_vs_torch": agree}
        del arrays, raws, a, b, decoded
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
