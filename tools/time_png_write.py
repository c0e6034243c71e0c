"""Time the "write" stage of apply_events for one batch of 16 outputs of 640 x 640 x 3: ``png.write`` (device encoder) at
level 1 (``gpu``) and at level 2 (``gpu_level2``: per-row dynamic Huffman / stored blocks) against ``PIL.Image.save`` from a
16-thread pool at PIL's default level and at ``compress_level=1``.

usage: python tools/time_png_write.py [--out DIR] [--reps 9] [--warmup 2] [--json FILE]

The images are real outputs: the small checkpoint's (tests/golden/ckpt_small options, every inference task, random
weights) ``infer_all`` floods of generated photos -- noise alone would be unrepresentative.  Every repetition of every path
starts from the same uint8 images where that path finds them (the device for ``png.write``, host arrays for PIL: the
device-to-host copy of the raw pixels PIL needs is timed separately and reported, not added), writes 16 files and ends when
the last file is closed; the four paths alternate inside each repetition and the medians are reported.  Prints seconds per
image and bytes per image for all four, the size ratios level 2 / level 1 and level 2 / PIL default, and one JSON line.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, SIZE, THREADS = 16, 640, 16


def photos(n, size, seed=0):
    """Generated photos: sky / ground gradients, a few rectangles, mild noise."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = int(rng.integers(size, 2 * size)), int(rng.integers(size, 2 * size))
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([80 + 100 * yy / h, 120 + 60 * xx / w, 200 - 120 * yy / h], axis=-1)
        for _ in range(12):
            y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
            img[y0:y0 + int(rng.integers(20, h // 2)), x0:x0 + int(rng.integers(20, w // 2))] = rng.integers(0, 256, 3)
        out.append(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))
    return out


def outputs():
    """uint8 [16, 640, 640, 3] on the device: flood images of the small model."""
    import yaml

    from climategan_amd import ops
    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.config import Opts
    from climategan_amd.trainer import Trainer

    o = Opts(yaml.safe_load((ROOT / "tests" / "golden" / "ckpt_small" / "opts.yaml").read_text()))
    o.tasks = ["d", "s", "m", "p"]
    T = Trainer(o, device="cuda").setup(inference=True)
    x = prepare_batch(photos(BATCH, SIZE), to=SIZE)
    ev = T.infer_all(x, numpy=False, bin_value=0.5, cloudy=False)
    return torch.cat([ops.normalize_to_uint8(ev[k]) for k in ("flood", "smog", "wildfire")])[
        torch.arange(0, 3 * BATCH, 3)].contiguous()      # a mix of the three events, 16 images


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def setup(doc, name):
    """What both write-timing tools start with -> (args, uint8 batch on the device, the same as a host array, output
    directory, its TemporaryDirectory or None, the PIL thread pool)."""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--out", default=None, help="directory to write into (default: a temporary one)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("%s: needs the GPU (nothing here can be timed on a CPU)" % name)
    dev = outputs()
    tmp = tempfile.TemporaryDirectory() if args.out is None else None
    out = Path(tmp.name if tmp else args.out)
    out.mkdir(parents=True, exist_ok=True)
    return args, dev, dev.cpu().numpy(), out, tmp, ThreadPoolExecutor(THREADS)


def measure(args, dev, runs, paths, **extra):
    """The paths of ``runs`` alternating inside each repetition, the raw device-to-host copy timed beside them -> the result
    dictionary: per path the median, minimum and maximum seconds per image and the bytes per image of its files."""
    times = {k: [] for k in runs}
    d2h = []
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():
            t = timed(fn)
            if rep >= args.warmup:
                times[k].append(t)
        t = timed(lambda: dev.cpu())
        if rep >= args.warmup:
            d2h.append(t)
    res = {"batch": BATCH, "shape": [SIZE, SIZE, 3], **extra, "reps": args.reps, "threads": THREADS,
           "raw_d2h_s_per_image": statistics.median(d2h) / BATCH}
    for k in runs:
        res[k] = {"s_per_image": statistics.median(times[k]) / BATCH,
                  "s_per_image_min_max": [min(times[k]) / BATCH, max(times[k]) / BATCH],
                  "bytes_per_image": sum(p.stat().st_size for p in paths[k]) / BATCH}
    return res


def finish(args, res, tmp, pool):
    line = json.dumps(res)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")
    pool.shutdown()
    if tmp:
        tmp.cleanup()


def main():
    args, dev, host, out, tmp, pool = setup(__doc__, "time_png_write")
    from PIL import Image

    from climategan_amd import png

    paths = {k: [out / ("%s_%02d.png" % (k, i)) for i in range(BATCH)] for k in ("gpu", "gpu_level2", "pil_default", "pil_level1")}

    def pil(kind, **kw):
        list(pool.map(lambda ip: Image.fromarray(ip[0]).save(ip[1], **kw), zip(host, paths[kind])))

    runs = {"gpu": lambda: png.write(dev, paths["gpu"]),
            "gpu_level2": lambda: png.write(dev, paths["gpu_level2"], level=2),
            "pil_default": lambda: pil("pil_default"),
            "pil_level1": lambda: pil("pil_level1", compress_level=1)}
    res = measure(args, dev, runs, paths)
    for i in range(BATCH):                                   # the device files hold the same pixels
        assert np.array_equal(np.asarray(Image.open(paths["gpu"][i])), host[i]), i
        assert np.array_equal(np.asarray(Image.open(paths["gpu_level2"][i])), host[i]), i
    for k in runs:
        print("%-12s %.6f s/image (min %.6f, max %.6f)  %.0f bytes/image" % (
            k, res[k]["s_per_image"], *res[k]["s_per_image_min_max"], res[k]["bytes_per_image"]))
    res["size_ratio_gpu_over_pil_default"] = res["gpu"]["bytes_per_image"] / res["pil_default"]["bytes_per_image"]
    res["size_ratio_level2_over_level1"] = res["gpu_level2"]["bytes_per_image"] / res["gpu"]["bytes_per_image"]
    res["size_ratio_level2_over_pil_default"] = res["gpu_level2"]["bytes_per_image"] / res["pil_default"]["bytes_per_image"]
    res["speedup_level2_over_level1"] = res["gpu"]["s_per_image"] / res["gpu_level2"]["s_per_image"]
    print("size: level 2 / level 1 = %.4f, level 2 / PIL default = %.4f" % (
        res["size_ratio_level2_over_level1"], res["size_ratio_level2_over_pil_default"]))
    res["speedup_gpu_over_pil_default"] = res["pil_default"]["s_per_image"] / res["gpu"]["s_per_image"]
    res["speedup_gpu_over_pil_level1"] = res["pil_level1"]["s_per_image"] / res["gpu"]["s_per_image"]
    finish(args, res, tmp, pool)


if __name__ == "__main__":
    main()
