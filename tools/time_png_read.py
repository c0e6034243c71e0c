"""Time reading a batch of PNG files of the training loaders' four kinds, three ways:

  device      file bytes -> ``png.decode`` (device decoder: one upload of the zlib streams, one wave per file); upload inside
  host        ``PIL.Image.open`` + ``np.asarray`` file after file, each array uploaded
  host_pool   the same from a 16-thread pool

usage: python tools/time_png_read.py [--reps 9] [--warmup 2] [--json profiles/png_read.json] [--quick]

The kinds are generated, written by PIL at its default level: ``x`` photo-like RGB, ``s`` RGBA flat-colour regions, ``d`` RGB
with a smooth depth coded the way Unity's depth files are (the value spread over the three channels), ``m`` a grey binary
mask; each at 640 x 640 and at 1200 x 1800, in batches of 16 and of 128 files.  ``noise`` is DESIGN 4.18's test data: the four
files of a sample as noise written at ``compress_level=1``, at 640 x 640.  A batch cycles through 8 distinct files per kind and
size.  Every repetition of every path starts from the files' bytes in host memory and ends when every image is on the device;
the paths alternate inside each repetition, each timed with events behind a synchronisation, and the medians are reported with
their minimum and maximum.  The three results are compared file by file and must be equal.
"""
import argparse
import io
import json
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

THREADS, DISTINCT = 16, 8
SIZES = ((640, 640), (1200, 1800))
BATCHES = (16, 128)


def make(kind, h, w, seed):
    """One generated image of a loader kind: uint8 [h, w, 3 | 4] or [h, w] (grey)."""
    rng = np.random.default_rng(1000 * seed + h)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "x":                                          # photo-like: gradients, rectangles, texture and sensor noise
        a = np.stack([xx * 200.0 / w + 30, yy * 180.0 / h + 40, (xx + yy) * 160.0 / (h + w) + 50], axis=-1)
        for _ in range(6):
            y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 40))
            a[y0:y0 + int(rng.integers(20, h // 3)), x0:x0 + int(rng.integers(20, w // 3))] += rng.normal(0, 40, 3)
        a += 10 * np.sin(xx / (4.0 + seed) + yy / 7.0)[..., None] + rng.normal(0, 5, (h, w, 3))
        return np.clip(a, 0, 255).astype(np.uint8)
    if kind in ("s", "m"):                                   # regions: the nearest of a few seeds, as flat colours or as 0 / 255
        n = 12
        sy, sx = rng.integers(0, h, n), rng.integers(0, w, n)
        near = np.argmin((yy[..., None] - sy) ** 2 * 3 + (xx[..., None] - sx) ** 2, axis=-1)
        if kind == "m":
            return ((near % 2) * 255).astype(np.uint8)
        colours = rng.integers(0, 256, (n, 4)).astype(np.uint8)
        colours[:, 3] = 255
        return colours[near]
    if kind == "d":                                          # a smooth depth in 24 bits, spread over R, G, B
        depth = (yy / h) ** 2 * 0.8 + 0.1 * np.sin(xx / (40.0 + seed)) * (yy / h) + 0.1
        v = np.clip(depth, 0, 1) * (2 ** 24 - 1)
        v = v.astype(np.uint32)
        return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8)
    raise ValueError(kind)


def png_bytes(a, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG", **kw)
    return b.getvalue()


def event_timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1000.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    ap.add_argument("--quick", action="store_true", help="640 x 640 and batches of 16 only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_png_read: needs the GPU (nothing here can be timed on a CPU)")
    from PIL import Image

    from climategan_amd import png

    pool = ThreadPoolExecutor(THREADS)

    def read(data):
        a = np.asarray(Image.open(io.BytesIO(data)))
        return torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to("cuda")

    cases = []
    for h, w in (SIZES[:1] if args.quick else SIZES):
        for kind in ("x", "s", "d", "m"):
            cases.append((kind, h, w, [png_bytes(make(kind, h, w, i)) for i in range(DISTINCT)]))
        if (h, w) == SIZES[0]:
            rng = np.random.default_rng(5)
            noise = [png_bytes(rng.integers(0, 256, (h, w) + c, dtype=np.uint8), compress_level=1)
                     for _ in range(DISTINCT // 4) for c in ((3,), (4,), (3,), ())]
            cases.append(("noise", h, w, noise))
    records = []
    for kind, h, w, distinct in cases:
        for batch in (BATCHES[:1] if args.quick else BATCHES):
            files = [distinct[i % len(distinct)] for i in range(batch)]
            result = {}
            runs = {"device": lambda: result.__setitem__("device", png.decode(files)),
                    "host": lambda: result.__setitem__("host", [read(f) for f in files]),
                    "host_pool": lambda: result.__setitem__("host_pool", list(pool.map(read, files)))}
            times = {k: [] for k in runs}
            for rep in range(args.warmup + args.reps):
                for k, fn in runs.items():
                    t = event_timed(fn)
                    if rep >= args.warmup:
                        times[k].append(t)
            for a, b, c in zip(result["device"], result["host"], result["host_pool"]):
                assert torch.equal(a, b) and torch.equal(b, c), (kind, h, w, batch)
            rec = {"kind": kind, "shape": [h, w], "batch": batch, "file_bytes_mean": sum(map(len, files)) / batch,
                   "raw_bytes_mean": sum(int(im.numel()) for im in result["host"]) / batch, "equal": True}
            for k in runs:
                rec[k] = {"ms_per_file": 1e3 * statistics.median(times[k]) / batch,
                          "ms_per_file_min_max": [1e3 * min(times[k]) / batch, 1e3 * max(times[k]) / batch]}
            rec["fastest"] = min(runs, key=lambda k: rec[k]["ms_per_file"])
            records.append(rec)
            print("%-5s %4d x %4d  batch %3d  %8.0f B/file   device %7.3f   host %7.3f   host_pool %7.3f ms/file   -> %s" % (
                kind, h, w, batch, rec["file_bytes_mean"], rec["device"]["ms_per_file"], rec["host"]["ms_per_file"],
                rec["host_pool"]["ms_per_file"], rec["fastest"]), flush=True)
    res = {"reps": args.reps, "warmup": args.warmup, "threads": THREADS, "distinct_files_per_case": DISTINCT,
           "launches_and_memsets_per_call": 4, "records": records}
    line = json.dumps(res)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()
