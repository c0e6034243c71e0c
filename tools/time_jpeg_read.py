"""Time the "data pre-processing" stage of apply_events for one batch of 16 JPEG photos of 1200 x 1800 x 3 (PIL's files of
``tools/time_png_write.py``'s generated photos: quality 90, 4:2:0, no restart markers), three ways:

  device      file bytes -> ``jpeg.decode`` (device decoder) -> ``prepare_batch``; the upload is inside
  host        what the command does without ``--decode device``: ``read_image`` file after file, then ``prepare_batch``
  host_pool   ``read_image`` from a 16-thread pool, then ``prepare_batch``

usage: python tools/time_jpeg_read.py [--reps 9] [--warmup 2] [--json profiles/jpeg_read.json]

Every repetition of every path starts from the files on disk and ends when the [16, 3, 640, 640] batch is complete on the
device; the paths alternate inside each repetition and the medians are reported with their minimum and maximum.  Also
recorded: the rounds the entropy decode's states need to their fixpoint (the host twin's count at the default subsequence
size, the largest over the files), the launches and memsets of the one decode call, and that the three batches are equal.
"""
import argparse
import json
import statistics
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

from time_png_write import BATCH, SIZE, THREADS, photos, timed  # noqa: E402

H, W, QUALITY = 1200, 1800, 90


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg_read: needs the GPU (nothing here can be timed on a CPU)")
    from PIL import Image

    import jpeg_decode_corpus as jc
    from climategan_amd import jpeg
    from climategan_amd.apply_events import prepare_batch, read_image

    tmp = tempfile.TemporaryDirectory()
    paths = []
    for i, img in enumerate(photos(BATCH, SIZE)):                    # 640 .. 1279 pixels a side: resized, then fine texture
        big = np.asarray(Image.fromarray(img).resize((W, H), Image.BICUBIC))
        yy, xx = np.mgrid[0:H, 0:W]
        tex = 12 * np.sin(xx / (3.0 + i) + yy / 5.0)[..., None] + np.random.default_rng(i).normal(0, 6, (H, W, 3))
        paths.append(Path(tmp.name) / ("photo_%02d.jpg" % i))
        Image.fromarray(np.clip(big + tex, 0, 255).astype(np.uint8)).save(paths[-1], "JPEG", quality=QUALITY, subsampling=2)
    pool = ThreadPoolExecutor(THREADS)
    result = {}

    def device():
        result["device"] = prepare_batch(jpeg.decode(paths), to=SIZE)

    def host():
        result["host"] = prepare_batch([read_image(p) for p in paths], to=SIZE)

    def host_pool():
        result["host_pool"] = prepare_batch(list(pool.map(read_image, paths)), to=SIZE)

    runs = {"device": device, "host": host, "host_pool": host_pool}
    times = {k: [] for k in runs}
    for rep in range(args.warmup + args.reps):
        for k, fn in runs.items():
            t = timed(fn)
            if rep >= args.warmup:
                times[k].append(t)
    datas = [p.read_bytes() for p in paths]
    rounds, tiles = [], []
    for data in datas:
        d, status, _ = jc.parse_host(data)
        _, status, r = jc.decode_host(data, d)
        assert status == 0
        rounds.append(r)
        tiles.append(-(-(-(-d.scan_bytes // 128)) // 256))
    res = {"batch": BATCH, "shape": [H, W, 3], "quality": QUALITY, "subsampling": "420", "reps": args.reps, "threads": THREADS,
           "file_bytes_per_image": sum(len(d) for d in datas) / BATCH, "raw_bytes_per_image": H * W * 3,
           "rounds_to_fixpoint_host_twin_max": max(rounds), "tiles_per_file_max": max(tiles),
           "launches_and_memsets_per_call": 2 + 1 + min(8, max(tiles)) + 4,
           "batches_equal": bool(torch.equal(result["device"], result["host"]) and torch.equal(result["host"], result["host_pool"]))}
    for k in runs:
        res[k] = {"s_per_image": statistics.median(times[k]) / BATCH,
                  "s_per_image_min_max": [min(times[k]) / BATCH, max(times[k]) / BATCH]}
        print("%-10s %.6f s/image (min %.6f, max %.6f)" % (k, res[k]["s_per_image"], *res[k]["s_per_image_min_max"]))
    res["speedup_device_over_host"] = res["host"]["s_per_image"] / res["device"]["s_per_image"]
    res["speedup_device_over_host_pool"] = res["host_pool"]["s_per_image"] / res["device"]["s_per_image"]
    line = json.dumps(res)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")
    pool.shutdown()
    tmp.cleanup()


if __name__ == "__main__":
    main()
