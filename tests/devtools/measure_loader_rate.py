"""Batches per second of ``OmniLoader`` alone (GPU box; a devtool, not a test and not part of bench.py).

    python tests/devtools/measure_loader_rate.py [--samples 128] [--epochs 4]

Writes 16 synthetic 640 x 640 samples of the simulated domain (x RGB PNG, s RGBA PNG, d Unity-coded PNG, m grey PNG) into a
temporary directory, lists them ``--samples`` times, and iterates the default pipeline (defaults.yaml's transforms, tasks
d, s, m, p) at batch sizes 4 and 32 with 16 reader threads and prefetch on: one warm-up epoch, then the median over the timed
epochs of batches / second, each epoch closed by a device synchronisation.  Next to it: where a batch's host time goes
(``loader.times``), what one file costs a single thread (read, decode), and the rate the training step of the latest
BENCH_*.json headline consumes -- three domain batches per step."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import data_decode_cases as cases  # noqa: E402
from loader_fixture import palette_rgba  # noqa: E402

SIZE, DISTINCT = 640, 16


def write_files(root):
    from PIL import Image
    from climategan_amd import data
    samples = []
    for k in range(DISTINCT):
        tag = "rate.%d" % k
        arrays = {"x": cases.x_image(tag + ".x", SIZE, SIZE), "m": cases.mask(tag + ".m", 255, h=SIZE, w=SIZE),
                  "d": cases.unity(tag + ".d", SIZE, SIZE), "s": palette_rgba(tag + ".s", data.classes_dict["s"], SIZE, SIZE)}
        paths = {}
        for task, arr in arrays.items():
            paths[task] = str(root / ("%s%d.png" % (task, k)))
            Image.fromarray(arr).save(paths[task], compress_level=1)
        samples.append(paths)
    return samples


def headline():
    found = sorted(ROOT.glob("BENCH_*.json"))
    if not found:
        return None
    parsed = json.loads(found[-1].read_text()).get("parsed") or {}
    return {"file": found[-1].name, "ms_per_step": parsed.get("ms_per_step"), "images_per_s": parsed.get("value"),
            "batch_per_domain": (parsed.get("config") or {}).get("batch_per_domain_per_gpu")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=4)
    args = ap.parse_args()
    from climategan_amd import data
    from climategan_amd.train import train_defaults

    bench = headline()
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        samples = write_files(root)
        (root / "train_s.json").write_text(json.dumps([samples[i % DISTINCT] for i in range(args.samples)]))
        # one file, one thread: bytes from the page cache, then the decode (PNG inflate + numpy)
        from PIL import Image
        for task in ("x", "s", "d", "m"):
            t_read, t_dec = [], []
            for s in samples:
                t0 = time.perf_counter()
                Path(s[task]).read_bytes()
                t1 = time.perf_counter()
                np.array(Image.open(s[task]))
                t_read.append(t1 - t0)
                t_dec.append(time.perf_counter() - t1)
            print("file %s: %.0f KiB, read %.2f ms, read + decode %.2f ms (one thread, median of %d)"
                  % (task, Path(samples[0][task]).stat().st_size / 1024, 1e3 * statistics.median(t_read),
                     1e3 * statistics.median(t_dec), DISTINCT))
        for bs in (4, 32):
            opts = train_defaults()
            opts.data.files = {"base": str(root), "train": {"s": "train_s.json"}}
            opts.data.loaders = {"batch_size": bs, "num_workers": 16}
            loader = data.get_loader("train", "s", opts, prefetch=1, device="cuda:0")
            rates = []
            for epoch in range(args.epochs + 1):
                if epoch == 1:
                    loader.times = {k: 0 for k in loader.times}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for batch in loader:
                    n += 1
                torch.cuda.synchronize()
                if epoch:                                # the first epoch warms the caches, the pool and the allocator
                    rates.append(n / (time.perf_counter() - t0))
            loader.close()
            t = loader.times
            per = {k: 1e3 * t[k] / max(t["batches"], 1) for k in ("read", "stage", "transform")}
            line = {"batch_size": bs, "threads": loader.num_workers, "batches_per_s_median": round(statistics.median(rates), 2),
                    "batches_per_s_all": [round(r, 2) for r in rates], "images_per_s": round(bs * statistics.median(rates), 1),
                    "host_ms_per_batch": {k: round(v, 2) for k, v in per.items()}}
            if bench and bench["images_per_s"]:
                need = 3.0 * bench["images_per_s"] / bs         # three domain batches per step at the headline's image rate
                line["step_needs_batches_per_s"] = round(need, 2)
                line["loader_over_step"] = round(statistics.median(rates) / need, 2)
            print(json.dumps(line))
    print("headline:", json.dumps(bench))


if __name__ == "__main__":
    main()
