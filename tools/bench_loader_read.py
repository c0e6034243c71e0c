"""Time whole epochs of the training loaders with ``data.loaders.decode`` host against device.

usage: python tools/bench_loader_read.py [--large] [--forms pil repacked jpeg] [--samples 256] [--epochs 5]
                                         [--json profiles/loader_decode.json]

The data set is generated (``tools/time_png_read.py``'s kinds: ``x`` photo-like RGB, ``s`` RGBA regions, ``d`` Unity-coded depth
in RGB, ``m`` a grey binary mask; 640 x 640, 1200 x 1800 with ``--large``), 16 distinct samples listed cyclically, in three
forms: ``pil`` -- PIL's own PNG files; ``repacked`` -- the same files through ``repack_png`` (RGB and grey become row-framed,
RGBA is copied); ``jpeg`` -- ``x`` as quality-90 JPEG, the rest as ``pil``.  Loaders: domain ``s`` with the tasks d, s, m (four
files a sample) and domain ``rf`` with p (x and m); ``decode`` host with 16 reader threads against device with the same 16;
batches of 4 and 32; ``prefetch=1``; the transforms of ``train_defaults()``.  An epoch is timed on the wall clock from the
first ``__iter__`` to a final synchronisation; one warm-up epoch, then the median of ``--epochs`` with minimum and maximum.  The
files were just written: every read comes from the page cache.
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from time_png_read import make, png_bytes  # noqa: E402

DISTINCT, THREADS = 16, 16
FORMS = ("pil", "repacked", "jpeg")
LOADERS = (("s", ["d", "s", "m"]), ("rf", ["p"]))


def write_forms(root, h, w):
    """-> {form: [{task: path}]}"""
    import io

    from PIL import Image

    from climategan_amd import repack_png

    forms = {f: [] for f in FORMS}
    for i in range(DISTINCT):
        files = {task: png_bytes(make(task, h, w, i)) for task in ("x", "s", "d", "m")}
        repacked, _ = repack_png.repack(list(files.values()), 2, "cuda")
        b = io.BytesIO()
        Image.fromarray(make("x", h, w, i)).save(b, "JPEG", quality=90)
        variants = {"pil": files, "repacked": {t: new or files[t] for t, new in zip(files, repacked)},
                    "jpeg": dict(files, x=b.getvalue())}
        for form, by_task in variants.items():
            sample = {}
            for task, data in by_task.items():
                path = root / form / ("%s%02d.%s" % (task, i, "jpg" if (form, task) == ("jpeg", "x") else "png"))
                path.parent.mkdir(parents=True, exist_ok=True)
                path.write_bytes(data)
                sample[task] = str(path)
            forms[form].append(sample)
    return forms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--large", action="store_true", help="1200 x 1800 instead of 640 x 640")
    ap.add_argument("--forms", nargs="+", choices=FORMS, default=list(FORMS), help="the forms to time (PIL's own files are slow on the device)")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader_read: needs the GPU (nothing here can be timed on a CPU)")
    from climategan_amd import data
    from climategan_amd.train import train_defaults

    h, w = (1200, 1800) if args.large else (640, 640)
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        forms = write_forms(root, h, w)
        for form in args.forms:
            for domain, tasks in LOADERS:
                listed = [{t: p for t, p in forms[form][i % DISTINCT].items() if domain == "s" or t in ("x", "m")}
                          for i in range(args.samples)]
                lists = root / ("%s_%s.json" % (form, domain))
                lists.write_text(json.dumps(listed))
                for batch in (4, 32):
                    rec = {"form": form, "domain": domain, "tasks": tasks, "shape": [h, w], "batch": batch, "samples": args.samples}
                    for decode in ("host", "device"):
                        opts = train_defaults()
                        opts.tasks = tasks
                        opts.data.files = {"base": str(root), "train": {domain: lists.name}}
                        opts.data.loaders = {"batch_size": batch, "num_workers": THREADS, "decode": decode}
                        loader = data.get_loader("train", domain, opts, prefetch=1, device="cuda:0")
                        seconds = []
                        for epoch in range(1 + args.epochs):
                            if epoch == 1:                       # the first epoch warms the pool, the allocator and the buffers
                                loader.times = {k: 0 for k in loader.times}
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            n = sum(1 for _ in loader)
                            torch.cuda.synchronize()
                            if epoch:
                                seconds.append((time.perf_counter() - t0) / (n * batch))
                        loader.close()
                        t = loader.times
                        rec[decode] = {"ms_per_sample": round(1e3 * statistics.median(seconds), 3),
                                       "ms_per_sample_min_max": [round(1e3 * min(seconds), 3), round(1e3 * max(seconds), 3)],
                                       "host_ms_per_batch": {k: round(1e3 * v / max(t["batches"], 1), 2) for k, v in t.items() if k != "batches"},
                                       "decode_counts": dict(loader.decode_counts)}
                    rec["device_over_host"] = round(rec["device"]["ms_per_sample"] / rec["host"]["ms_per_sample"], 3)
                    records.append(rec)
                    print("%-8s %-2s batch %2d   host %7.3f   device %7.3f ms/sample   (x %.2f)   %s" % (
                        form, domain, batch, rec["host"]["ms_per_sample"], rec["device"]["ms_per_sample"], rec["device_over_host"],
                        rec["device"]["decode_counts"]), flush=True)
                    res = {"epochs": args.epochs, "warmup_epochs": 1, "threads": THREADS, "distinct_samples": DISTINCT, "prefetch": 1,
                           "files": "generated, read from the page cache", "device": torch.cuda.get_device_name(0), "machines": 1,
                           "runs": 1, "records": records}
                    if args.json:                            # after every case: a long run that is cut short keeps what it measured
                        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
                        Path(args.json).write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
