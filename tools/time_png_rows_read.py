"""Time reading a batch of row-framed PNG files three ways, on the same files:

  rows        file bytes -> ``png.decode``: the row path (``cgan_png_decode_rows``, one wave per row); uploads inside
  serial      the same bytes through ``cgan_png_decode`` (one wave per file) of ANOTHER build of the library loaded beside this
              one (``--serial-lib``: the parent commit's libcgan_hip.so); without it, this build's ``cgan_png_decode``
  host_pool   ``PIL.Image.open`` + ``np.asarray`` from a 16-thread pool, each array uploaded
  pil_files   the same pool on the same images as PIL writes them at its default level (what a data set holds before it is
              repacked): other files, the same pixels

usage: python tools/time_png_rows_read.py [--serial-lib PATH] [--reps 9] [--warmup 2] [--json profiles/png_rows_read.json] [--quick]

The files are ``tools/time_png_read.py``'s generated kinds the encoder can write -- ``x`` photo-like RGB, ``d`` Unity-coded depth
in RGB, ``m`` a grey binary mask -- at 640 x 640 and 1200 x 1800, encoded by ``png.encode`` at level 2 (what
``python -m climategan_amd.repack_png`` writes), in batches of 16 and 128 that cycle through 8 distinct files.  Every repetition
of every path starts from the files' bytes in host memory and ends when every image is on the device; the paths alternate
inside each repetition, each timed with events behind a synchronisation; medians with minimum and maximum.  The three results
are compared file by file and must be equal.  Recorded beside them, for the row path alone: the time of the call
``ops.png_decode_rows`` with everything already uploaded (the memset and the five launches) for the batch and for one file --
one file's rows all run side by side, so that time is about one row's latency.
"""
import argparse
import ctypes as C
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
sys.path.insert(0, str(ROOT / "tools"))

from time_png_read import BATCHES, DISTINCT, SIZES, THREADS, event_timed, make  # noqa: E402

KINDS = ("x", "d", "m")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--serial-lib", default=None, help="another build of libcgan_hip.so whose cgan_png_decode is the serial path")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    ap.add_argument("--quick", action="store_true", help="640 x 640 and batches of 16 only")
    ap.add_argument("--only-rows", action="store_true", help="time the row path alone (an A/B of two builds of it, run after run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_png_rows_read: needs the GPU (nothing here can be timed on a CPU)")
    from PIL import Image

    from climategan_amd import _lib, ops, png

    P = C.c_void_p
    serial_lib = C.CDLL(str(Path(args.serial_lib).resolve())) if args.serial_lib else _lib.load()
    serial_lib.cgan_png_decode_workspace_bytes.restype, serial_lib.cgan_png_decode_workspace_bytes.argtypes = C.c_size_t, [P, C.c_int32]
    serial_lib.cgan_png_decode.restype = C.c_int
    serial_lib.cgan_png_decode.argtypes = [P, C.c_size_t, P, P, C.c_int32, P, C.c_size_t, P, P, C.c_size_t, P]

    def serial(files):
        """``png.decode`` with the batch handed to the serial library's ``cgan_png_decode``: the same probe, uploads and wait."""
        taken = [png.probe(f)[0] for f in files]
        blob, descs, descs_dev = png.upload(list(zip(taken, files)), "cuda")
        n = len(descs)
        nbytes = serial_lib.cgan_png_decode_workspace_bytes(C.addressof(descs), n)
        assert nbytes
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        out = torch.empty(max(d.out_offset + d.width * d.height * d.channels for d in descs), dtype=torch.uint8, device="cuda")
        rc = serial_lib.cgan_png_decode(blob.data_ptr(), blob.numel(), C.addressof(descs), descs_dev.data_ptr(), n, out.data_ptr(),
                                        out.numel(), status.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and status.tolist() == [0] * n                                    # the one wait
        return [out[d.out_offset:d.out_offset + d.width * d.height * d.channels].view(d.height, d.width, d.channels) for d in descs]

    def call_alone(files, reps):
        """The device call of the row path with its inputs in place -> median seconds."""
        taken = [png.probe(f)[0] for f in files]
        blob, descs, descs_dev = png.upload(list(zip(taken, files)), "cuda")
        tables, tables_dev = png.row_tables(descs, files, "cuda")
        times = [event_timed(lambda: ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)) for _ in range(2 + reps)]
        return statistics.median(times[2:])

    pool = ThreadPoolExecutor(THREADS)

    def read(data):
        a = np.asarray(Image.open(io.BytesIO(data)))
        return torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to("cuda")

    records = []
    for h, w in (SIZES[:1] if args.quick else SIZES):
        for kind in KINDS:
            imgs = np.stack([make(kind, h, w, i).reshape(h, w, -1) for i in range(DISTINCT)])
            distinct = png.encode(torch.from_numpy(imgs).cuda(), level=2)
            pil_distinct = [_pil(a) for a in imgs]
            pil_bytes = sum(map(len, pil_distinct)) / DISTINCT
            assert all(png.probe(f)[0].rows == h for f in distinct)
            for batch in (BATCHES[:1] if args.quick else BATCHES):
                files = [distinct[i % DISTINCT] for i in range(batch)]
                pil_files = [pil_distinct[i % DISTINCT] for i in range(batch)]
                result = {}
                runs = {"rows": lambda: result.__setitem__("rows", png.decode(files)),
                        "serial": lambda: result.__setitem__("serial", serial(files)),
                        "host_pool": lambda: result.__setitem__("host_pool", list(pool.map(read, files))),
                        "pil_files": lambda: result.__setitem__("pil_files", list(pool.map(read, pil_files)))}
                if args.only_rows:
                    runs = {"rows": runs["rows"]}
                times = {k: [] for k in runs}
                for rep in range(args.warmup + args.reps):
                    for k, fn in runs.items():
                        t = event_timed(fn)
                        if rep >= args.warmup:
                            times[k].append(t)
                for k in list(runs)[1:]:
                    assert all(torch.equal(a, b) for a, b in zip(result["rows"], result[k])), (kind, h, w, batch, k)
                assert all(torch.equal(a.cpu(), torch.from_numpy(imgs[i % DISTINCT])) for i, a in enumerate(result["rows"]))
                rec = {"kind": kind, "shape": [h, w], "batch": batch, "level": 2, "file_bytes_mean": sum(map(len, files)) / batch,
                       "pil_default_file_bytes_mean": pil_bytes, "raw_bytes_mean": h * w * imgs.shape[3], "equal": True}
                for k in runs:
                    rec[k] = {"ms_per_file": 1e3 * statistics.median(times[k]) / batch,
                              "ms_per_file_min_max": [1e3 * min(times[k]) / batch, 1e3 * max(times[k]) / batch]}
                rec["fastest"] = min(runs, key=lambda k: rec[k]["ms_per_file"])
                rec["rows_call_alone_ms"] = {"batch": 1e3 * call_alone(files, args.reps), "one_file": 1e3 * call_alone(files[:1], args.reps)}
                records.append(rec)
                print("%-2s %4d x %4d  batch %3d  %8.0f B/file  %s ms/file   -> %s   (the row call alone: %.3f ms the batch, %.3f ms one file)" % (
                    kind, h, w, batch, rec["file_bytes_mean"], "".join("   %s %7.3f" % (k, rec[k]["ms_per_file"]) for k in runs),
                    rec["fastest"], rec["rows_call_alone_ms"]["batch"], rec["rows_call_alone_ms"]["one_file"]), flush=True)
    res = {"reps": args.reps, "warmup": args.warmup, "threads": THREADS, "distinct_files_per_case": DISTINCT,
           "serial_library": "another build (--serial-lib)" if args.serial_lib else "this build's cgan_png_decode",
           "device": torch.cuda.get_device_name(0), "machines": 1, "runs": 1, "records": records}
    line = json.dumps(res)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")
    pool.shutdown()


def _pil(a):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(b, "PNG")
    return b.getvalue()


if __name__ == "__main__":
    main()
