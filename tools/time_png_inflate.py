"""Time reading a batch of ordinary PNG files (PIL's own, one zlib stream per file) through the device decoder's whole-stream
inflate in its forms, on the same files:

  lanes       file bytes -> ``ops.png_decode``: the stream's tokens decoded across the wave's 64 lanes, at the compiled
              subsequence bits and lane tokens (what ``png.decode`` runs); uploads inside
  serial0     the same with ``subseq_bits=0``: this build's serial kernel, lane 0 decodes
  parent      the same bytes through ``cgan_png_decode`` of ANOTHER build of the library loaded beside this one
              (``--serial-lib``: the parent commit's libcgan_hip.so, the yardstick); left out without it
  parent_serial0  the other build's ``cgan_png_decode_lanes`` with ``subseq_bits=0``: the yardstick of ``serial0``
  host_pool   ``PIL.Image.open`` + ``np.asarray`` from a 16-thread pool, each array uploaded

usage: python tools/time_png_inflate.py [--serial-lib PATH] [--reps 9] [--warmup 2] [--json profiles/png_inflate_lanes.json]
                                        [--quick] [--kinds xsdm] [--also BITS,TOKENS]
       python tools/time_png_inflate.py --stats        (no GPU: the host twin's pass statistics per kind and size)
       python tools/time_png_inflate.py --trace-run    (the workload of a kernel trace: 16 ``x`` files of 640 x 640, 3 calls each
                                                        of lanes and serial0, under ``rocprofv3 --kernel-trace --stats``)

The files and the method are ``tools/time_png_read.py``'s: its generated kinds ``x``, ``s``, ``d``, ``m`` written by PIL at its
default level, 640 x 640 and 1200 x 1800, batches of 16 and 128 that cycle through 8 distinct files; every repetition of every
path starts from the files' bytes in host memory and ends when every image is on the device; the paths alternate inside each
repetition, each timed with events behind a synchronisation; medians with minimum and maximum.  The results are compared file
by file and must be equal.  Beside every record: the twin's statistics on the 8 files (``cgan_png_inflate_lanes_host``:
windows, passes, the most passes of one window, windows ended by a lane's token cap, tokens) and the stream's bits per
inflated byte.
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

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from time_png_read import BATCHES, DISTINCT, SIZES, THREADS, make, png_bytes  # noqa: E402

STATS = ("windows", "passes", "max_passes", "full_windows", "tokens")


def twin_stats(files):
    """The host twin at the compiled values over ``files`` -> the statistics summed (the most passes: the maximum)."""
    from climategan_amd import _lib, png

    lib = _lib.load()
    params = png.inflate_params()
    total = dict.fromkeys(STATS, 0)
    stream_bits = inflated = 0
    for data in files:
        d, why = png.probe(data)
        assert d is not None, why
        stream = np.frombuffer(png.stream_of(data, d), dtype=np.uint8).copy()
        out = np.zeros(d.height * (1 + d.width * d.channels * d.bit_depth // 8), dtype=np.uint8)
        trailer, status, stats = C.c_uint32(0), C.c_int32(-1), (C.c_uint32 * 5)()
        rc = lib.cgan_png_inflate_lanes_host(stream.ctypes.data, C.addressof(d), params["subseq_bits"], params["lane_tokens"],
                                             out.ctypes.data, C.addressof(trailer), stats, C.addressof(status))
        assert rc == 0 and status.value == 0
        for k, v in zip(STATS, stats):
            total[k] = max(total[k], v) if k == "max_passes" else total[k] + v
        stream_bits += 8 * stream.size
        inflated += out.size
    total["passes_per_window"] = round(total["passes"] / max(total["windows"], 1), 3)
    total["tokens_per_window"] = round(total["tokens"] / max(total["windows"], 1), 1)
    total["stream_bits_per_inflated_byte"] = round(stream_bits / inflated, 4)
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--serial-lib", default=None, help="another build of libcgan_hip.so whose cgan_png_decode is the yardstick")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the result line to this file")
    ap.add_argument("--quick", action="store_true", help="640 x 640 and batches of 16 only")
    ap.add_argument("--kinds", default="xsdm")
    ap.add_argument("--also", default=None, metavar="BITS,TOKENS", help="one more path: the lanes at these values (cgan_png_decode_lanes)")
    ap.add_argument("--stats", action="store_true", help="the twin's statistics alone: needs no GPU")
    ap.add_argument("--trace-run", action="store_true", help="the short workload of a kernel trace")
    args = ap.parse_args()
    sizes, batches = (SIZES[:1], BATCHES[:1]) if args.quick else (SIZES, BATCHES)
    if args.stats:
        for h, w in sizes:
            for kind in args.kinds:
                print(kind, h, w, json.dumps(twin_stats([png_bytes(make(kind, h, w, i)) for i in range(DISTINCT)])), flush=True)
        return
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_png_inflate: needs the GPU (only --stats runs without one)")
    from PIL import Image

    from climategan_amd import ops, png
    from time_png_read import event_timed

    def ours(files, **kw):
        taken = [png.probe(f)[0] for f in files]
        blob, descs, descs_dev = png.upload(list(zip(taken, files)), "cuda")
        out, status = ops.png_decode(blob, descs, descs_dev, **kw)
        assert status.tolist() == [0] * len(files)                                        # the one wait
        return [png.image_view(out, d) for d in descs]

    if args.trace_run:
        files = [png_bytes(make("x", 640, 640, i % DISTINCT)) for i in range(16)]
        for kw in ({}, {"subseq_bits": 0}):
            for _ in range(3):
                ours(files, **kw)
        torch.cuda.synchronize()
        print("16 x files of 640 x 640: 3 calls at the compiled values, then 3 of the serial kernel")
        return

    P = C.c_void_p
    parent_lib = None
    if args.serial_lib:
        parent_lib = C.CDLL(str(Path(args.serial_lib).resolve()))
        parent_lib.cgan_png_decode_workspace_bytes.restype, parent_lib.cgan_png_decode_workspace_bytes.argtypes = C.c_size_t, [P, C.c_int32]
        parent_lib.cgan_png_decode.restype = C.c_int
        parent_lib.cgan_png_decode.argtypes = [P, C.c_size_t, P, P, C.c_int32, P, C.c_size_t, P, P, C.c_size_t, P]
        parent_lib.cgan_png_decode_lanes.restype = C.c_int
        parent_lib.cgan_png_decode_lanes.argtypes = parent_lib.cgan_png_decode.argtypes + [C.c_int32, C.c_int32]

    def parent(files, serial0=False):
        """``ours`` with the batch handed to the other library's ``cgan_png_decode`` (serial0: its ``cgan_png_decode_lanes`` with
        ``subseq_bits=0``, its serial kernel): the same probe, uploads and wait."""
        taken = [png.probe(f)[0] for f in files]
        blob, descs, descs_dev = png.upload(list(zip(taken, files)), "cuda")
        n = len(descs)
        nbytes = parent_lib.cgan_png_decode_workspace_bytes(C.addressof(descs), n)
        assert nbytes
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        out = torch.empty(max(d.out_offset + d.width * d.height * d.channels for d in descs), dtype=torch.uint8, device="cuda")
        call_args = (blob.data_ptr(), blob.numel(), C.addressof(descs), descs_dev.data_ptr(), n, out.data_ptr(), out.numel(),
                     status.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        if serial0:
            rc = parent_lib.cgan_png_decode_lanes(*call_args, 0, png.inflate_params()["lane_tokens"])
        else:
            rc = parent_lib.cgan_png_decode(*call_args)
        assert rc == 0 and status.tolist() == [0] * n                                     # the one wait
        return [png.image_view(out, d) for d in descs]

    pool = ThreadPoolExecutor(THREADS)

    def read(data):
        a = np.asarray(Image.open(io.BytesIO(data)))
        return torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to("cuda")

    records = []
    for h, w in sizes:
        for kind in args.kinds:
            distinct = [png_bytes(make(kind, h, w, i)) for i in range(DISTINCT)]
            stats = twin_stats(distinct)
            for batch in batches:
                files = [distinct[i % DISTINCT] for i in range(batch)]
                result = {}
                runs = {"lanes": lambda: result.__setitem__("lanes", ours(files)),
                        "serial0": lambda: result.__setitem__("serial0", ours(files, subseq_bits=0)),
                        "parent": lambda: result.__setitem__("parent", parent(files)),
                        "parent_serial0": lambda: result.__setitem__("parent_serial0", parent(files, serial0=True)),
                        "host_pool": lambda: result.__setitem__("host_pool", list(pool.map(read, files)))}
                if parent_lib is None:
                    del runs["parent"], runs["parent_serial0"]
                if args.also:
                    bits, tokens = (int(v) for v in args.also.split(","))
                    runs["lanes_%d_%d" % (bits, tokens)] = lambda: result.__setitem__("also", ours(files, subseq_bits=bits, lane_tokens=tokens))
                times = {k: [] for k in runs}
                for rep in range(args.warmup + args.reps):
                    for k, fn in runs.items():
                        t = event_timed(fn)
                        if rep >= args.warmup:
                            times[k].append(t)
                for k in list(result)[1:]:
                    assert all(torch.equal(a, b) for a, b in zip(result["lanes"], result[k])), (kind, h, w, batch, k)
                rec = {"kind": kind, "shape": [h, w], "batch": batch, "file_bytes_mean": sum(map(len, files)) / batch,
                       "raw_bytes_mean": sum(int(im.numel()) for im in result["lanes"]) / batch, "equal": True, "twin": stats}
                for k in runs:
                    rec[k] = {"ms_per_file": 1e3 * statistics.median(times[k]) / batch,
                              "ms_per_file_min_max": [1e3 * min(times[k]) / batch, 1e3 * max(times[k]) / batch]}
                records.append(rec)
                print("%-2s %4d x %4d  batch %3d  %8.0f B/file  %s ms/file   passes/window %.2f" % (
                    kind, h, w, batch, rec["file_bytes_mean"],
                    "".join("   %s %7.3f [%.3f %.3f]" % ((k, rec[k]["ms_per_file"]) + tuple(rec[k]["ms_per_file_min_max"])) for k in runs),
                    stats["passes_per_window"]), flush=True)
    res = {"reps": args.reps, "warmup": args.warmup, "threads": THREADS, "distinct_files_per_case": DISTINCT,
           "inflate_params": png.inflate_params(),
           "parent_library": "another build (--serial-lib)" if parent_lib is not None else None,
           "device": torch.cuda.get_device_name(0), "machines": 1, "runs": 1, "records": records}
    line = json.dumps(res)
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()
