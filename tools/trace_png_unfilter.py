"""The PNG decoder's kernel times from a kernel trace, per build of the library (the choice of the unfilter
kernel's waves per file against the parent's one-wave kernel).

  run       the workload to trace: ``png.decode`` on 1, 16 and 128 ``x`` files of 640 x 640 and on 1 and 16 of 1200 x 1800
            (``tools/time_png_read.py``'s generated photo-like RGB, encoded by ``png.encode`` at level 2: row-framed files),
            each batch ``--reps`` times after one warm-up.  ``--lib PATH``: the device call ``cgan_png_decode_rows`` of another
            build of the library loaded beside this one (the parent commit's, a build with other waves per file):

              rocprofv3 --kernel-trace --output-format csv -d OUT/label -- \\
                  python tools/trace_png_unfilter.py run --lib other/libcgan_hip.so

  collect   ``label=OUT/label ...`` -> one JSON line (and ``--json FILE``): per build and case the median, minimum and maximum
            of every decode kernel's duration over the repetitions; the launches of a kernel are matched to the cases by their
            order in the trace.
"""
import argparse
import csv
import json
import re
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

CASES = ((640, 640, 1), (640, 640, 16), (640, 640, 128), (1200, 1800, 1), (1200, 1800, 16))
KERNELS = ("layout_kernel", "inflate_rows_kernel", "inflate_kernel", "unfilter_kernel")
DISTINCT = 8


def run(reps, lib_path):
    import ctypes as C

    import numpy as np
    import torch

    from climategan_amd import _lib, png
    from time_png_read import make

    P = C.c_void_p
    lib = C.CDLL(str(Path(lib_path).resolve())) if lib_path else _lib.load()
    size_of, call = lib.cgan_png_decode_rows_workspace_bytes, lib.cgan_png_decode_rows
    size_of.restype, size_of.argtypes = C.c_size_t, [P, P, C.c_size_t, C.c_int32]
    call.restype = C.c_int
    call.argtypes = [P, C.c_size_t, P, P, P, P, C.c_size_t, C.c_int32, P, C.c_size_t, P, P, P, C.c_size_t, P]

    def decode(files):
        """``png.decode`` with the device call made in ``lib``: the same probe, uploads and wait."""
        taken = [png.probe(f)[0] for f in files]
        blob, descs, descs_dev = png.upload(list(zip(taken, files)), "cuda")
        tables, tables_dev = png.row_tables(descs, files, "cuda")
        n = len(descs)
        nbytes = size_of(C.addressof(descs), C.addressof(tables), len(tables), n)
        assert nbytes
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        status, path = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        out = torch.empty(max(d.out_offset + d.width * d.height * d.channels for d in descs), dtype=torch.uint8, device="cuda")
        rc = call(blob.data_ptr(), blob.numel(), C.addressof(descs), descs_dev.data_ptr(), C.addressof(tables), tables_dev.data_ptr(),
                  len(tables), n, out.data_ptr(), out.numel(), status.data_ptr(), path.data_ptr(), ws.data_ptr(), nbytes,
                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and status.tolist() == [0] * n and path.tolist() == [1] * n                # the one wait
        return [png.image_view(out, d) for d in descs]

    for h, w, batch in CASES:
        imgs = np.stack([make("x", h, w, i) for i in range(min(batch, DISTINCT))])
        distinct = png.encode(torch.from_numpy(imgs).cuda(), level=2)
        files = [distinct[i % len(distinct)] for i in range(batch)]
        for _ in range(1 + reps):
            images = decode(files)
        torch.cuda.synchronize()
        assert all(torch.equal(im.cpu(), torch.from_numpy(imgs[i % len(distinct)])) for i, im in enumerate(images))
        print("%d x %d, %d files: decoded %d times" % (h, w, batch, 1 + reps), flush=True)


def plain_name(demangled):
    """``void (anonymous namespace)::unfilter_kernel<8, 8>(...)`` -> ``unfilter_kernel``"""
    m = re.match(r"(?:void\s+)?(?:\w+::)*(\w+)", demangled.replace("(anonymous namespace)::", ""))
    return m.group(1) if m else demangled


def collect(pairs, reps):
    builds = {}
    for pair in pairs:
        label, folder = pair.split("=", 1)
        rows = []
        for path in sorted(Path(folder).rglob("*kernel_trace.csv")):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        records = []
        for kernel in KERNELS:
            mine = [r for r in rows if plain_name(r["Kernel_Name"]) == kernel]
            if len(mine) != len(CASES) * (1 + reps):
                raise SystemExit("%s: %d launches of %s, %d expected" % (label, len(mine), kernel, len(CASES) * (1 + reps)))
            for k, (h, w, batch) in enumerate(CASES):
                ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in mine[k * (1 + reps) + 1:(k + 1) * (1 + reps)]]
                if len(records) <= k:
                    records.append({"kind": "x", "shape": [h, w], "batch": batch, "kernel_ms": {}})
                records[k]["kernel_ms"][kernel] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        builds[label] = records
    return {"tool": "rocprofv3 --kernel-trace, one session, one machine; level-2 files of tools/time_png_read.py's kind x; "
                    "median of %d calls after one warm-up" % reps, "builds": builds}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=("run", "collect"))
    ap.add_argument("traces", nargs="*", help="collect: label=folder of one traced run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lib", default=None, help="run: another build of libcgan_hip.so whose cgan_png_decode_rows is traced")
    args = ap.parse_args()
    if args.mode == "run":
        return run(args.reps, args.lib)
    line = json.dumps(collect(args.traces, args.reps))
    print(line)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(line + "\n")


if __name__ == "__main__":
    main()
