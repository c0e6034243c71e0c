"""Time the "write" stage of apply_events for one batch of 16 outputs of 640 x 640 x 3 as JPEG: ``jpeg.write`` (device
encoder) at quality 90 in 4:4:4 and in 4:2:0 against ``png.write`` at level 2 and against
``PIL.Image.save(..., "JPEG", quality=90, subsampling=...)`` from a 16-thread pool.

usage: python tools/time_jpeg_write.py [--out DIR] [--reps 9] [--warmup 2] [--json profiles/jpeg_write.json]

The batch is ``tools/time_png_write.py``'s: the small checkpoint's ``infer_all`` events of generated photos.  Every repetition
of every path starts from the same uint8 images where that path finds them (the device for the device encoders, host arrays
for PIL: the device-to-host copy of the raw pixels PIL needs is timed separately and reported, not added), writes 16 files
and ends when the last file is closed; the paths alternate inside each repetition and the medians are reported with their
minimum and maximum.  Prints seconds per image and bytes per image for every path, the PSNR of the device files and of PIL's
against the source pixels, and one JSON line.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from time_png_write import BATCH, finish, measure, setup  # noqa: E402

QUALITY = 90


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def main():
    args, dev, host, out, tmp, pool = setup(__doc__, "time_jpeg_write")
    from PIL import Image

    from climategan_amd import jpeg, png

    kinds = ("gpu_jpeg_444", "gpu_jpeg_420", "gpu_png_level2", "pil_jpeg_444", "pil_jpeg_420")
    paths = {k: [out / ("%s_%02d.%s" % (k, i, "png" if "png" in k else "jpg")) for i in range(BATCH)] for k in kinds}

    def pil(kind, subsampling):
        list(pool.map(lambda ip: Image.fromarray(ip[0]).save(ip[1], "JPEG", quality=QUALITY, subsampling=subsampling),
                      zip(host, paths[kind])))

    runs = {"gpu_jpeg_444": lambda: jpeg.write(dev, paths["gpu_jpeg_444"], quality=QUALITY, subsampling="444"),
            "gpu_jpeg_420": lambda: jpeg.write(dev, paths["gpu_jpeg_420"], quality=QUALITY, subsampling="420"),
            "gpu_png_level2": lambda: png.write(dev, paths["gpu_png_level2"], level=2),
            "pil_jpeg_444": lambda: pil("pil_jpeg_444", 0),
            "pil_jpeg_420": lambda: pil("pil_jpeg_420", 2)}
    res = measure(args, dev, runs, paths, quality=QUALITY)
    for k in runs:
        decoded = np.stack([np.asarray(Image.open(p)) for p in paths[k]])          # every file opens; PNG holds the pixels
        res[k]["psnr_db"] = psnr(decoded, host)
        print("%-15s %.6f s/image (min %.6f, max %.6f)  %8.0f bytes/image  PSNR %.2f dB" % (
            k, res[k]["s_per_image"], *res[k]["s_per_image_min_max"], res[k]["bytes_per_image"], res[k]["psnr_db"]))
    assert res["gpu_png_level2"]["psnr_db"] == float("inf")
    res["gpu_png_level2"]["psnr_db"] = None                                        # lossless; JSON has no infinity
    for sub in ("444", "420"):
        g, p, z = res["gpu_jpeg_" + sub], res["pil_jpeg_" + sub], res["gpu_png_level2"]
        res["size_ratio_jpeg_%s_over_png_level2" % sub] = g["bytes_per_image"] / z["bytes_per_image"]
        res["size_ratio_jpeg_%s_over_pil" % sub] = g["bytes_per_image"] / p["bytes_per_image"]
        res["time_ratio_jpeg_%s_over_png_level2" % sub] = g["s_per_image"] / z["s_per_image"]
        res["speedup_jpeg_%s_over_pil" % sub] = p["s_per_image"] / g["s_per_image"]
        print("%s: bytes JPEG / PNG level 2 = %.4f, JPEG / PIL's JPEG = %.4f; time JPEG / PNG level 2 = %.3f, PIL / JPEG = %.2f"
              % (sub, res["size_ratio_jpeg_%s_over_png_level2" % sub], res["size_ratio_jpeg_%s_over_pil" % sub],
                 res["time_ratio_jpeg_%s_over_png_level2" % sub], res["speedup_jpeg_%s_over_pil" % sub]))
    finish(args, res, tmp, pool)


if __name__ == "__main__":
    main()
