"""Rewrite a folder's PNG files as row-framed files, which the device decoder inflates one wave per row:

    python -m climategan_amd.repack_png -i SRC -o DST [--level {1,2}] [-b N] [--overwrite]

The SRC tree is mirrored into DST.  Every ``.png`` that decodes to uint8 pixels with 1 or 3 channels and a width of at most
``ops.PNG_MAX_WIDTH`` (on the device, ``png.try_decode``; through PIL where the device decoder does not take the file and PIL
opens it as mode L or RGB) is encoded again by the device encoder (``png.encode``), batched by shape.  The new bytes are
written only after two checks: they probe as ``rows == height``, and they decode on the device to the source's pixels.  Every
other file -- RGBA, 16-bit, palette, too wide, not a PNG at all -- is copied byte for byte.  The files stay ordinary PNG files
(level 2 is within a few percent of PIL's default size); a data set is repacked once and read every epoch.
"""
import argparse
import io
import sys
from collections import Counter, defaultdict
from pathlib import Path

import torch

from . import ops, png


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m climategan_amd.repack_png", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-i", "--input", required=True, help="the folder to read")
    p.add_argument("-o", "--output", required=True, help="the folder to write: SRC's tree, mirrored; not SRC and not inside it")
    p.add_argument("--level", type=int, choices=(1, 2), default=2, help="the encoder's level (ops.png_encode); default 2")
    p.add_argument("-b", "--batch", type=int, default=16, help="files decoded and encoded per device call; default 16")
    p.add_argument("--overwrite", action="store_true", help="write into a DST that exists")
    return p.parse_args(argv)


def source_pixels(datas, device):
    """The files' bytes -> (images, reasons): a uint8 [H, W, 1 | 3] device tensor for every file to repack, else None and why
    the file is copied."""
    images, why = png.try_decode(datas, device)
    reasons = {}
    for i, data in enumerate(datas):
        im = images[i]
        if im is None:                                        # not the device decoder's: PIL's L and RGB files still are ours
            import numpy as np
            from PIL import Image

            try:
                pil = Image.open(io.BytesIO(data))
                if pil.format != "PNG" or pil.mode not in ("L", "RGB"):
                    reasons[i] = "not a PNG file" if pil.format != "PNG" else "mode %s" % pil.mode
                    continue
                a = np.asarray(pil)
            except Exception:
                reasons[i] = "unreadable (%s)" % why[i]
                continue
            im = images[i] = torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to(device)
        if im.dtype != torch.uint8:
            reasons[i] = "16-bit"
        elif im.shape[2] not in (1, 3):
            reasons[i] = "%d channels" % im.shape[2]
        elif im.shape[1] > ops.PNG_MAX_WIDTH:
            reasons[i] = "wider than %d" % ops.PNG_MAX_WIDTH
        if i in reasons:
            images[i] = None
    return images, reasons


def repack(datas, level, device):
    """-> (new bytes or None per file, reasons for the None ones)."""
    images, reasons = source_pixels(datas, device)
    out = [None] * len(datas)
    groups = defaultdict(list)
    for i, im in enumerate(images):
        if im is not None:
            groups[tuple(im.shape)].append(i)
    for shape, members in groups.items():
        files = png.encode(torch.stack([images[i] for i in members]).contiguous(), level=level)
        framed = [(png.probe(f)[0], f) for f in files]
        again, bad = png.try_decode(files, device)
        for k, i in enumerate(members):
            d = framed[k][0]
            if d is None or d.rows != shape[0]:
                reasons[i] = "check failed: the new file is not row-framed"
            elif k in bad or again[k].shape != images[i].shape or not torch.equal(again[k], images[i]):
                reasons[i] = "check failed: the new file does not decode to the source's pixels"
            else:
                out[i] = files[k]
    return out, reasons


def main(argv=None):
    args = parse_args(argv)
    src, dst = Path(args.input).resolve(), Path(args.output).resolve()
    if not src.is_dir():
        raise SystemExit("repack_png: %s is not a folder" % src)
    if dst == src or src in dst.parents:
        raise SystemExit("repack_png: the output %s is the input or lies inside it" % dst)
    if dst.exists() and not args.overwrite:
        raise SystemExit("repack_png: %s exists (--overwrite to write into it)" % dst)
    if args.batch < 1:
        raise SystemExit("repack_png: -b %d" % args.batch)
    if not torch.cuda.is_available():
        raise SystemExit("repack_png: needs a device; there is no CPU path")
    files = sorted(p for p in src.rglob("*") if p.is_file())
    pngs = [p for p in files if p.suffix.lower() == ".png"]
    copied, repacked, before, after = Counter(), 0, 0, 0

    def put(path, data):
        target = dst / path.relative_to(src)
        target.parent.mkdir(parents=True, exist_ok=True)
        target.write_bytes(data)

    for p in files:
        if p.suffix.lower() != ".png":
            put(p, p.read_bytes())
            copied["not a .png"] += 1
    for at in range(0, len(pngs), args.batch):
        batch = pngs[at:at + args.batch]
        datas = [p.read_bytes() for p in batch]
        new, reasons = repack(datas, args.level, "cuda")
        for i, p in enumerate(batch):
            if new[i] is None:
                put(p, datas[i])
                copied[reasons[i]] += 1
            else:
                put(p, new[i])
                repacked += 1
                before += len(datas[i])
                after += len(new[i])
    print("repack_png: %d repacked at level %d (%d -> %d bytes), %d copied%s" % (
        repacked, args.level, before, after, sum(copied.values()),
        "".join("; %d %s" % (n, why) for why, n in sorted(copied.items()))))
    return 1 if any(why.startswith("check failed") for why in copied) else 0


if __name__ == "__main__":
    sys.exit(main())
