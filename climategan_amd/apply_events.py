"""Mirror of the reference's ``apply_events.py``: a folder of photos in, one flood, smog and
wildfire PNG per photo out.

    python -m climategan_amd.apply_events -i IMAGES -r RUN -o OUT [-b 16] [--half] [--save_masks] [-s] ...

Same options, defaults, size validation, output-directory and file names, ``-n`` rule, timing table and run record
(``command.txt`` / ``hash.txt``) as the reference (apply_events.py:4-148, 294-374, 377-642).  Every stage runs on the device:
``resize_and_crop`` (apply_events.py:211-241) and ``to_m1_p1`` (apply_events.py:179-195) as one HIP call per image
(``prepare_batch`` / ``resize_keep_ratio``; the reference spends ~25 ms per 1-2 Mpixel photo in scikit-image, here the uint8
image is uploaded once, 3 bytes / pixel), ``Trainer.infer_all``, the uint8 conversion, and the PNG encoding (``png.write``):
only compressed bytes come back to the host.

Differences: ``--upload`` (comet) is refused; an existing output directory without ``--overwrite`` is refused with a
message instead of the reference's ``input()`` prompt, which nobody answers in a batch job; images are read, inferred and
written batch by batch rather than all held in memory; ``--dtype`` selects the kernels' 16-bit type; ``--png_level 2`` asks
the device PNG encoder for smaller files (same pixels; neither is an option of the reference's script); ``--format jpg``
writes the events and the input picture as baseline JPEG files from the device encoder (``jpeg.write``, DESIGN 4.19;
``--jpeg_quality``, ``--jpeg_subsampling``) -- several times smaller, lossy; the masks stay PNG; ``--decode device`` uploads
baseline JPEG and 8-bit RGB PNG inputs as file bytes and decodes them with the device decoders (``jpeg.decode``, DESIGN 4.20;
``png.decode``).
"""
import argparse
import shutil
import subprocess
import sys
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from . import ops


def resize_and_crop(img, to=640, device="cuda"):
    """uint8 HWC image (numpy array or tensor) -> fp32 [3, to, to] device tensor in [-1, 1]
    (= ``to_m1_p1(resize_and_crop(img, to))`` transposed to CHW).  RGBA must be converted by the caller as the
    reference does (apply_events.py:491)."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(img)
    if t.dtype != torch.uint8:
        raise ValueError("resize_and_crop: np.uint8 255 image expected (apply_events.py:218), got %s" % t.dtype)
    return ops.resize_and_crop_u8(t.to(device), to)


def prepare_batch(images, to=640, device="cuda"):
    """list of uint8 HWC images of any sizes -> fp32 [B, 3, to, to] in [-1, 1] (the ``np.stack(images)`` the reference
    hands to ``infer_all``, apply_events.py:521-524, already NCHW and on the device)."""
    if len(images) == 0:
        raise ValueError("prepare_batch: no images")
    batch = torch.empty((len(images), 3, to, to), dtype=torch.float32, device=device)
    for i, img in enumerate(images):
        t = img if isinstance(img, torch.Tensor) else torch.from_numpy(img)
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("prepare_batch: image %d is not [H, W, 3] (convert RGBA / grey first)" % i)
        ops.resize_and_crop_u8(t.to(device), to, out=batch[i])
    return batch


def to_128(im, w_target=-1):
    """reference utils.py:998-1007: (nh, nw) = the largest multiples of 128 not above w_target and nw * h / w."""
    h, w = im.shape[:2]
    aspect_ratio = h / w
    if w_target < 0:
        w_target = w
    nw = int(w_target / 128) * 128
    nh = int(nw * aspect_ratio / 128) * 128
    return nh, nw


def resize_keep_ratio(img, max_im_width=-1, device="cuda"):
    """The keep_ratio branch of the reference loop (apply_events.py:494-497, 502): uint8 HWC image -> fp32
    [3, nh, nw] in [-1, 1] with (nh, nw) = to_128(img, max_im_width); images of different sizes cannot be stacked, so
    ``infer_all`` takes them one at a time (batch_size 1, as the reference requires for keep_ratio)."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(img)
    if t.dtype != torch.uint8:
        raise ValueError("resize_keep_ratio: np.uint8 255 image expected, got %s" % t.dtype)
    nh, nw = to_128(t, max_im_width)
    if nh <= 0 or nw <= 0:
        raise ValueError("resize_keep_ratio: image %s is smaller than 128 pixels in one direction" % (tuple(t.shape),))
    return ops.resize_u8(t.to(device), (nh, nw))


# ------------------------------------------------------------------------------------------------ the command line
REFUSED = {"--upload": "comet upload: this script does not log to comet"}
DTYPES = ("bf16", "fp16")
EVENT_ORDER = ("flood", "wildfire", "smog", "mask", "input")       # the order infer_all fills its dict in, then the input


class _Args(argparse.Namespace):
    """``png_level`` is 1 unless the command line gives it: an attribute with a class default, so that the namespace of a
    run without it -- what ``main`` prints under "Using args" -- holds the entries it held before the option existed.  The
    same for ``format``, the two JPEG options and ``decode``."""
    png_level = 1
    decode = "host"
    format = "png"
    jpeg_quality = 90
    jpeg_subsampling = "444"


def parse_args(argv=None):
    """apply_events.py:4-148 (same names, short forms, defaults and help) + ``--dtype``, ``--png_level``, ``--format``, the
    two ``--jpeg_*`` options and ``--decode``."""
    argv = list(sys.argv[1:] if argv is None else argv)
    for a in argv:
        key = a.split("=", 1)[0]
        if key in REFUSED:
            raise SystemExit("apply_events: %s is not supported here: %s" % (key, REFUSED[key]))
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0], allow_abbrev=False)
    parser.add_argument("-b", "--batch_size", type=int, default=4,
                        help="Batch size to process input images to events. Defaults to 4")
    parser.add_argument("-i", "--images_paths", type=str, required=True, help="Path to a directory with image files")
    parser.add_argument("-o", "--output_path", type=str, default=None,
                        help="Path to a directory were events should be written. Will NOT write anything to disk if this "
                        "flag is not used.")
    parser.add_argument("-s", "--save_input", action="store_true", default=False,
                        help="Include the input image to the model (after crop and resize) in the images written")
    parser.add_argument("-r", "--resume_path", type=str, default=None,
                        help="Path to a directory containing the trainer to resume (opts.yaml and checkpoints/)")
    parser.add_argument("--no_time", action="store_true", default=False, help="Prevent the timing of operations")
    parser.add_argument("-f", "--flood_mask_binarization", type=float, default=0.5,
                        help="Value to use to binarize masks (mask > value). Set to -1 to use soft masks. Defaults to 0.5")
    parser.add_argument("-t", "--target_size", type=int, default=640,
                        help="Output image size (when not using keep_ratio_128); must be a multiple of 128. Defaults to 640")
    parser.add_argument("--half", action="store_true", default=False, help="fp16 input / output tensors (infer_all(half=True))")
    parser.add_argument("-n", "--n_images", default=-1, type=int,
                        help="Limit the number of images processed (more than the directory holds: the list is repeated)")
    parser.add_argument("--no_conf", action="store_true", default=False,
                        help="Disable writing the apply_events hash and command in the output folder")
    parser.add_argument("--overwrite", action="store_true", default=False,
                        help="Write into an output directory that already exists (it is refused otherwise)")
    parser.add_argument("--no_cloudy", action="store_true", default=False,
                        help="Prevent the use of the cloudy intermediate image to create the flood image")
    parser.add_argument("--keep_ratio_128", action="store_true", default=False,
                        help="Resize the images to the closest multiples of 128, keeping their aspect ratio; forces a batch "
                        "size of 1. Use --max_im_width to cap the resulting dimensions")
    parser.add_argument("--fuse", action="store_true", default=False, help="Use batch norm fusion to speed up inference")
    parser.add_argument("--save_masks", action="store_true", default=False, help="Save output masks along events")
    parser.add_argument("-m", "--max_im_width", type=int, default=-1,
                        help="With --keep_ratio_128: cap the resized image's width. Defaults to -1 (no cap)")
    parser.add_argument("--zip_outdir", "-z", action="store_true",
                        help="Zip the output directory as '{outdir.parent}/{outdir.name}.zip'")
    parser.add_argument("--dtype", default=None, choices=DTYPES,
                        help="G.set_compute_dtype: the kernels' 16-bit type (default: the trainer's)")
    parser.add_argument("--png_level", type=int, default=argparse.SUPPRESS, choices=(1, 2),
                        help="Not an option of the reference's script: the device PNG encoder's level. 1: fixed-Huffman "
                        "blocks; 2: per row the smallest of a fixed, dynamic or stored block (smaller files, same pixels). "
                        "Defaults to 1")
    parser.add_argument("--format", default=argparse.SUPPRESS, choices=("png", "jpg"),
                        help="Not an option of the reference's script: the file format of the events and of the input "
                        "picture. jpg: baseline JPEG from the device encoder (lossy, several times smaller); the masks stay "
                        "PNG. Defaults to png")
    parser.add_argument("--jpeg_quality", type=int, default=argparse.SUPPRESS,
                        help="With --format jpg: libjpeg's quality scale, 1 to 100. Defaults to 90")
    parser.add_argument("--jpeg_subsampling", default=argparse.SUPPRESS, choices=("444", "420"),
                        help="With --format jpg: chroma at full resolution (444) or halved both ways (420). Defaults to 444")
    parser.add_argument("--decode", default=argparse.SUPPRESS, choices=("host", "device"),
                        help="Not an option of the reference's script: where the input files are decoded. device: baseline "
                        "JPEG files and 8-bit RGB PNG files are uploaded as bytes and decoded by the device decoders; every "
                        "other file (RGBA, interlaced or palette PNG, progressive JPEG), and any the device reports as "
                        "corrupt, is read on the host as with host. Defaults to host")
    args = parser.parse_args(argv, namespace=_Args())
    given = vars(args)
    if args.format != "jpg" and ("jpeg_quality" in given or "jpeg_subsampling" in given):
        parser.error("--jpeg_quality and --jpeg_subsampling need --format jpg")
    if not 1 <= args.jpeg_quality <= 100:
        parser.error("--jpeg_quality must be between 1 and 100")
    if args.batch_size < 1:
        parser.error("--batch_size must be positive")
    if args.zip_outdir and args.output_path is None:
        parser.error("--zip_outdir needs --output_path")
    return args


def validate_sizes(batch_size, target_size, keep_ratio, max_im_width):
    """apply_events.py:407-429 -> (batch_size, target_size, max_im_width) as the run uses them."""
    if keep_ratio:
        if target_size != 640:
            print("\nWARNING: using --keep_ratio_128 overwrites target_size which is ignored.")
        if batch_size != 1:
            print("\nWARNING: batch_size overwritten to 1 when using keep_ratio_128")
            batch_size = 1
        if max_im_width > 0 and max_im_width % 128 != 0:
            new_im_width = int(max_im_width / 128) * 128
            print("\nWARNING: max_im_width should be <0 or a multiple of 128.")
            print("            Was {} but is now overwritten to {}".format(max_im_width, new_im_width))
            max_im_width = new_im_width
    elif target_size % 128 != 0:
        print("\nWarning: target size %d is not a multiple of 128." % target_size)
        target_size = target_size - (target_size % 128)
        print("Setting target_size to %d." % target_size)
    return batch_size, target_size, max_im_width


def get_outdir_name(half, keep_ratio, max_im_width, target_size, bin_value, cloudy):
    """apply_events.py:308-327: the output directory's name from the arguments."""
    name_items = []
    if half:
        name_items.append("half")
    if keep_ratio:
        name_items.append("AR")
    if max_im_width and keep_ratio:
        name_items.append("%s" % max_im_width)
    if target_size and not keep_ratio:
        name_items.append("S")
        name_items.append("%s" % target_size)
    if bin_value != 0.5:
        name_items.append("bin%s" % bin_value)
    if not cloudy:
        name_items.append("no_cloudy")
    return "-".join(name_items)


def make_outdir(outdir, overwrite, half, keep_ratio, max_im_width, target_size, bin_value, cloudy):
    """apply_events.py:330-353.  A directory called ``_auto_`` becomes ``outdir.parent / get_outdir_name(...)``.  Where the
    reference asks ``Continue anyway? [y / n]`` about an existing directory, this refuses: nobody answers a prompt in a
    batch job; pass ``--overwrite`` to write into it."""
    outdir = Path(outdir)
    if outdir.name == "_auto_":
        outdir = outdir.parent / get_outdir_name(half, keep_ratio, max_im_width, target_size, bin_value, cloudy)
    if outdir.exists() and not overwrite:
        raise SystemExit("apply_events: outdir (%s) already exists; pass --overwrite to write into it (files with existing "
                         "names will be overwritten)" % outdir)
    outdir.mkdir(exist_ok=True, parents=True)
    return outdir


def get_time_stores(import_time):
    """apply_events.py:356-374."""
    return OrderedDict((k, [import_time] if k == "imports" else []) for k in (
        "imports", "setup", "data pre-processing", "encode", "mask", "flood", "depth", "segmentation", "smog", "wildfire",
        "all events", "numpy", "inference on all images", "write"))


def print_store(store, purge=-1):
    """apply_events.py:244-291: single measurements, then mean +/- std of the series, in s/batch."""
    def line(text, series):
        if purge > 0 and len(series) > purge:
            series = series[purge:]
        print("%s  %.5f%s" % ("{:.<26}".format(text.capitalize() + " "), np.mean(series),
                              " +/- %.5f" % np.std(series) if len(series) > 1 else ""))

    empties = [k for k, v in store.items() if len(v) == 0]
    if empties:
        print("Ignoring empty stores ", ", ".join(empties))
        print()
    for k, v in store.items():
        if len(v) == 1:
            line(k, v)
    print()
    print("Unit: s/batch")
    for k, v in store.items():
        if len(v) > 1:
            line(k, v)
    print()


def select_paths(paths, n_images):
    """apply_events.py:479-485: the first ``n_images`` paths, the list repeated when it is shorter."""
    paths = list(paths)
    if 0 < n_images < len(paths):
        return paths[:n_images]
    if n_images > len(paths) > 0:
        repeats = n_images // len(paths) + 1
        return (paths * repeats)[:n_images]
    return paths


def rgba_to_rgb(im):
    """apply_events.py:491, ``uint8(rgba2rgb(im) * 255)``: the image blended over a white background in float64,
    ``(1 - a) + a * rgb`` on [0, 1] values, then truncated.  scikit-image is not a dependency here, so this restates its
    formula and is not pinned against it by a test."""
    f = im.astype(np.float64) / 255.0
    a = f[..., 3:4]
    return (np.clip((1.0 - a) + a * f[..., :3], 0.0, 1.0) * 255).astype(np.uint8)


def read_image(path):
    """An RGB uint8 [H, W, 3] array; RGBA is blended over white, grey files are refused."""
    from PIL import Image

    a = np.asarray(Image.open(path))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("apply_events: %s is not an 8-bit RGB or RGBA image (shape %s, %s)" % (path, a.shape, a.dtype))
    return a if a.shape[2] == 3 else rgba_to_rgb(a)


def read_images(paths, decode="host", device="cuda"):
    """The batch's images, each uint8 [H, W, 3]: host arrays from ``read_image``, or with ``decode="device"`` device tensors
    from ``jpeg.decode`` for the files ``jpeg.probe`` accepts as 3-component baseline JPEG and from
    ``png.decode`` for those ``png.probe`` accepts as 8-bit RGB.  Everything else -- RGBA (blended on the host),
    interlaced or palette PNG, progressive JPEG, a file the device reports as corrupt or not converged -- goes through
    ``read_image`` unchanged; a grey file is refused with ``read_image``'s message in both modes."""
    if decode != "device":
        return [read_image(p) for p in paths]
    from . import jpeg, png

    datas = [Path(p).read_bytes() for p in paths]
    images = [None] * len(paths)
    for codec, channels in ((jpeg, "ncomp"), (png, "channels")):
        pick = [i for i, data in enumerate(datas) if getattr(codec.probe(data)[0], channels, 0) == 3]
        if pick:
            for i, im in zip(pick, codec.try_decode([datas[i] for i in pick], device=device)[0]):
                images[i] = im
    return [read_image(p) if im is None else im for p, im in zip(paths, images)]


def event_file_name(stem, event, width, keep_ratio, no_cloudy, ext="png"):
    """apply_events.py:590-616; ``ext``: "jpg" for the files ``--format jpg`` writes."""
    suffix = ("_AR" if keep_ratio else "") + ("_no_cloudy" if no_cloudy else "")
    return "%s_%s_%s%s.%s" % (stem, event, width, suffix, ext)


def get_git_revision_hash():
    """This repository's commit, or "unknown" outside git."""
    try:
        out = subprocess.run(["git", "-C", str(Path(__file__).resolve().parent), "rev-parse", "HEAD"], capture_output=True,
                             text=True, timeout=30)
        return out.stdout.strip() if out.returncode == 0 and out.stdout.strip() else "unknown"
    except (OSError, subprocess.SubprocessError):
        return "unknown"


def write_apply_config(out, argv):
    """apply_events.py:294-305."""
    command = "cd %s\n" % Path.cwd().expanduser().resolve()
    command += " ".join(argv)
    (out / "command.txt").write_text(command)
    (out / "hash.txt").write_text(get_git_revision_hash())


def events_to_uint8(events, x, save_input):
    """``infer_all(numpy=False)``'s dict -> {name: uint8 [N, H, W, C] device tensor}, what its ``numpy=True`` branch hands to
    the host (trainer.py:311-332).  The mask comes back from ``infer_all`` already binarised by ``ops.binarize(...,
    want_uint8=True)`` but as a host array [N, 1, H, W] (``infer_all`` is shared with the reference's callers and stays as it
    is), so it is uploaded again: one byte per pixel.  ``input``: apply_events.py:539, ``uint8((x + 1) / 2 * 255)``."""
    out = OrderedDict()
    for name, ev in events.items():
        if name == "mask":
            m = torch.from_numpy(ev).to(x.device)
            out[name] = m.reshape(m.shape[0], m.shape[2], m.shape[3], 1)
        else:
            out[name] = ops.normalize_to_uint8(ev)
    if save_input:
        out["input"] = ((x.float() + 1) / 2 * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return out


def main(argv=None):
    args = parse_args(argv)
    print("\u2022 Using args\n\n" + "\n".join(["{:25}: {}".format(k, v) for k, v in vars(args).items()]))
    bin_value = args.flood_mask_binarization
    cloudy = not args.no_cloudy
    keep_ratio = args.keep_ratio_128
    time_inference = not args.no_time
    batch_size, target_size, max_im_width = validate_sizes(args.batch_size, args.target_size, keep_ratio, args.max_im_width)
    outdir = None
    if args.output_path is not None:
        outdir = make_outdir(Path(args.output_path).expanduser().resolve(), args.overwrite, args.half, keep_ratio,
                             max_im_width, target_size, bin_value, cloudy)

    import_time = time.time()
    from . import jpeg, png
    from .bn_fusion import bn_fuse
    from .eval_masker import find_images
    from .trainer import Timer, Trainer

    stores = get_time_stores(time.time() - import_time)

    def timed(key):
        return Timer(store=stores[key], ignore=not time_inference)

    with timed("setup"):
        print("\n\u2022 Initializing trainer\n")
        torch.set_grad_enabled(False)
        trainer = Trainer.resume_from_path(args.resume_path, setup=True, inference=True, new_exp=None,
                                           device=torch.device("cuda", torch.cuda.current_device()))
        if args.fuse:
            trainer.G = bn_fuse(trainer.G)
        if args.dtype:
            trainer.G.set_compute_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype])

    print("\n\u2022 Reading & Pre-processing Data\n")
    base_data_paths = find_images(Path(args.images_paths).expanduser().resolve())
    if not base_data_paths:
        raise SystemExit("apply_events: no images in %s" % args.images_paths)
    data_paths = select_paths(base_data_paths, args.n_images)
    print("Found", len(base_data_paths), "images. Inferring on", len(data_paths), "images.")
    print("\n\u2022 Using device %s\n" % trainer.device)
    if outdir is not None:
        print("\n\u2022 Output directory:\n")
        print(str(outdir), "\n")

    # per-stage times need a device drain around every stage; without them infer_all runs its branches side by side
    stage_stores = stores if time_inference else {}
    with timed("inference on all images"):
        for b in range(0, len(data_paths), batch_size):
            paths = data_paths[b:b + batch_size]
            with timed("data pre-processing"):
                images = read_images(paths, args.decode, trainer.device)
                if keep_ratio:
                    x = torch.stack([resize_keep_ratio(im, max_im_width, device=trainer.device) for im in images])
                else:
                    x = prepare_batch(images, to=target_size, device=trainer.device)
            events = trainer.infer_all(x, numpy=False, stores=stage_stores, bin_value=bin_value, half=args.half,
                                       cloudy=cloudy, return_masks=args.save_masks)
            if outdir is None:
                continue
            with timed("write"):
                width = x.shape[-1]
                for event, im_u8 in events_to_uint8(events, x, args.save_input).items():
                    as_jpeg = args.format == "jpg" and event != "mask"         # a binary mask must not be lossy
                    names = [outdir / event_file_name(Path(p).stem, event, width, keep_ratio, args.no_cloudy,
                                                      "jpg" if as_jpeg else "png") for p in paths]
                    if as_jpeg:
                        jpeg.write(im_u8, names, quality=args.jpeg_quality, subsampling=args.jpeg_subsampling)
                    else:
                        png.write(im_u8, names, level=args.png_level)

    if args.zip_outdir:
        print("\n\u2022 Zipping output directory... ", end="", flush=True)
        archive_path = Path(shutil.make_archive(str(outdir.parent / outdir.name), "zip", root_dir=outdir))
        print("Done:\n")
        print(str(archive_path))
    if time_inference:
        print("\n\u2022 Timings\n")
        print_store(stores)
    if not args.no_conf and outdir is not None:
        write_apply_config(outdir, sys.argv if argv is None else ["apply_events"] + list(argv))
    return outdir


if __name__ == "__main__":
    main()
