"""The metric half of the reference's ``eval_masker.py``: evaluate trained Maskers on a labelled test set.

    python -m climategan_amd.eval_masker --model RUN --images_dir I --labels_dir L [--write_metrics]

Same pairing (images sorted by name, labels sorted with ``_labeled.`` removed, matched by position, eval_masker.py:423-430),
same pre-processing (the image resize + centre crop of ``apply_events.prepare_batch``; the label's nearest-neighbour resize,
crop and colour encoding in one kernel, ``eval_metrics.crop_resize_encode_label``), same binarisation (eval_masker.py:507-508)
and the same CSV (``<model>/eval-metrics/eval_masker.csv``, ``index_label="idx"``).  Masks come from ``G.mask`` in batches
and every metric of a batch from one ``eval_metrics.masker_eval`` call.

Not built: comet logging, plots and the painted-image log; their arguments are refused.  Where the reference stops at an
image it rejects (an absent label class trips its assertions; prediction edges without a "must" label edge make
``euclidean_distances`` raise), this script reports the image and writes nan in its row.
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

from . import eval_metrics

IMG_EXTENSIONS = {".jpg", ".JPG", ".jpeg", ".JPEG", ".png", ".PNG", ".ppm", ".PPM", ".bmp", ".BMP"}   # utils.py:31-33
REFUSED = {
    "--tags": "comet tags: this script does not log to comet",
    "-t": "comet tags: this script does not log to comet",
    "--plot": "the matplotlib figures are not built",
    "--no_paint": "the painted-image log is not built (nothing is painted)",
    "--prepare_torch": "only the reference's default crop_and_resize pre-processing is built",
    "--output_csv": "the multi-model comparison plots are not built",
}
DTYPES = ("fp16", "bf16", "split24")


def parse_args(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    for a in argv:
        key = a.split("=", 1)[0]
        if key in REFUSED:
            raise SystemExit("eval_masker: %s is not supported here: %s" % (key, REFUSED[key]))
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--model", type=str, help="Path to a run directory (opts.yaml + checkpoints/)")
    parser.add_argument("--images_dir", type=str, required=True, help="Directory containing the original test images")
    parser.add_argument("--labels_dir", type=str, required=True, help="Directory containing the labeled images")
    parser.add_argument("--image_size", default=640, type=int, help="The height and width of the pre-processed images")
    parser.add_argument("--max_files", default=-1, type=int, help="Limit loaded samples")
    parser.add_argument("--bin_value", default=0.5, type=float, help="Mask binarization threshold")
    parser.add_argument("-y", "--yaml", default=None, type=str, help="load a yaml file to parametrize the evaluation")
    parser.add_argument("--write_metrics", action="store_true", default=False,
                        help="If True, write CSV file and maps images in model's path directory")
    parser.add_argument("--load_metrics", action="store_true", default=False,
                        help="If True, load predictions and metrics instead of re-computing")
    parser.add_argument("--batch_size", default=16, type=int, help="Images per Masker forward and per metric call")
    parser.add_argument("--dtype", default="split24", choices=DTYPES,
                        help="G.set_compute_dtype mode (split24: fp32-grade masks, the reference evaluates in fp32)")
    args = parser.parse_args(argv)
    if args.image_size != 640:
        parser.error("--image_size: the reference's crop_and_resize always produces 640 x 640 (eval_masker.py:190-215)")
    if not args.model and not args.yaml:
        parser.error("one of --model or --yaml is required")
    if args.batch_size < 1:
        parser.error("--batch_size must be positive")
    return args


def find_images(path):
    """utils.py:1018-1032 (non-recursive)."""
    p = Path(path)
    assert p.exists()
    assert p.is_dir()
    return [i for i in p.glob("*") if i.is_file() and i.suffix in IMG_EXTENSIONS]


def pair_paths(images_dir, labels_dir, max_files=-1):
    """eval_masker.py:423-430: images by name, labels by name without ``_labeled.``, matched by position."""
    imgs = sorted(find_images(images_dir), key=lambda x: x.name)
    labels = sorted(find_images(labels_dir), key=lambda x: x.name.replace("_labeled.", "."))
    if max_files > 0:
        imgs, labels = imgs[:max_files], labels[:max_files]
    return imgs, labels


def read_rgb(path, what):
    """An RGB uint8 [H, W, 3] array; RGBA and grey files are refused (the reference crashes on an RGBA label in
    encode_mask_label and sends an RGBA image through a float rgba2rgb this script does not restate)."""
    from PIL import Image

    a = np.asarray(Image.open(path))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("eval_masker: %s %s is not an 8-bit RGB image (shape %s, %s); convert it to RGB first"
                         % (what, path, a.shape, a.dtype))
    return a


def evaluations(args):
    if args.yaml:
        import yaml

        y_path = Path(args.yaml)
        assert y_path.exists()
        assert y_path.suffix in {".yaml", ".yml"}
        data = yaml.safe_load(y_path.read_text())
        assert "models" in data
        return list(data["models"])
    return [args.model]


def load_test_set(img_paths, label_paths):
    imgs = [read_rgb(p, "image") for p in img_paths]
    labels = []
    for img, lp in zip(imgs, label_paths):
        lab = read_rgb(lp, "label")
        labels.append(eval_metrics.crop_resize_encode_label(lab, image_hw=img.shape[:2], to=640))
    return imgs, labels


def compute_metrics(G, imgs, labels, bin_value, batch_size, want_maps=False):
    """Masks of every image (G.mask on batches of ``batch_size``) and the per-image metrics -> (columns dict of numpy
    float64 arrays, status array, [(pred numpy, maps dict)] when ``want_maps``)."""
    from .apply_events import prepare_batch

    cols = {k: [] for k in eval_metrics.COLUMNS}
    status, extras = [], []
    for b in range(0, len(imgs), batch_size):
        x = prepare_batch(imgs[b:b + batch_size])
        with torch.no_grad():
            m = G.mask(x=x)[:, 0].float().contiguous()
        lab = torch.stack(labels[b:b + batch_size])
        r = eval_metrics.masker_eval(m, lab, bin_value=bin_value, maps=want_maps)
        for k in eval_metrics.COLUMNS:
            cols[k].append(r[k].numpy())
        status.append(r["status"].numpy())
        if want_maps:
            pred = (m > bin_value) if bin_value > 0 else m
            pred_np = pred.cpu().numpy()
            maps = r["maps"].cpu().numpy()
            for i in range(pred_np.shape[0]):
                extras.append((pred_np[i], {name: maps[k, i] for k, name in enumerate(eval_metrics._MAP_NAMES)}))
    return {k: np.concatenate(v) for k, v in cols.items()}, np.concatenate(status), extras


def write_maps(out_dir, stem, pred, maps):
    """eval_masker.py:610-626: ``pred.astype(uint8)`` and each map's ``astype(uint8)`` as PNG."""
    from PIL import Image

    pred_out = out_dir / "pred"
    pred_out.mkdir(exist_ok=True)
    Image.fromarray(pred.astype(np.uint8)).save(pred_out / ("%s_pred.png" % stem))
    for k, v in maps.items():
        metric_out = out_dir / k
        metric_out.mkdir(exist_ok=True)
        Image.fromarray(v.astype(np.uint8)).save(metric_out / ("%s_%s.png" % (stem, k)))


def make_frame(cols, names):
    import pandas as pd

    df = pd.DataFrame({k: cols[k] for k in eval_metrics.COLUMNS})
    df["filename"] = names
    return df


def summarize(df):
    """The printed summary of eval_masker.py:636-644: column means, mean and std confusion matrices (3 decimals)."""
    means = df[list(eval_metrics.COLUMNS)].mean(axis=0)
    print(means.to_string())
    cm, cs = eval_metrics.get_confusion_matrix(df.tpr, df.tnr, df.fpr, df.fnr, df.mpr, df.mnr)
    print("Confusion matrix (mean) [pred, true], classes Cannot / Must / May:")
    print(np.around(cm, decimals=3))
    print("Confusion matrix (std):")
    print(np.around(cs, decimals=3))
    return means, cm, cs


def main(argv=None):
    args = parse_args(argv)
    print("Args:\n" + "\n".join(["    {:20}: {}".format(k, v) for k, v in vars(args).items()]))
    img_paths, label_paths = pair_paths(args.images_dir, args.labels_dir, args.max_files)
    if len(img_paths) != len(label_paths):
        raise SystemExit("eval_masker: %d images but %d labels" % (len(img_paths), len(label_paths)))
    if not img_paths:
        raise SystemExit("eval_masker: no images in %s" % args.images_dir)
    names = [p.name for p in img_paths]
    imgs = labels = None                             # loaded for the first model that is not skipped
    from .trainer import Trainer

    frames = []
    for e, eval_path in enumerate(evaluations(args)):
        print("\n>>>>> Evaluation", e, ":", eval_path)
        out_dir = Path(eval_path) / "eval-metrics"
        out_dir.mkdir(exist_ok=True)
        if args.load_metrics:
            if (out_dir / "eval_masker.csv").exists() and (out_dir / "pred").exists():
                print("Skipping model because pre-computed metrics exist")
                continue
        if imgs is None:
            print("Loading %d images and labels..." % len(img_paths))
            imgs, labels = load_test_set(img_paths, label_paths)
        trainer = Trainer.resume_from_path(eval_path, inference=True, new_exp=None,
                                           device=torch.device("cuda", torch.cuda.current_device()))
        trainer.G.set_compute_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}.get(args.dtype, args.dtype))
        cols, status, extras = compute_metrics(trainer.G, imgs, labels, args.bin_value, args.batch_size,
                                               want_maps=args.write_metrics)
        for i in np.nonzero(status)[0]:
            why = []
            if status[i] & eval_metrics.STATUS_ASSERT:
                why.append("a label class is absent (the reference's masker_classification_metrics asserts)")
            if status[i] & eval_metrics.STATUS_NO_LABEL_EDGE:
                why.append("prediction edges but no must-flood label edge (the reference's edge coherence raises)")
            print("WARNING: %s: %s; its row is nan" % (names[i], "; ".join(why)), file=sys.stderr)
        df = make_frame(cols, names)
        if args.write_metrics:
            for (pred, maps), p in zip(extras, img_paths):
                write_maps(out_dir, p.stem, pred, maps)
            print("Writing metrics in %s" % out_dir)
            df.to_csv(out_dir / "eval_masker.csv", index_label="idx")
        if (status == 0).any():                     # the summary of the images the reference accepts
            summarize(df[status == 0])
        frames.append(df)
    return frames


if __name__ == "__main__":
    main()
