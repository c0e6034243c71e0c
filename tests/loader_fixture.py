"""The small dataset on disk that the loader tests share (test_data_loaders_host.py, test_gpu_data_loaders.py,
test_gpu_train_loop.py): ``write(root)`` fills ``root`` with four domains (r, s, rf, kitti) of five samples each, of five
source sizes, in the file kinds tests/data_decode_cases.py covers, and the file lists that name them.  The pixels come from
``climategan_amd.fill`` through that module's builders."""
import json
import os

import numpy as np
import yaml

import data_decode_cases as cases
from climategan_amd.config import default_opts

SIZES = [(24, 40), (40, 24), (33, 33), (64, 48), (48, 64)]
DOMAINS = ("r", "s", "rf", "kitti")
BATCH = 2
ENV = "CGAN_LOADER_FIXTURE"            # the variable the one ``$VAR`` list entry names
# resize (short side 32) -> crop 16 -> hflip -> the three jitters: every branch of ``transforms.Plan`` within one batch
ITEMS = [{"name": "resize", "ignore": False, "new_size": 32, "keep_aspect_ratio": True},
         {"name": "crop", "ignore": False, "center": "val", "height": 16, "width": 16},
         {"name": "hflip", "ignore": "val", "p": 0.5},
         {"name": "brightness", "ignore": "val"}, {"name": "saturation", "ignore": "val"}, {"name": "contrast", "ignore": "val"}]


def palette_rgba(name, classes, h, w):
    """colour-coded segmentation image: palette colours, a third of them perturbed (any alpha)"""
    cols = np.array([list(c)[:4] for c in classes.values()], np.int64)
    out = cols[np.floor(cases._u(name, (h, w)) * len(cols)).astype(np.int64)]
    noise = np.floor(cases._u(name + ".noise", (h, w, 4)) * 61).astype(np.int64) - 30
    noisy = cases._u(name + ".sel", (h, w)) > 0.66
    out[noisy] = np.clip(out[noisy] + noise[noisy], 0, 255)
    return out.astype(np.uint8)


def real_depth(name, h, w):
    from climategan_amd import fill
    return fill.uniform((h, w), fill.key_seed("loader." + name, 5), 0.25, 80.0).astype(np.float32)


def _save(path, arr):
    from PIL import Image
    if path.suffix == ".npy":
        np.save(path, arr)
    else:
        Image.fromarray(arr).save(path)
    return str(path)


def sample_files(root, mode, domain, k, classes_dict):
    """write sample ``k`` and return {task: path}"""
    h, w = SIZES[k]
    tag = "%s.%s.%d" % (mode, domain, k)
    d = root / mode / domain
    d.mkdir(parents=True, exist_ok=True)
    npy = k % 2 == 1                                            # odd samples hold their labels / depth as .npy
    out = {"x": _save(d / ("x%d.png" % k), cases.x_image(tag + ".x", h, w, channels=4 if k == 1 else 3)),
           "m": _save(d / ("m%d.png" % k), cases.mask(tag + ".m", 255, h=h, w=w))}
    if domain == "rf":
        return out
    if domain == "kitti":
        out["d"] = _save(d / ("d%d.%s" % (k, "npy" if npy else "png")), cases.kitti_depth(tag + ".d", h, w))   # 16-bit PNG
        out["s"] = _save(d / ("s%d.png" % k), cases.kitti_seg(tag + ".s", classes_dict["kitti"], h, w))
        return out
    if domain == "s":
        out["d"] = _save(d / ("d%d.png" % k), cases.unity(tag + ".d", h, w))
    else:
        out["d"] = _save(d / ("d%d.npy" % k), real_depth(tag + ".d", h, w))
    out["s"] = _save(d / ("s%d.%s" % (k, "npy" if npy else "png")), palette_rgba(tag + ".s", classes_dict[domain], h, w))
    return out


def write(root):
    """The files and the lists; returns {mode: {domain: [{task: path}]}} as listed.  train/r is a JSON list found through
    ``data.files.base``, train/s a YAML list, train/rf's first ``x`` names its directory as ``$CGAN_LOADER_FIXTURE``."""
    from climategan_amd import data
    listed = {}
    lists = root / "lists"
    lists.mkdir(parents=True, exist_ok=True)
    for mode in ("train", "val"):
        listed[mode] = {}
        for domain in DOMAINS:
            samples = [sample_files(root, mode, domain, k, data.classes_dict) for k in range(len(SIZES))]
            if (mode, domain) == ("train", "rf"):
                samples[0]["x"] = samples[0]["x"].replace(str(root / mode / domain), "$" + ENV)
            listed[mode][domain] = samples
            if (mode, domain) == ("train", "s"):
                (lists / "train_s.yaml").write_text(yaml.safe_dump(samples))
            else:
                (lists / ("%s_%s.json" % (mode, domain))).write_text(json.dumps(samples))
    os.environ[ENV] = str(root / "train" / "rf")
    return listed


def files_opts(root):
    lists = root / "lists"
    return {"base": str(lists),
            "train": {"r": "train_r.json", "s": "train_s.yaml", "rf": str(lists / "train_rf.json"),
                      "kitti": str(lists / "train_kitti.json")},
            "val": {d: str(lists / ("val_%s.json" % d)) for d in DOMAINS}}


def fixture_opts(root, tasks=("d", "s", "m"), items=ITEMS, num_workers=4):
    """``default_opts()`` + what the loaders and the loop read, on the fixture"""
    opts = default_opts()
    opts.tasks = list(tasks)
    opts.data = {"files": files_opts(root), "max_samples": -1, "check_samples": False, "normalization": "default",
                 "loaders": {"batch_size": BATCH, "num_workers": num_workers}, "transforms": [dict(i) for i in items]}
    opts.train.kitti = {"pretrain": False, "epochs": 10, "batch_size": 1}
    opts.train.pseudo = {"tasks": [], "epochs": 10}
    opts.train.epochs = 2
    opts.train.fid = {"n_images": 3}
    opts.comet = {"display_size": 2}
    return opts
