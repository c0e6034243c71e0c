"""The cases of tests/golden/data_transforms.npz, shared by the script that writes the fixture from the real reference
(tests/devtools/make_golden_data_transforms.py) and the tests that read it (test_data_transforms_host.py,
test_gpu_data_transforms.py).  Inputs come from ``climategan_amd.fill``, so the fixture holds outputs only."""
import random

import numpy as np

from climategan_amd import fill
from climategan_amd.config import Opts

JITTER = [{"name": "brightness", "ignore": "val"}, {"name": "saturation", "ignore": "val"},
          {"name": "contrast", "ignore": "val"}]


def pipeline(first, crop, last, flip_after_resize=False):
    """The shape of the reference's default item list (shared/trainer/defaults.yaml:43-67) at other sizes"""
    flip = {"name": "hflip", "ignore": "val", "p": 0.5}
    resize = {"name": "resize", "ignore": False, "new_size": first, "keep_aspect_ratio": True}
    return ([resize, flip] if flip_after_resize else [flip, resize]) + [
        {"name": "crop", "ignore": False, "center": "val", "height": crop, "width": crop}] + JITTER + [
        {"name": "resize", "ignore": False, "new_size": last}]


DEFAULT_ITEMS = pipeline(640, 600, {"default": 640, "d": 160, "s": 160})      # defaults.yaml:43-67, checked by the script
SMALL = pipeline(64, 60, {"default": 64, "d": 16, "s": 16})
ALL = ("x", "m", "d", "s")


def same(tasks, h, w):
    return {t: (h, w) for t in tasks}


# name -> dict(items, mode, domain, samples = [{task: (H, W)}], seed; optional: normalization, classify, s_int64, sub)
# seed None: searched by the script (the first seed whose first draw flips / does not flip) and stored in the fixture
CASES = {
    "default_train": dict(items=SMALL, mode="train", samples=[same(ALL, 130, 90)], seed=1),                 # portrait
    "default_val": dict(items=SMALL, mode="val", samples=[same(ALL, 90, 130)], seed=2),                     # landscape
    "flip_true": dict(items=SMALL, mode="train", samples=[same(ALL, 90, 131)], seed=None, want_flip=True),
    "flip_false": dict(items=SMALL, mode="train", samples=[same(ALL, 91, 130)], seed=None, want_flip=False),
    "square": dict(items=SMALL, mode="train", samples=[same(ALL, 100, 100)], seed=5),     # keep_aspect_ratio: else branch
    "m_other_res": dict(items=SMALL, mode="train", seed=6,
                        samples=[{"x": (90, 130), "m": (45, 65), "d": (61, 83), "s": (180, 260)}]),
    "hflip_after_resize": dict(items=pipeline(64, 60, {"default": 64, "d": 16, "s": 16}, True), mode="train",
                               samples=[same(ALL, 90, 130)], seed=7),
    "one_resize": dict(items=[{"name": "hflip", "p": 0.5}, {"name": "crop", "center": "val", "height": 60, "width": 70},
                              {"name": "resize", "new_size": {"default": 32, "d": 8}}],
                       mode="train", samples=[same(ALL, 90, 130)], seed=8),
    "three_resizes": dict(items=[{"name": "resize", "new_size": 80, "keep_aspect_ratio": True},
                                 {"name": "crop", "center": "val", "height": 72, "width": 76},
                                 {"name": "hflip", "p": 0.5},
                                 {"name": "resize", "new_size": 64},
                                 {"name": "crop", "center": "val", "height": 60, "width": 58},
                                 {"name": "resize", "new_size": {"default": 48, "d": 12, "s": 12}}],
                          mode="train", samples=[same(ALL, 90, 130), same(ALL, 120, 100)], seed=9),
    "dict_only": dict(items=[{"name": "resize", "new_size": {"default": 40, "d": 10, "s": 10}}], mode="train", seed=10,
                      samples=[{"x": (90, 130), "m": (33, 47), "d": (70, 20), "s": (90, 130)}]),
    "int64_s": dict(items=SMALL, mode="train", samples=[same(("m", "s"), 90, 130)], seed=11, s_int64=True),
    "hrnet": dict(items=SMALL, mode="train", samples=[same(("x", "m"), 90, 130)], seed=12, normalization="HRNet"),
    "bucketize_on": dict(items=SMALL, mode="train", samples=[same(("d", "m"), 90, 130)], seed=13, classify=True, domain="s"),
    "bucketize_off": dict(items=SMALL, mode="train", samples=[same(("d", "m"), 90, 130)], seed=14, classify=True, domain="r"),
    "out_w1": dict(items=[{"name": "hflip", "p": 0.5}, {"name": "resize", "new_size": [9, 1]}], mode="train",
                   samples=[same(ALL, 30, 40)], seed=15),
    "out_h1": dict(items=[{"name": "resize", "new_size": 20, "keep_aspect_ratio": True},
                          {"name": "resize", "new_size": [1, 9]}], mode="train", samples=[same(ALL, 30, 40)], seed=16),
    "mixed_batch": dict(items=SMALL, mode="train", seed=17,
                        samples=[same(ALL, 130, 90), {"x": (90, 130), "m": (45, 65), "d": (90, 130), "s": (64, 64)},
                                 same(ALL, 100, 100)]),
    # the default sizes; the fixture keeps every 9th row and 7th column of each output
    "default_640": dict(items=DEFAULT_ITEMS, mode="train", samples=[same(ALL, 723, 1101)], seed=18, sub=(9, 7)),
}

# source shapes whose Resize(640, keep_aspect_ratio=True).compute_new_default_size the fixture records
NEW_SIZE_SHAPES = [(723, 1101), (1101, 723), (700, 700), (1200, 1800), (90, 130), (641, 640), (333, 1000), (1000, 333)]


def case_opts(case, tasks=("d", "s", "m", "p")):
    """The options ``get_transforms`` reads, as plain data (``Opts`` here, the reference's addict stand-in in the script)"""
    return {"tasks": list(tasks),
            "data": {"normalization": case.get("normalization", "default"), "transforms": case["items"]},
            "gen": {"d": {"classify": {"enable": bool(case.get("classify", False)),
                                       "linspace": {"min": 0.35, "max": 6.95, "buckets": 256}}}}}   # defaults.yaml:129-134


def mirror_opts(case, tasks=("d", "s", "m", "p")):
    return Opts(case_opts(case, tasks))


def sample_inputs(name, k, shapes, s_int64=False):
    """{task: [1, C, H, W] numpy array} of sample ``k`` of case ``name``: x uniform in [0, 1), m binary, d uniform in
    [0, 7.5) (beyond both ends of the bucket range), s class ids 0..10 (fp32, or int64)"""
    out = {}
    for task, (h, w) in shapes.items():
        seed = fill.key_seed("%s.%d.%s" % (name, k, task), 3)
        if task == "x":
            out[task] = fill.uniform01((1, 3, h, w), seed).astype(np.float32)
        elif task == "m":
            out[task] = (fill.uniform01((1, 1, h, w), seed) > 0.5).astype(np.float32)
        elif task == "d":
            out[task] = fill.uniform((1, 1, h, w), seed, 0.0, 7.5)
        elif task == "s":
            ids = np.floor(fill.uniform01((1, 1, h, w), seed) * 11)
            out[task] = ids.astype(np.int64 if s_int64 else np.float32)
        else:
            raise KeyError(task)
    return out


def seed_all(seed):
    np.random.seed(seed)
    random.seed(seed)


def subsample(arr, sub):
    return arr if sub is None else arr[..., ::sub[0], ::sub[1]]
