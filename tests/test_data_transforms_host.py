"""Host side of the loaders' transforms (climategan_amd/transforms.py; reference climategan/transforms.py:22-289, 424-490):
the reduction of flip / crop / resize sequences to the kernel's plans, the item handling of get_transform(s), the draws,
and -- with the plans evaluated in numpy -- the reference's recorded d / m / s outputs.  No GPU here.
Fixture: tests/golden/data_transforms.npz (tests/devtools/make_golden_data_transforms.py, from the real reference)."""
import numpy as np
import pytest

import data_transform_cases as dc
from climategan_amd import transforms as T
from climategan_amd.config import Opts
from helpers import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "data_transforms.npz")


def near(idx, n_in, n_out):
    """F.interpolate(mode="nearest") in fp32: min((int)floorf(dst * scale), in - 1), scale = (float)in / out"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(idx.astype(np.float32) * scale).astype(np.int64), n_in - 1)


def eval_launches(launches, h, w):
    """(rows, cols) of the source pixel behind every output pixel, from the plans in the form the kernel reads them:
    stages (in_h, in_w, out_h, out_w), maps (row_off, col_off, flip), and for every index the bounds the C side checks"""
    rows_total, cols_total = np.arange(h), np.arange(w)
    for stages, maps, (oh, ow) in launches:
        assert len(stages) <= 2 and len(maps) == len(stages) + 1
        rows, cols = np.arange(oh), np.arange(ow)
        for k in range(len(stages), -1, -1):
            r0, c0, flip = maps[k]
            rows, cols = r0 + rows, (c0 - cols if flip else c0 + cols)
            lim_h, lim_w = (stages[k - 1][2:] if k else (len(rows_total), len(cols_total)))
            assert rows.min() >= 0 and rows.max() < lim_h and cols.min() >= 0 and cols.max() < lim_w
            if k:
                in_h, in_w, out_h, out_w = stages[k - 1]
                rows, cols = near(rows, in_h, out_h), near(cols, in_w, out_w)
        rows_total, cols_total = rows_total[rows], cols_total[cols]
    return rows_total, cols_total


def test_plan_reduction_equals_the_steps_on_every_pixel():
    """300 random pipelines of flips, crops (windows that leave the map and negative offsets included) and resizes in any
    order: the plan, split into launches of at most two stages, shows the same source pixel as the steps one by one"""
    rng = np.random.RandomState(0)
    done = 0
    most_stages = 0
    while done < 300:
        h, w = int(rng.randint(1, 40)), int(rng.randint(1, 40))
        plan = T.Plan(h, w)
        rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for _ in range(rng.randint(0, 9)):
            op = rng.randint(0, 3)
            ch, cw = rr.shape
            if op == 0:
                plan.flip()
                rr, cc = rr[:, ::-1], cc[:, ::-1]
            elif op == 1:
                top, left = int(rng.randint(-3, ch + 1)), int(rng.randint(-3, cw + 1))
                kh, kw = int(rng.randint(1, ch + 3)), int(rng.randint(1, cw + 3))
                rr, cc = (a[top:top + kh, left:left + kw] for a in (rr, cc))
                if rr.size == 0:                                  # an empty crop is refused, and only that
                    with pytest.raises(ValueError, match="is empty"):
                        plan.crop(top, left, kh, kw)
                    break
                plan.crop(top, left, kh, kw)
            else:
                nh, nw = int(rng.randint(1, 50)), int(rng.randint(1, 50))
                plan.resize(nh, nw)
                ri, ci = near(np.arange(nh), ch, nh), near(np.arange(nw), cw, nw)
                rr, cc = rr[np.ix_(ri, ci)], cc[np.ix_(ri, ci)]
        if rr.size == 0:
            continue
        rows, cols = eval_launches(plan.launches(), h, w)
        assert (plan.h, plan.w) == rr.shape == (len(rows), len(cols))
        assert np.array_equal(rows[:, None] + 0 * cols[None, :], rr) and np.array_equal(0 * rows[:, None] + cols[None, :], cc)
        most_stages = max(most_stages, len(plan.stages))
        done += 1
    assert most_stages >= 5          # launches through intermediate maps were part of it


def transforms_of(case, tasks=("d", "s", "m", "p"), draws=None):
    return T.get_transforms(dc.mirror_opts(case, tasks), case["mode"], case.get("domain", "r"), draws=draws)


def test_get_transforms_returns_the_reference_class_lists(golden):
    for name, case in dc.CASES.items():
        assert [type(t).__name__ for t in transforms_of(case)] == list(golden[name + ".classes"]), name
    for mode in ("train", "val"):
        for tag, tasks in (("p", ["d", "s", "m", "p"]), ("nop", ["d", "s", "m"])):
            opts = dc.mirror_opts(dc.CASES["default_640"], tasks)
            got = [type(t).__name__ for t in T.get_transforms(opts, mode, "r")]
            assert got == list(golden["classes.%s.%s" % (mode, tag)]), (mode, tag)
    # the jitter comes last before Normalize, in train mode without the Painter task only (transforms.py:482-485)
    assert list(golden["classes.train.nop"])[-5:] == ["RandBrightness", "RandSaturation", "RandContrast", "Normalize",
                                                      "BucketizeDepth"]
    assert "RandContrast" not in list(golden["classes.train.p"]) + list(golden["classes.val.nop"])


def test_get_transform_item_handling():
    item = lambda **kw: Opts(kw)   # noqa: E731
    c = T.get_transform(item(name="crop", height=5, width=7, center="val"), "val")
    assert isinstance(c, T.RandomCrop) and (c.h, c.w, c.center) == (5, 7, True)
    assert T.get_transform(item(name="crop", height=5, width=7, center="val"), "train").center is False
    assert T.get_transform(item(name="hflip"), "train").p == 0.5                    # p or 0.5
    assert T.get_transform(item(name="hflip", p=0), "train").p == 0.5
    assert T.get_transform(item(name="hflip", p=0.2), "train").p == 0.2
    assert T.get_transform(item(name="hflip", ignore="val"), "val") is None
    assert T.get_transform(item(name="hflip", ignore=True), "train") is None
    assert T.get_transform(item(name="nonsense", ignore="val"), "val") is None      # ignored before it is looked at
    with pytest.raises(ValueError, match="Unknown transform_item"):
        T.get_transform(item(name="nonsense", ignore="val"), "train")
    r = T.get_transform(item(name="resize", new_size=640, keep_aspect_ratio=True), "train")
    assert (r.h, r.w, r.default_h, r.default_w, r.sizes, r.keep_aspect_ratio) == (640, 640, 640, 640, {}, True)
    r = T.get_transform(item(name="resize", new_size={"default": 640, "d": 160}), "train")
    assert r.sizes == {"d": {"h": 160, "w": 160}} and r.keep_aspect_ratio is False
    assert r.compute_new_size_for_task("d") == (160, 160) and r.compute_new_size_for_task("m") == (640, 640)
    r = T.Resize([3, 4])
    assert (r.h, r.w, r.default_h, r.default_w) == (3, 4, 3, 4)
    assert T.interpolation("m") == {"mode": "nearest"} and T.interpolation("x") == {"mode": "bilinear", "align_corners": True}
    for name in ("brightness", "saturation", "contrast"):
        assert isinstance(T.get_transform(item(name=name, ignore="val"), "train"), T._RandJitter)
    # config.default_opts() has neither data.normalization nor gen.d.classify: default constants, no bucketize
    from climategan_amd.config import default_opts
    ts = T.get_transforms(default_opts(), "train", "s")
    assert [type(t).__name__ for t in ts] == ["Resize", "Normalize", "BucketizeDepth"]
    assert ts[1].std == (0.5, 0.5, 0.5) and ts[2].buckets is None


class LoggedDraws(T.PipelineDraws):
    def __init__(self):
        self.log = []

    def rand(self):
        v = super().rand()
        self.log.append(("rand", float(v)))
        return v

    def randint(self, low, high):
        v = super().randint(low, high)
        self.log.append(("randint", float(v)))
        return v

    def uniform(self, a, b):
        v = super().uniform(a, b)
        self.log.append(("uniform", float(v)))
        return v


class Shape:
    def __init__(self, h, w):
        self.shape = (1, 1, h, w)


def recorded(golden, name):
    return list(zip([str(k) for k in golden[name + ".draw_kinds"]], [float(v) for v in golden[name + ".draw_values"]]))


def test_default_draw_source_reproduces_the_recorded_draws(golden):
    for name, case in dc.CASES.items():
        draws = LoggedDraws()
        bt = T.BatchTransform(transforms_of(case, draws=draws))
        dc.seed_all(int(golden[name + ".seed"][0]))
        for shapes in case["samples"]:
            bt.plan_sample({task: Shape(*hw) for task, hw in shapes.items()})
        assert draws.log == recorded(golden, name), name
    assert recorded(golden, "default_val") == []                                   # centre crop, no flip: nothing drawn
    kinds = [k for k, _ in recorded(golden, "default_train")]
    assert kinds == ["rand", "randint", "randint"]                                 # flip, then top, then left
    assert recorded(golden, "flip_true")[0][1] <= 0.5 < recorded(golden, "flip_false")[0][1]


def test_jitter_draws_follow_the_geometry_per_sample():
    case = dc.CASES["default_train"]
    draws = LoggedDraws()
    bt = T.BatchTransform(transforms_of(case, tasks=("d", "s", "m"), draws=draws))
    dc.seed_all(3)
    _, factors = bt.plan_sample({task: Shape(90, 130) for task in dc.ALL})
    assert [k for k, _ in draws.log] == ["rand", "randint", "randint", "uniform", "uniform", "uniform"]
    assert factors == [v for k, v in draws.log if k == "uniform"] and all(0.5 <= f <= 1.5 for f in factors)
    import random
    random.seed(3)
    assert factors == [random.uniform(0.5, 1.5) for _ in range(3)]


def test_random_crop_window():
    c = T.RandomCrop(60)
    for H in (60, 59):                                   # np.random.randint(0, H - h): an empty range (transforms.py:169)
        with pytest.raises(ValueError):
            c.window(H, 100)
    with pytest.raises(ValueError):
        T.RandomCrop(60, center=False).window(100, 60)
    c.draws = T.RecordedPipelineDraws([("randint", 0), ("randint", 0)])
    with pytest.raises(ValueError):
        c.window(60, 100)                                # the replayed source raises like numpy
    np.random.seed(0)
    tops = {T.RandomCrop((4, 4)).window(6, 6)[0] for _ in range(200)}
    assert tops == {0, 1}                                # never the last offset, 2
    assert T.RandomCrop((60, 40), center=True).window(100, 101) == (20, 30)


def test_compute_new_default_size(golden):
    r = T.Resize(640, keep_aspect_ratio=True)
    got = [r.compute_new_default_size(Shape(h, w)) for h, w in dc.NEW_SIZE_SHAPES]
    assert got == [tuple(v) for v in golden["new_size"].tolist()]
    assert r.compute_new_default_size(Shape(700, 700)) == (640, 640)               # square: the else branch
    assert T.Resize(64).compute_new_default_size(Shape(5, 9)) == (64, 64)
    # the size comes from x (else the first entry) and goes to every task; a dict Resize ignores x's size
    sizes = T.Resize(64, True).new_sizes({"m": Shape(10, 10), "x": Shape(90, 130)})
    assert sizes == {"m": (64, 92), "x": (64, 92)}
    assert T.Resize(64, True).new_sizes({"m": Shape(10, 20), "d": Shape(90, 90)}) == {"m": (64, 128), "d": (64, 128)}
    assert T.Resize({"default": 8, "d": 2}).new_sizes({"x": Shape(90, 130), "d": Shape(3, 3)}) == {"x": (8, 8), "d": (2, 2)}


def test_plans_reproduce_the_reference_nearest_outputs(golden):
    """The recorded draws -> plans -> numpy gather of the fill inputs = the reference's d / m / s (and bucketized depth),
    every element equal: the host half of the pipeline is right before any kernel runs"""
    checked = 0
    for name, case in dc.CASES.items():
        draws = T.RecordedPipelineDraws(recorded(golden, name))
        ts = transforms_of(case, draws=draws)
        bt = T.BatchTransform(ts)
        bucket = ts[-1].buckets
        for k, shapes in enumerate(case["samples"]):
            plans, _ = bt.plan_sample({task: Shape(*hw) for task, hw in shapes.items()})
            src = dc.sample_inputs(name, k, shapes, case.get("s_int64", False))
            for task in shapes:
                if task == "x":
                    continue
                rows, cols = eval_launches(plans[task].launches(), *shapes[task])
                got = src[task][0][:, rows[:, None], cols[None, :]]
                if task == "d" and bucket is not None:
                    got = np.searchsorted(bucket.numpy(), got, side="right").astype(np.int32)
                want = golden["%s.%d.%s" % (name, k, task)]
                got = dc.subsample(got, case.get("sub"))
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, k, task)
                checked += 1
        assert draws.used == len(draws.draws), name
    assert checked >= 50
    assert golden["bucketize_on.0.d"].dtype == np.int32 and golden["bucketize_off.0.d"].dtype == np.float32
    assert golden["int64_s.0.s"].dtype == np.int64


def test_batch_transform_refuses_what_it_cannot_order():
    with pytest.raises(NotImplementedError):
        T.BatchTransform([T.Normalize(Opts()), T.Resize(8)])
    with pytest.raises(NotImplementedError):
        T.BatchTransform([lambda d: d])
    with pytest.raises(ValueError):
        T.BatchTransform([T.Resize(8)])([])
