"""Host side of the loaders' decode (climategan_amd.data, transforms.RawSource, the raw source kinds of cgan_data_transform):
the mirror's tables against the fixture's record of the reference's, a numpy restatement of each kind's decode formula (the
one csrc/data_tf.hip documents) against the reference's outputs in tests/golden/data_decode.npz, and the item-table
validation of the C entry points, which runs before anything touches a device."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import data_decode_cases as cases
from climategan_amd import _lib, data, ops
from climategan_amd.transforms import RawSource, Resize

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "data_decode.npz")


def test_tables_equal_the_reference(golden):
    for domain in ("s", "r", "kitti", "flood"):
        assert list(data.classes_dict[domain]) == golden["classes.%s.keys" % domain].tolist()
        assert list(data.classes_dict[domain].values()) == golden["classes.%s.colours" % domain].tolist()
    assert list(data.kitti_mapping.items()) == [tuple(r) for r in golden["kitti_mapping"].tolist()]


# ---- the kernel's decode, restated in numpy ------------------------------------------------------------------------------
def f32(v):
    return np.asarray(v, dtype=np.float32)


def np_minmax(v):
    """torch.min / torch.max: NaN wins"""
    return (f32(np.nan), f32(np.nan)) if np.isnan(v).any() else (v.min(), v.max())


def np_depth(kind, raw, log, normalize):
    with np.errstate(all="ignore"):
        if kind == "f32_d":
            mn, mx = np_minmax(raw)
            return (raw - mn) / f32(mx - mn)
        if kind == "unity_d":
            r, g, b = (raw[..., k].astype(np.int32) for k in range(3))
            trunc = lambda a: np.trunc(a / 8.0).astype(np.int32)          # noqa: E731  C's int division
            code = trunc(247 - r) * (256 * 31) + trunc(247 - g) * 256 + (255 - b)
            depth = code.astype(np.float32) / f32(246015) * f32(cases.FAR)
        else:
            depth = raw.astype(np.float32) / f32(100)
        if log:
            return np.log(depth.astype(np.float64)).astype(np.float32)
        v = f32(1) / depth
        if normalize:
            mn, mx = np_minmax(v)
            v = (v - mn) / f32(mx - mn)
        return v


def np_mask(raw):
    raw = raw[:, :, :3] if raw.ndim == 3 and raw.shape[2] == 4 else raw
    out = (raw > 127).astype(np.float32) if raw.max() > 127 else raw.astype(np.float32)
    return out[:, :, 0] if out.ndim == 3 else out


def np_seg_exact(raw, colours, classes, default):
    out = np.full(raw.shape[:2], default, np.float64)
    for col, cls in zip(colours, classes):
        out[(raw == np.array(col, np.uint8)).all(-1)] = cls
    return out


def np_seg_nearest(raw, colours, classes):
    d = ((raw.astype(np.int64)[:, :, None, :] - np.array(colours, np.int64)[None, None]) ** 2).sum(-1)
    return np.array(classes)[d.argmin(-1)].astype(np.float32)            # argmin: the first of equal distances


def np_decode(task, domain, raw, o):
    if task == "d":
        kind = {"s": "unity_d", "kitti": "kitti_d", "r": "f32_d"}[domain]
        return np_depth(kind, raw, o["log"], o["normalize"])[None, None]
    if task == "m":
        return np_mask(raw)[None, None]
    if task == "s" and domain == "kitti":
        cl = data.classes_dict["kitti"]
        merged = [data.kitti_mapping.get(c, 14) for c in cl]
        return np_seg_exact(raw, cl.values(), merged, data.kitti_mapping.get(14, 14))[None, None]
    if task == "s":
        cl = data.classes_dict[domain]
        return np_seg_nearest(raw, list(cl.values()), list(cl))[None, None]
    x = raw.astype(np.float32)
    x = x - x.min()
    return np.moveaxis(x / x.max(), 2, 0)[None]


def ulp_diff(a, b):
    """|a - b| in fp32 ulps of b; 0 where both are the same inf / NaN"""
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
    return np.where(same, 0.0, d)


def same_specials(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


@pytest.mark.parametrize("name", list(cases.single_cases(data.classes_dict)))
def test_decode_formula_reproduces_the_reference(golden, name):
    task, domain, build, o = cases.single_cases(data.classes_dict)[name]
    got, ref = np_decode(task, domain, build(), o), golden[name]
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert same_specials(got, ref)
    if name in cases.LOG_CASES:
        # float32(log(float64(depth))) against the reference's fp32 log: 1 ulp, in a share of the elements far below 1e-3
        d = ulp_diff(got, ref)
        print("%s: %d of %d elements differ, max %.2f ulp" % (name, (d > 0).sum(), d.size, d.max()))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3
    else:
        assert np.array_equal(got, ref, equal_nan=True)


def test_quirk_case_holds_the_quirks(golden):
    inv, lg = golden["unity_quirks_inv"], golden["unity_quirks_log"]
    assert (inv < 0).any() and np.isposinf(inv).any()           # negative codes, code 0
    assert np.isnan(lg).any() and np.isneginf(lg).any()
    assert np.isnan(golden["real_nan"]).all()                   # a NaN in a normalised source: min and max are NaN
    assert golden["mask_01"].max() == 1 and set(np.unique(golden["mask_255"])) == {0.0, 1.0}
    assert golden["kitti_seg"].dtype == np.float64 and golden["kitti_seg"].max() == 10     # label 14 -> class 10


def test_palette_cases_hold_ties():
    for domain in ("s", "r"):
        cols = np.array(list(data.classes_dict[domain].values()), np.int64)
        raw = cases.palette_seg("palette_" + domain, data.classes_dict[domain]).astype(np.int64)
        d = np.sort(((raw[:, :, None, :] - cols[None, None]) ** 2).sum(-1), axis=-1)
        assert (d[..., 0] == d[..., 1]).sum() >= 8 and (d[..., 0] == 0).sum() > 100


@pytest.mark.parametrize("name", list(cases.E2E))
def test_bucketized_depths_keep_clear_of_the_boundaries(golden, name):
    case = cases.E2E[name]
    bounds = cases.boundaries()
    for k, hw in enumerate(case["samples"]):
        raw = cases.e2e_sources(name, k, hw, data.classes_dict)["d"]
        assert cases.ulps_from_boundaries(case["domain"], raw).min() >= 4
        ref = golden["%s.%d.d_loaded" % (name, k)]              # the reference's own log depth, too
        gap = np.abs(ref.astype(np.float64)[..., None] - bounds.astype(np.float64)).min(-1)
        assert (gap / np.spacing(np.abs(ref)).astype(np.float64)).min() >= 4
        assert golden["%s.%d.d" % (name, k)].dtype == np.int32


# ---- RawSource ------------------------------------------------------------------------------------------------------------
def test_raw_source_checks_its_array():
    u8 = torch.zeros(8, 12, 3, dtype=torch.uint8)
    src = RawSource(u8, "unity_d", log=True)
    assert src.shape == (1, 1, 8, 12) and src.task == "d" and src.flags == ops.DTF_DEC_LOG and not src.needs_stats
    assert RawSource(u8, "unity_d", normalize=True).needs_stats
    assert not RawSource(u8, "unity_d", normalize=True, minmax=(0.5, 2.0)).needs_stats
    assert RawSource(u8, "x").shape == (1, 3, 8, 12) and RawSource(u8, "x").needs_stats
    assert RawSource(torch.zeros(8, 12, 4, dtype=torch.uint8), "x").t.shape == (8, 12, 3)
    assert RawSource(u8, "mask").needs_stats and not RawSource(u8, "mask", threshold=True).needs_stats
    assert RawSource(torch.zeros(8, 12), "f32_d").needs_stats
    with pytest.raises(AssertionError):
        RawSource(u8, "unity_d", normalize=True, log=True)
    with pytest.raises(RuntimeError):
        RawSource(u8.float(), "unity_d")
    with pytest.raises(RuntimeError):
        RawSource(u8[:, :, :2], "unity_d")
    with pytest.raises(RuntimeError):
        RawSource(u8, "kitti_d")
    with pytest.raises(ValueError):
        RawSource(u8, "kitti_s")
    with pytest.raises(ValueError):
        RawSource(u8, "depth")
    with pytest.raises(TypeError, match="per-sample transforms take tensors"):
        Resize(8)({"d": src})


def test_palettes():
    pal = data.exact_palette(data.classes_dict["kitti"], data.kitti_mapping, 14)
    assert pal.n == 15 and pal.default_class == 10 and list(pal.cls)[:15] == list(data.kitti_mapping.values())
    assert pal.colour[1] == 90 | 200 << 8 | 255 << 16
    near = data.nearest_palette("r")
    assert near.n == 11 and list(near.cls)[:11] == list(range(11)) and near.colour[8] == 220 | 20 << 8 | 60 << 16 | 255 << 24
    with pytest.raises(RuntimeError):
        ops.data_palette([(0, 0, 0)] * 17, list(range(17)))
    labels = np.array([[0.0, 14.0, 99.0, 6.0]])
    assert data.merge_labels(labels, data.kitti_mapping).tolist() == [[5.0, 10.0, 14.0, 3.0]]


# ---- the C entry points refuse bad tables before anything is launched -------------------------------------------------------
def _item(kind, **kw):
    items = (_lib.DataTfItem * 1)()
    it = items[0]
    it.src = it.dst = 4096                      # never read: every call below is refused on the host
    it.src_h, it.src_w, it.out_h, it.out_w = 8, 12, 8, 12
    it.channels = {ops.DTF_SRC_UNITY_D: 3, ops.DTF_SRC_SEG_EXACT: 3, ops.DTF_SRC_SEG_NEAREST: 4}.get(kind, 1)
    it.stride_h, it.stride_w, it.stride_c = 12 * it.channels, it.channels, 1
    it.far_plane = 1000.0
    for k, v in kw.items():
        setattr(it, k, v)
    return items


def _call(items, kind, mode=ops.DTF_NEAREST, epi=ops.DTF_EPI_NONE, palette=None):
    p = C.cast(items, C.c_void_p)
    pal = C.cast(C.pointer(palette), C.c_void_p) if palette is not None else None
    return _lib.load().cgan_data_transform(p, p, 1, mode, kind, epi, None, None, None, 0, pal, None)


@pytest.mark.parametrize("what, items, kw", [
    ("kind", _item(ops.DTF_SRC_MASK), dict(kind=9)),
    ("bilinear", _item(ops.DTF_SRC_MASK), dict(kind=ops.DTF_SRC_MASK, mode=ops.DTF_BILINEAR)),
    ("unity channels", _item(ops.DTF_SRC_UNITY_D, channels=2), dict(kind=ops.DTF_SRC_UNITY_D)),
    ("kitti channels", _item(ops.DTF_SRC_KITTI_D, channels=3), dict(kind=ops.DTF_SRC_KITTI_D)),
    ("kitti alignment", _item(ops.DTF_SRC_KITTI_D, src=4097), dict(kind=ops.DTF_SRC_KITTI_D)),
    ("zero range", _item(ops.DTF_SRC_F32_D, u8_range=0.0), dict(kind=ops.DTF_SRC_F32_D)),
    ("zero range", _item(ops.DTF_SRC_UNITY_D, dec_flags=ops.DTF_DEC_NORMALIZE), dict(kind=ops.DTF_SRC_UNITY_D)),
    ("log and normalize", _item(ops.DTF_SRC_UNITY_D, dec_flags=3, u8_range=1.0), dict(kind=ops.DTF_SRC_UNITY_D)),
    ("flags", _item(ops.DTF_SRC_MASK, dec_flags=ops.DTF_DEC_LOG), dict(kind=ops.DTF_SRC_MASK)),
    ("far", _item(ops.DTF_SRC_UNITY_D, far_plane=0.0), dict(kind=ops.DTF_SRC_UNITY_D)),
    ("no palette", _item(ops.DTF_SRC_SEG_EXACT), dict(kind=ops.DTF_SRC_SEG_EXACT)),
    ("stray palette", _item(ops.DTF_SRC_MASK), dict(kind=ops.DTF_SRC_MASK, palette=data.nearest_palette("s"))),
    ("alpha", _item(ops.DTF_SRC_SEG_EXACT), dict(kind=ops.DTF_SRC_SEG_EXACT, palette=data.nearest_palette("s"))),
    ("window", _item(ops.DTF_SRC_MASK, out_w=13), dict(kind=ops.DTF_SRC_MASK)),
    ("bucketize", _item(ops.DTF_SRC_MASK), dict(kind=ops.DTF_SRC_MASK, epi=ops.DTF_EPI_BUCKETIZE)),
    ("stats on a tensor", _item(ops.DTF_SRC_B4, stats=4096), dict(kind=ops.DTF_SRC_B4)),
])
def test_item_validation_refuses(what, items, kw):
    assert _call(items, **kw) != 0, what
    assert _lib.load().cgan_last_error()


def test_minmax_validation_refuses():
    lib = _lib.load()
    items = (_lib.DataMinmaxItem * 1)()
    it = items[0]
    it.src, it.out, it.pixels, it.channels, it.far_plane = 4096, 4096, 96, 3, 1000.0
    p = C.cast(items, C.c_void_p)

    def call(kind):
        return lib.cgan_data_source_minmax(p, p, 1, kind, C.c_void_p(4096), None)
    assert call(ops.DTF_SRC_SEG_EXACT) != 0                     # no min / max of a segmentation map
    assert call(ops.DTF_SRC_KITTI_D) != 0                       # three channels
    it.src = 4100
    assert call(ops.DTF_SRC_UNITY_D) != 0                       # 16-byte loads need an aligned source
    it.src, it.pixels = 4096, 0
    assert call(ops.DTF_SRC_UNITY_D) != 0
    it.pixels, it.far_plane = 96, 0.0
    assert call(ops.DTF_SRC_UNITY_D) != 0
