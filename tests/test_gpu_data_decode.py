"""The loaders' decode on the GPU (climategan_amd/data.py, transforms.RawSource, the raw source kinds of csrc/data_tf.hip)
against the real reference's recorded outputs (tests/golden/data_decode.npz, written by
tests/devtools/make_golden_data_decode.py).

Bounds.  Labels, masks, bucket indices, inverse and normalised depth, x: every element equal, NaN and inf at the same places
with the same sign.  Log depth: the kernel rounds the float64 log of the fp32 depth to fp32; numpy's float64 log may differ
from the device's in its last bit across a rounding boundary, so 1 fp32 ulp against the numpy restatement, hence 2 ulp against
the reference's fp32 log (which itself differs from the float64-rounded value by at most 1 ulp in 5e-5 of the elements), and
fewer than 1 element in 1000 may differ from the fixture at all: a wrong formula fails that cap, rounding does not."""
import numpy as np
import pytest
import torch

import data_decode_cases as cases
import data_transform_cases as dc
from climategan_amd.config import Opts
from helpers import GOLDEN
from test_data_decode_host import np_decode, same_specials, ulp_diff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "data_decode.npz")


def single(name):
    from climategan_amd import data
    return cases.single_cases(data.classes_dict)[name]


def raw_of(name):
    from climategan_amd import data
    task, domain, build, o = single(name)
    return data.raw_source(build(), task, domain, Opts(cases.loader_opts(**o)), device=DEV), task


def check(name, got, ref, what):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, got.dtype)
    assert same_specials(got, ref), what
    if name in cases.LOG_CASES:
        d = ulp_diff(got, ref)
        print("%s %s: %d of %d elements differ from the fixture, max %.2f ulp" % (name, what, (d > 0).sum(), d.size, d.max()))
        assert d.max() <= 2 and (d > 0).mean() < 1e-3, what
    else:
        assert np.array_equal(got, ref, equal_nan=True), what


ALL = list(cases.single_cases({"s": {}, "r": {}, "kitti": {}}))


@pytest.mark.parametrize("name", ALL)
def test_tensor_loader_equals_the_reference(name, golden):
    from climategan_amd import data
    task, domain, build, o = single(name)
    got = data.tensor_loader(build(), task, domain, Opts(cases.loader_opts(**o)), device=DEV)
    check(name, got, golden[name], "tensor_loader")
    if name in cases.LOG_CASES:                     # 1 ulp against the formula in numpy's float64
        d = ulp_diff(got.cpu().numpy(), np_decode(task, domain, build(), o))
        assert d.max() <= 1


def small_pipeline():
    """flip, resize, crop, resize: a window that is not the whole image"""
    from climategan_amd import transforms as T
    return [T.RandomHorizontalFlip(), T.Resize(48, keep_aspect_ratio=True), T.RandomCrop(40), T.Resize({"default": 32, "d": 12})]


def draws_for(flip, top, left):
    return [("rand", 0.1 if flip else 0.9), ("randint", top), ("randint", left)]


@pytest.mark.parametrize("name", ALL)
def test_batch_equals_decode_then_the_tensor_path(name, golden):
    """raw sources through the batch transform == tensor_loader's tensor through the existing tensor path, bit for bit, and
    == the reference's decoded map through the tensor path; a window at each corner, flipped and not"""
    from climategan_amd import transforms as T
    raw, task = raw_of(name)
    decoded = raw.to_tensor()
    ref = torch.from_numpy(golden[name]).to(DEV)
    # a 48 x 72 map after the first resize: corners of the 40 x 40 crop are top 0..7 (randint's range), left 0..31
    for flip, top, left in [(False, 0, 0), (True, 0, 0), (False, 7, 31), (True, 7, 31), (True, 0, 31), (False, 7, 0)]:
        outs = []
        for src in (raw, decoded, ref):
            bt = T.BatchTransform(small_pipeline(), draws=T.RecordedPipelineDraws(draws_for(flip, top, left) * 2))
            outs.append(bt([{task: src}, {task: src}])[task])
        assert outs[0].dtype == outs[1].dtype
        assert np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy(), equal_nan=True)
        if task == "x":         # the tensor path resamples the reference's fp32 x; the raw path the same values
            assert torch.equal(outs[0], outs[2])
        else:
            check(name, outs[0], outs[2].cpu().numpy(), "batch flip=%s top=%d left=%d" % (flip, top, left))


def test_mixed_sizes_in_one_batch(golden):
    from climategan_amd import data, transforms as T
    shapes = [(64, 96), (50, 70), (33, 47)]
    for kind, build, kw in [("unity_d", cases.unity, dict(normalize=True)), ("kitti_d", cases.kitti_depth, dict(log=True)),
                            ("mask", lambda n, h, w: cases.mask(n, 255, h=h, w=w), {}),
                            ("x", cases.x_image, {})]:
        srcs = [T.RawSource.from_numpy(build("mixed.%s.%d" % (kind, k), h, w), kind, DEV, **kw) for k, (h, w) in enumerate(shapes)]
        task = srcs[0].task
        pipeline = [T.RandomHorizontalFlip(), T.Resize({"default": 24})]
        rec = [("rand", 0.1), ("rand", 0.9), ("rand", 0.1)]
        got = T.BatchTransform(pipeline, draws=T.RecordedPipelineDraws(rec))([{task: s} for s in srcs])[task]
        want = T.BatchTransform(pipeline, draws=T.RecordedPipelineDraws(rec))([{task: s.to_tensor()} for s in srcs])[task]
        assert got.shape[0] == 3 and torch.equal(got, want), kind


def test_known_constants_equal_the_device_ones():
    """a RawSource that is told its min / max, or its threshold flag, gives the bits of the one that finds them"""
    from climategan_amd import transforms as T
    raw = cases.unity("known")
    found = T.RawSource.from_numpy(raw, "unity_d", DEV, normalize=True).to_tensor()
    inv = T.RawSource.from_numpy(raw, "unity_d", DEV).to_tensor()
    told = T.RawSource.from_numpy(raw, "unity_d", DEV, normalize=True, minmax=(inv.min().item(), inv.max().item())).to_tensor()
    assert torch.equal(found, told)
    m = cases.mask("known.m", 255)
    assert torch.equal(T.RawSource.from_numpy(m, "mask", DEV).to_tensor(), T.RawSource.from_numpy(m, "mask", DEV, threshold=True).to_tensor())
    x = cases.x_image("known.x")
    assert torch.equal(T.RawSource.from_numpy(x, "x", DEV).to_tensor(),
                       T.RawSource.from_numpy(x, "x", DEV, minmax=(x.min(), x.max())).to_tensor())


def test_minmax_is_the_same_every_run_and_equals_torch():
    from climategan_amd import ops
    # sizes that leave a tail behind the last 16-byte group, and one large enough for every partial
    for h, w in [(1, 5), (7, 9), (64, 96), (1200, 1800)]:
        srcs = {ops.DTF_SRC_UNITY_D: cases.unity("mm.u", h, w), ops.DTF_SRC_KITTI_D: cases.kitti_depth("mm.k", h, max(w, 4)),
                ops.DTF_SRC_U8: cases.x_image("mm.x", h, w),
                ops.DTF_SRC_F32_D: np.ascontiguousarray(cases._u("mm.f%d" % h, (h, w)).astype(np.float32))}
        for kind, arr in srcs.items():
            t = torch.from_numpy(arr).to(DEV)
            far = [1000.0, 1000.0]
            a = ops.data_source_minmax([t, t], kind, far=far)
            b = ops.data_source_minmax([t, t], kind, far=far)
            assert torch.equal(a, b) and torch.equal(a[0], a[1])
            if kind == ops.DTF_SRC_UNITY_D:
                v = np_decode("d", "s", arr, dict(log=False, normalize=False))
            elif kind == ops.DTF_SRC_KITTI_D:
                v = np_decode("d", "kitti", arr, dict(log=False, normalize=False))
            else:
                v = arr.astype(np.float32)
            want = [v.min(), np.float32(v.max() - v.min()), v.max(), np.float32(v.max() > 127)]
            assert a[0].cpu().numpy().tolist() == [float(x) for x in want], (kind, h, w)
    nan = np.ones((40, 40), np.float32)
    nan[17, 3] = np.nan
    out = ops.data_source_minmax([torch.from_numpy(nan).to(DEV)], ops.DTF_SRC_F32_D)
    assert torch.isnan(out[0, :3]).all()


def recorded(golden, name):
    return list(zip([str(k) for k in golden[name + ".draw_kinds"]], [float(v) for v in golden[name + ".draw_values"]]))


@pytest.mark.parametrize("name", list(cases.E2E))
def test_end_to_end_equals_the_reference(name, golden):
    """raw sources of all four tasks through the default train pipeline, bucketized log depth included"""
    from climategan_amd import data, transforms as T
    case = cases.E2E[name]
    opts = Opts(cases.e2e_opts(case))
    samples = []
    for k, hw in enumerate(case["samples"]):
        src = cases.e2e_sources(name, k, hw, data.classes_dict)
        samples.append({task: data.raw_source(src[task], task, case["domain"], opts, device=DEV) for task in cases.E2E_TASKS})
    bt = T.compile_transforms(opts, case["mode"], case["domain"], draws=T.RecordedPipelineDraws(recorded(golden, name)))
    out = bt(samples)
    for k in range(len(samples)):
        for task in cases.E2E_TASKS:
            got, ref = out[task][k].cpu().numpy(), golden["%s.%d.%s" % (name, k, task)]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (task, got.dtype, ref.dtype)
            if task == "x":
                assert np.abs(got - ref).max() <= 2e-6 / 0.5        # the bound of test_gpu_data_transforms.py
            else:
                assert np.array_equal(got, ref), (k, task)
    assert out["d"].dtype == torch.int32


def test_helpers_of_tutils_and_data(golden):
    from climategan_amd import data, tutils
    raw = cases.unity("unity_norm")
    got = tutils.decode_unity_depth_t(torch.from_numpy(raw.astype(np.float32)).to(DEV), log=False, normalize=True)
    assert np.array_equal(got.cpu().numpy(), golden["unity_norm"][0])
    k = cases.kitti_depth("kitti_inv")
    got = tutils.get_normalized_depth_t(torch.from_numpy(k.astype(np.float32)).to(DEV), "kitti", normalize=False, log=False)
    assert np.array_equal(got.cpu().numpy(), golden["kitti_inv"][0])
    seg = cases.kitti_seg("kitti_seg", data.classes_dict["kitti"])
    labels = data.encode_exact_segmap(seg, data.classes_dict["kitti"])
    assert labels.dtype == np.float64
    assert np.array_equal(data.merge_labels(labels, data.kitti_mapping)[None, None], golden["kitti_seg"])
    ids = data.encode_segmap(cases.palette_seg("palette_s", data.classes_dict["s"]), "s")
    assert ids.dtype == np.float64 and np.array_equal(ids[None].astype(np.float32), golden["palette_s"])
