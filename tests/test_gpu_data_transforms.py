"""The loaders' transforms on the GPU (climategan_amd/transforms.py, csrc/data_tf.hip) against the real reference's recorded
outputs (tests/golden/data_transforms.npz, written by tests/devtools/make_golden_data_transforms.py): every case through the
per-sample classes and through the batch transform, replaying the recorded draws.

Bounds.  d, m, s and the bucketized depth: every element equal, nothing excluded.  x: max |err| <= 2e-6 / min(std) (4e-6 with
the default constants, 9e-6 with HRNet's): the weights are the reference's bit for bit, what may differ is the order and
the contraction of the 16-tap sum, about a dozen fp32 roundings (2^-24 each) of quantities <= 1, before the division by std.
The case ``int64_s`` compares with the reference's run on the fp32 tensor of the same class ids (the installed torch has no
int64 nearest kernel on the CPU; see the fixture script).  The colour jitter is pinned to torchvision's documented formulas,
restated below in torch fp32, not to a run of the reference."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import data_transform_cases as dc
from climategan_amd import fill
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "data_transforms.npz")


def recorded(golden, name):
    return list(zip([str(k) for k in golden[name + ".draw_kinds"]], [float(v) for v in golden[name + ".draw_values"]]))


def device_samples(name, case):
    return [{task: torch.from_numpy(v).to(DEV) for task, v in
             dc.sample_inputs(name, k, shapes, case.get("s_int64", False)).items()}
            for k, shapes in enumerate(case["samples"])]


def transforms_of(case, draws, tasks=("d", "s", "m", "p")):
    from climategan_amd import transforms as T
    return T.get_transforms(dc.mirror_opts(case, tasks), case["mode"], case.get("domain", "r"), draws=draws)


def x_bound(case):
    std = (0.229, 0.224, 0.225) if case.get("normalization") == "HRNet" else (0.5, 0.5, 0.5)
    return 2e-6 / min(std)


# The plain gather on its own: a multi-channel source read in place through a non-contiguous view, 4-byte (fp32) and 8-byte
# (float64) elements, 0, 1 and 2 stages, flipped in every map or in none, a crop offset in every map; against CPU torch
# applying torch.flip, slicing and F.interpolate(mode="nearest") in the same order.  33 x 47 = 1551 output pixels: one full
# block of 1024 and one whose threads own 1 to 3 live pixels of their 4; 1 x 1: a single live pixel.
PLAIN_GATHER = {"plain_gather_f32x3": (torch.float32, 3), "plain_gather_f64x2": (torch.float64, 2)}


def plain_gather_equals_torch(name):
    from climategan_amd import ops, transforms as T

    dtype, c = PLAIN_GATHER[name]
    if dtype == torch.float32:      # CHW inside a larger CHW tensor; every element distinct and exact
        big, view = torch.arange(c * 56 * 80, dtype=dtype).reshape(c, 56, 80), lambda t: t[:, 3:53, 5:75]
    else:                           # an HWC tensor seen as CHW: channel stride 1, column stride C
        big, view = torch.arange(60 * 80 * c, dtype=dtype).reshape(60, 80, c), lambda t: t.permute(2, 0, 1)[:, 3:53, 5:75]
    cpu, dev = view(big), view(big.to(DEV))
    assert tuple(dev.shape) == (c, 50, 70) and not dev.is_contiguous()
    for oh, ow in [(33, 47), (1, 1)]:
        crops = [(2, 3, oh + 11, ow + 13), (1, 2, oh + 4, ow + 2), (2, 1, oh, ow)]
        sizes = [(oh + 7, ow + 5), (oh + 3, ow + 3)]
        for ns in (0, 1, 2):
            for flip in (False, True):
                plan, want = T.Plan(50, 70), cpu.unsqueeze(0)
                for k, (top, left, h, w) in enumerate(crops[:ns] + crops[-1:]):
                    if flip:
                        plan.flip()
                        want = torch.flip(want, [3])
                    plan.crop(top, left, h, w)
                    want = want[:, :, top:top + h, left:left + w]
                    if k < ns:
                        plan.resize(*sizes[2 - ns + k])
                        want = F.interpolate(want, size=sizes[2 - ns + k], mode="nearest")
                (launch,) = plan.launches()
                assert len(launch[0]) == ns and all(m[0] and m[1] and m[2] == flip for m in launch[1])
                got = ops.data_transform([dev], [launch], ops.DTF_NEAREST)
                assert got.dtype == dtype and torch.equal(got.cpu(), want), (name, oh, ow, ns, flip)


@pytest.mark.parametrize("name", list(dc.CASES) + list(PLAIN_GATHER))
def test_case_equals_the_reference(name, golden):
    from climategan_amd import transforms as T

    if name in PLAIN_GATHER:
        return plain_gather_equals_torch(name)
    case = dc.CASES[name]
    samples = device_samples(name, case)
    draws = T.RecordedPipelineDraws(recorded(golden, name))
    single = T.Compose(transforms_of(case, draws))
    per_sample = [single(s) for s in samples]
    assert draws.used == len(draws.draws)
    draws = T.RecordedPipelineDraws(recorded(golden, name))
    batch = T.BatchTransform(transforms_of(case, draws))(samples)
    assert draws.used == len(draws.draws)
    torch.cuda.synchronize()
    for task in case["samples"][0]:
        assert batch[task].shape[0] == len(samples)
        for k in range(len(samples)):
            want = golden["%s.%d.%s" % (name, k, task)]
            one = per_sample[k][task]
            assert one.dim() == 3                                          # Normalize dropped the batch dimension (:235)
            assert torch.equal(batch[task][k], one), (name, k, task)       # the batch path = the per-sample path, bit for bit
            got = dc.subsample(one.cpu().numpy(), case.get("sub"))
            assert got.dtype == want.dtype and got.shape == want.shape, (name, k, task, got.dtype, got.shape, want.shape)
            if task == "x":
                err = float(np.abs(got - want).max())
                print("%s sample %d x: max |err| = %.3g (bound %.3g)" % (name, k, err, x_bound(case)))
                assert err <= x_bound(case), (name, k, err)
            else:
                assert np.array_equal(got, want), (name, k, task, int((got != want).sum()))


def u8_image(h, w, seed):
    return np.floor(fill.uniform01((h, w, 3), seed) * 200 + 13).astype(np.uint8)          # min > 0, max < 255


def tensor_loader_x(arr_u8):
    """reference data.py:377-399 for task x"""
    arr = arr_u8.astype(np.float32)
    arr -= arr.min()
    arr /= arr.max()
    return torch.from_numpy(np.moveaxis(arr, 2, 0).copy()).unsqueeze(0)


def test_uint8_sources_equal_the_fp32_path_bit_for_bit():
    from climategan_amd import transforms as T

    case = dc.CASES["default_train"]
    imgs = [u8_image(90, 130, 1), u8_image(130, 90, 2), u8_image(77, 77, 3)]
    u8 = [{"x": T.RawSource.from_numpy(a, "x", DEV, minmax=(a.min(), a.max()))} for a in imgs]
    f32 = [{"x": tensor_loader_x(a).to(DEV)} for a in imgs]
    for a, b in zip(u8, f32):
        assert torch.equal(a["x"].to_tensor(), b["x"])
    outs = []
    for samples in (u8, f32):
        dc.seed_all(5)
        outs.append(T.compile_transforms(dc.mirror_opts(case), "train", "r")(samples)["x"])
    assert outs[0].shape == (3, 3, 64, 64) and torch.equal(outs[0], outs[1])
    one = T.Resize(64, keep_aspect_ratio=True)({"x": f32[0]["x"]})["x"]
    assert one.shape == (1, 3, 64, 92)


# ---- colour jitter: torchvision's documented formulas in torch fp32 (CPU) ------------------------------------------------
def blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0, 1)


def gray(x):
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


def jitter_ref(x, name, f):
    if name == "RandBrightness":
        y = blend(x, torch.zeros_like(x), f)
    elif name == "RandSaturation":
        y = blend(x, gray(x), f)
    else:
        y = blend(x, gray(x).mean(dim=(-3, -2, -1), keepdim=True), f)
    y[:, :, 0, 0] = 1.0                # the reference's dummy pixels, transforms.py:504-506
    y[:, :, -1, -1] = 0.0
    return y


# Both sides form every per-pixel expression with the same fp32 operations in the same order (no contraction in the kernel,
# none between torch's element-wise ops), so brightness and saturation are held to torch.equal, normalised or not.  The
# contrast mean is the one quantity whose summation order differs.  For h * w <= 4096 * 256 (every shape here; beyond
# that a thread's chain grows with h * w / 65536) the kernel adds at most 16 values per thread, then two 8-level trees: 32
# roundings on a chain, and torch's pairwise mean no more; each mean is within 32 * 2^-24 of the exact one (values <= 1),
# the two within 64 * 2^-24 of each other.  The blend scales that by |1 - f| <= 0.5 and adds, per side, the rounding of
# (1 - f) * mean (<= 0.5: 2^-25) and of the sum (< 2: 2^-24): 32 * 2^-24 + 2 * (2^-25 + 2^-24) = 35 * 2^-24 = 2.1e-6
# before Normalize.  Normalize divides that by std and adds, per side, the rounding of the difference (<= 1: 2^-25) and of
# the quotient (< 4: 2^-23): 2^-24 + 2^-22.  Both sides start from the same input, so there is no term for the gather.
def contrast_bound(min_std=None):
    b = 35 * 2.0 ** -24
    return b if min_std is None else b / min_std + 2.0 ** -24 + 2.0 ** -22


@pytest.mark.parametrize("shape", [(3, 3, 60, 64), (1, 3, 33, 70), (2, 3, 1, 1), (1, 3, 300, 333)])
def test_jitter_ops_equal_the_formulas(shape):
    from climategan_amd import ops, transforms as T

    n = shape[0]
    assert shape[2] * shape[3] <= 4096 * 256
    x = torch.from_numpy(fill.uniform01(shape, 11).astype(np.float32))
    rnd = random.Random(4)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for cls in (T.RandBrightness, T.RandSaturation, T.RandContrast):
        fs = [rnd.uniform(0.5, 1.5) for _ in range(n)]
        want = torch.cat([jitter_ref(x[k:k + 1].clone(), cls.__name__, fs[k]) for k in range(n)])
        wantn = (want - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
        got = ops.data_jitter(x.to(DEV), cls.op, T._jitter_factors(fs, DEV)).cpu()
        gotn = ops.data_jitter(x.to(DEV), cls.op, T._jitter_factors(fs, DEV), normalize=(mean, std)).cpu()
        err, errn = float((got - want).abs().max()), float((gotn - wantn).abs().max())
        print("%s %s: max |err| = %.3g, normalised %.3g" % (cls.__name__, shape, err, errn))
        if cls is T.RandContrast:
            assert err <= contrast_bound() and errn <= contrast_bound(min(std))
        else:
            assert torch.equal(got, want) and torch.equal(gotn, wantn)
        assert torch.equal(got[:, :, -1, -1], torch.zeros(n, 3))                    # the dummy pixels, exact
        if shape[2] * shape[3] > 1:
            assert torch.equal(got[:, :, 0, 0], torch.ones(n, 3))
        # one image through the class = its row of the batch
        cls_obj = cls()
        cls_obj.draws = T.RecordedPipelineDraws([("uniform", fs[0])])
        assert torch.equal(cls_obj({"x": x[:1].to(DEV), "m": x[:1, :1]})["x"].cpu(), got[:1])


def test_pipeline_with_jitter():
    """train mode without the Painter task: gather -> brightness -> saturation -> contrast -> Normalize, per sample and as
    a batch (bit-equal), against the formulas applied to the un-jittered gather of the same draws"""
    from climategan_amd import transforms as T

    case = dc.CASES["mixed_batch"]
    samples = device_samples("mixed_batch", case)
    dc.seed_all(21)
    log = []

    class Logged(T.PipelineDraws):
        def rand(self):
            log.append(("rand", super().rand()))
            return log[-1][1]

        def randint(self, low, high):
            log.append(("randint", super().randint(low, high)))
            return log[-1][1]

        def uniform(self, a, b):
            log.append(("uniform", super().uniform(a, b)))
            return log[-1][1]

    batch = T.BatchTransform(transforms_of(case, Logged(), tasks=("d", "s", "m")))(samples)
    assert [k for k, _ in log] == ["rand", "randint", "randint", "uniform", "uniform", "uniform"] * len(samples)
    single = T.Compose(transforms_of(case, T.RecordedPipelineDraws(log), tasks=("d", "s", "m")))
    for k, s in enumerate(samples):
        one = single(s)
        for task in one:
            assert torch.equal(one[task], batch[task][k]), (k, task)
    # the same geometry without jitter and Normalize, then the formulas
    plain = [t for t in transforms_of(case, T.RecordedPipelineDraws([d for d in log if d[0] != "uniform"]))
             if isinstance(t, (T.Resize, T.RandomCrop, T.RandomHorizontalFlip))]
    x0 = T.BatchTransform(plain)(samples)["x"].cpu()
    assert float(x0.min()) >= 0.0 and float(x0.max()) <= 1.0
    fs = [v for k, v in log if k == "uniform"]
    for k in range(len(samples)):
        y = x0[k:k + 1].clone()
        for j, name in enumerate(("RandBrightness", "RandSaturation", "RandContrast")):
            y = jitter_ref(y, name, fs[3 * k + j])
        y = (y - 0.5) / 0.5
        err = float((batch["x"][k].cpu() - y[0]).abs().max())
        print("jitter pipeline sample %d: max |err| = %.3g (bound %.3g)" % (k, err, contrast_bound(0.5)))
        assert err <= contrast_bound(0.5)            # brightness and saturation are bit-equal: contrast's bound alone
        assert torch.equal(batch["x"][k, :, 0, 0].cpu(), torch.ones(3)) and torch.equal(batch["x"][k, :, -1, -1].cpu(),
                                                                                       -torch.ones(3))


def test_u8_images_are_refused_where_they_cannot_go():
    from climategan_amd import transforms as T

    arr = u8_image(20, 30, 1)
    img = T.RawSource.from_numpy(arr, "x", DEV, minmax=(arr.min(), arr.max()))
    x = img.to_tensor()
    for t in (T.Resize(8), T.RandomCrop(4, center=True), T.RandomHorizontalFlip(1.0), T.Normalize(dc.mirror_opts({"items": []})),
              T.RandBrightness()):
        with pytest.raises(TypeError, match="to_tensor"):
            t({"x": img})
    with pytest.raises(TypeError, match="1 of 2 samples"):
        T.BatchTransform([T.Resize(8)])([{"x": img}, {"x": x}])


def test_bad_plans_are_refused_before_the_launch():
    from climategan_amd import ops

    x = torch.zeros(1, 1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="leaves its"):
        ops.data_transform([x], [([], [(0, 0, False)], (9, 8))], ops.DTF_NEAREST)
    with pytest.raises(RuntimeError, match="leaves its"):
        ops.data_transform([x], [([(8, 8, 4, 4)], [(1, 0, False), (0, 0, False)], (4, 4))], ops.DTF_NEAREST)
    with pytest.raises(RuntimeError, match="leaves its"):
        ops.data_transform([x], [([], [(0, 6, True)], (8, 8))], ops.DTF_NEAREST)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.data_transform([x.cpu()], [([], [(0, 0, False)], (8, 8))], ops.DTF_NEAREST)
    with pytest.raises(RuntimeError, match="float32"):
        ops.data_transform([x.long()], [([], [(0, 0, False)], (8, 8))], ops.DTF_BILINEAR)
    with pytest.raises(RuntimeError, match="32-bit fields"):           # ctypes would wrap it to 8 and the C side accept it
        ops.data_transform([x], [([], [(0, 0, False)], (8 + 2 ** 32, 8))], ops.DTF_NEAREST)
    with pytest.raises(RuntimeError, match="32-bit fields"):
        ops.data_transform([x], [([(8, 8, 4, 4 - 2 ** 32)], [(0, 0, False), (0, 0, False)], (4, 4))], ops.DTF_NEAREST)
