"""Mirror of the reference's ``climategan/transforms.py``.

**The loaders' transforms** (``transforms.py:22-289, 424-490``): ``Resize``, ``RandomCrop``, ``RandomHorizontalFlip``,
``Normalize``, ``BucketizeDepth``, ``RandBrightness / RandSaturation / RandContrast``, ``interpolation``, ``get_transform``
and ``get_transforms`` with the reference's names, constructor arguments and attributes.  Each class is callable on a dict
of ``[1, C, H, W]`` DEVICE tensors like the reference's (one sample, at most one HIP launch per task and call; a crop is a
view, as in the reference).  ``compile_transforms(opts, mode, domain)`` is the form a training loop wants: given the N
sample dicts of a batch (sizes may differ between samples and between the tasks of one sample) it makes the reference's
random draws in the reference's order, reduces each task's flips, crops and resizes to one *plan* on the host (``Plan``:
up to two resampling stages with an integer index map before, between and after them) and runs ONE launch per task for the
whole batch (``ops.data_transform``, csrc/data_tf.hip), which reads only the source pixels the final crop needs and
writes the collated ``[N, C, h, w]`` batch ``Trainer.train_step`` takes.  The index arithmetic is ATen's own fp32
formulas, so ``d``, ``m``, ``s`` equal the reference bit for bit and ``x`` to a few fp32 roundings.  A sample's entries may
also be ``RawSource``s -- the arrays as the image decoder left them (Unity / kitti / fp32 depth, uint8 mask, RGB or RGBA
segmentation image, uint8 ``x``): the same launch then decodes the pixels it gathers (``tensor_loader``'s work,
``climategan_amd.data``), and only a min / max that nobody knows costs two launches more.

The colour jitter of the pipeline (the ``is_diff_augment=False`` branches of ``rand_brightness / rand_saturation /
rand_contrast``, ``transforms.py:501-541``) calls torchvision's ``adjust_*``.  No run of the reference backs this part:
the ``Rand*`` classes are PINNED TO TORCHVISION'S DOCUMENTED FORMULAS (``gray = 0.2989 r + 0.587 g + 0.114 b``,
``blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)``; brightness ``blend(x, 0, f)``, saturation ``blend(x, gray, f)``,
contrast ``blend(x, mean(gray), f)``), not to a run of the reference.  The module-level ``rand_*`` functions below stay
the DiffAugment forms only.

**DiffAugment** (``transforms.py:494-626``): the ``rand_*`` functions with the reference's signatures and
``DiffTransforms``, the transform ``Trainer`` applies to the Painter discriminator's inputs when ``gen.p.diff_aug.use`` is
on (trainer.py:772-773, 1079-1081, 1319-1321).  The random draws are the reference's own torch calls, with the same shapes,
dtypes, devices and order (``TorchDraws``), so that the same generator state gives the same draws; the arithmetic is one
HIP kernel pair per batch (``ops.diffaug`` / ``autograd.DiffAugFn``: forward and backward, all ops of the transform fused).
The source of the draws is replaceable (``RecordedDraws`` replays recorded values) so that tests can compare against the
reference's recorded runs.

Device tensors only, as everywhere in this package: there is no CPU path.
"""
import random
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops


class TorchDraws:
    """The reference's calls: ``torch.rand(N, 1, 1, 1, dtype, device)`` (transforms.py:499, 516, 532) and
    ``torch.randint(low, high, size=[N, 1, 1], device)`` (:558-569, :587-592), on the default generator."""

    def rand(self, n, dtype, device):
        return torch.rand(n, 1, 1, 1, dtype=dtype, device=device)

    def randint(self, low, high, n, device):
        return torch.randint(low, high, size=[n, 1, 1], device=device)


class RecordedDraws:
    """Replays a list of recorded draws (the results of the calls ``TorchDraws`` makes, in call order)."""

    def __init__(self, values):
        self.values = [torch.as_tensor(v) for v in values]
        self.used = 0

    def _next(self, shape):
        if self.used >= len(self.values):
            raise RuntimeError("RecordedDraws: all %d recorded draws are used" % len(self.values))
        v = self.values[self.used]
        if tuple(v.shape) != tuple(shape):
            raise RuntimeError("RecordedDraws: draw %d has shape %s, the call asks for %s"
                               % (self.used, tuple(v.shape), tuple(shape)))
        self.used += 1
        return v

    def rand(self, n, dtype, device):
        return self._next((n, 1, 1, 1)).to(device=device, dtype=dtype)

    def randint(self, low, high, n, device):
        v = self._next((n, 1, 1)).to(device=device, dtype=torch.int64)
        return v


class DiffAugParams(NamedTuple):
    """One batch's augmentation: color [N, 3] fp32 = the raw (brightness, contrast, saturation) draws, geo [N, 4] int64 =
    (tx, ty, ox, oy), flags = ops.DA_* bits, cut_hw = the cutout box size."""
    color: torch.Tensor
    geo: torch.Tensor
    flags: int
    cut_hw: Tuple[int, int]


def draw_params(n, h, w, device, dtype=torch.float32, color=(False, False, False), translation_ratio=None,
                cutout_ratio=None, draws=None) -> Optional[DiffAugParams]:
    """The draws of one DiffTransforms call on an [n, c, h, w] batch, in the reference's order: brightness, contrast,
    saturation, translation (tx then ty), cutout (ox then oy); an op that is off draws nothing.  None when every op is off."""
    draws = draws if draws is not None else TorchDraws()
    flags = 0
    col = [torch.zeros(n, 1, dtype=torch.float32, device=device) for _ in range(3)]
    geo = [torch.zeros(n, 1, dtype=torch.int64, device=device) for _ in range(4)]
    for k, (on, bit) in enumerate(zip(color, (ops.DA_BRIGHTNESS, ops.DA_CONTRAST, ops.DA_SATURATION))):
        if on:
            col[k] = draws.rand(n, dtype, device).reshape(n, 1).float()
            flags |= bit
    if translation_ratio is not None:                                               # transforms.py:583-592
        sx, sy = int(h * translation_ratio + 0.5), int(w * translation_ratio + 0.5)
        geo[0] = draws.randint(-sx, sx + 1, n, device).reshape(n, 1)
        geo[1] = draws.randint(-sy, sy + 1, n, device).reshape(n, 1)
        flags |= ops.DA_TRANSLATION
    cut_hw = (0, 0)
    if cutout_ratio is not None:                                                    # transforms.py:548-569
        cut_hw = (int(h * cutout_ratio + 0.5), int(w * cutout_ratio + 0.5))
        geo[2] = draws.randint(0, h + (1 - cut_hw[0] % 2), n, device).reshape(n, 1)
        geo[3] = draws.randint(0, w + (1 - cut_hw[1] % 2), n, device).reshape(n, 1)
        flags |= ops.DA_CUTOUT
    if not flags:
        return None
    return DiffAugParams(torch.cat(col, dim=1).contiguous(), torch.cat(geo, dim=1).to(torch.int64).contiguous(), flags,
                         cut_hw)


def apply_params(tensor, params: Optional[DiffAugParams]):
    """The augmentation with given draws on an NCHW fp32 device tensor (autograd-aware: the gradient reaches ``tensor``)."""
    if params is None:
        return tensor
    from .autograd import DiffAugFn
    return DiffAugFn.apply(tensor, params.color, params.geo, params.flags, params.cut_hw)


def _check4(tensor, what):
    assert len(tensor.shape) == 4, "For %s, tensor must be 4D." % what


def _no_pipeline(name):
    raise NotImplementedError("%s(is_diff_augment=False) is the data pipeline's torchvision adjust_* branch "
                              "(reference transforms.py:494-541): use the RandBrightness / RandSaturation / RandContrast "
                              "classes of this module" % name)


def rand_brightness(tensor, is_diff_augment=False, draws=None):
    """reference transforms.py:494-507: ``tensor + (rand - 0.5)`` per image"""
    if not is_diff_augment:
        _no_pipeline("rand_brightness")
    _check4(tensor, "rand brightness")
    n, _, h, w = tensor.shape
    return apply_params(tensor, draw_params(n, h, w, tensor.device, tensor.dtype, (True, False, False), draws=draws))


def rand_saturation(tensor, is_diff_augment=False, draws=None):
    """reference transforms.py:510-524: ``(t - mean_c) * (2 rand) + mean_c``"""
    if not is_diff_augment:
        _no_pipeline("rand_saturation")
    _check4(tensor, "rand saturation")
    n, _, h, w = tensor.shape
    return apply_params(tensor, draw_params(n, h, w, tensor.device, tensor.dtype, (False, False, True), draws=draws))


def rand_contrast(tensor, is_diff_augment=False, draws=None):
    """reference transforms.py:527-541: ``(t - mean_chw) * (rand + 0.5) + mean_chw``"""
    if not is_diff_augment:
        _no_pipeline("rand_contrast")
    _check4(tensor, "rand contrast")
    n, _, h, w = tensor.shape
    return apply_params(tensor, draw_params(n, h, w, tensor.device, tensor.dtype, (False, True, False), draws=draws))


def rand_cutout(tensor, ratio=0.5, draws=None):
    """reference transforms.py:544-577: a box of int(h ratio + 0.5) x int(w ratio + 0.5) set to 0, clipped to the image"""
    _check4(tensor, "rand cutout")
    n, _, h, w = tensor.shape
    return apply_params(tensor, draw_params(n, h, w, tensor.device, cutout_ratio=ratio, draws=draws))


def rand_translation(tensor, ratio=0.125, draws=None):
    """reference transforms.py:580-606: a shift of up to int(h ratio + 0.5) / int(w ratio + 0.5) pixels, zero fill"""
    _check4(tensor, "rand translation")
    n, _, h, w = tensor.shape
    return apply_params(tensor, draw_params(n, h, w, tensor.device, translation_ratio=ratio, draws=draws))


class DiffTransforms:
    """reference transforms.py:609-626.  ``draws``: where the random values come from (default: the reference's torch
    calls).  ``draw`` gives one call's parameters without applying them (the Trainer's fused Painter heads apply them
    inside their own kernel); ``__call__`` draws and applies, like the reference."""

    def __init__(self, diff_aug_opts, draws=None):
        self.do_color_jittering = diff_aug_opts.do_color_jittering
        self.do_cutout = diff_aug_opts.do_cutout
        self.do_translation = diff_aug_opts.do_translation
        self.cutout_ratio = diff_aug_opts.cutout_ratio
        self.translation_ratio = diff_aug_opts.translation_ratio
        self.draws = draws if draws is not None else TorchDraws()

    @property
    def active(self):
        """False when every ``do_*`` is off: the transform is the identity (no draw, no launch)."""
        return bool(self.do_color_jittering or self.do_cutout or self.do_translation)

    def draw(self, n, h, w, device, dtype=torch.float32) -> Optional[DiffAugParams]:
        return draw_params(n, h, w, device, dtype, (self.do_color_jittering,) * 3,
                           self.translation_ratio if self.do_translation else None,
                           self.cutout_ratio if self.do_cutout else None, self.draws)

    def __call__(self, tensor):
        if not self.active:
            return tensor
        _check4(tensor, "DiffTransforms")
        n, _, h, w = tensor.shape
        return apply_params(tensor, self.draw(n, h, w, tensor.device, tensor.dtype))


# ----------------------------------------------------------------------------------------------------------------------
# The loaders' transforms (reference transforms.py:22-289, 424-490)
# ----------------------------------------------------------------------------------------------------------------------
def interpolation(task):
    """reference transforms.py:22-26"""
    if task in ["d", "m", "s"]:
        return {"mode": "nearest"}
    return {"mode": "bilinear", "align_corners": True}


def _mode(task):
    return ops.DTF_NEAREST if interpolation(task)["mode"] == "nearest" else ops.DTF_BILINEAR


class PipelineDraws:
    """The reference's calls, in the reference's order per sample: ``np.random.rand()`` for the flip (transforms.py:187),
    ``np.random.randint(0, H - h)`` for ``top`` then ``left`` (:169-170), ``random.uniform(0.5, 1.5)`` per jitter item
    (:502, :519, :536), on numpy's and Python's global generators."""

    def rand(self):
        return np.random.rand()

    def randint(self, low, high):
        return np.random.randint(low, high)

    def uniform(self, a, b):
        return random.uniform(a, b)


class RecordedPipelineDraws:
    """Replays recorded ``(kind, value)`` draws, kind one of "rand", "randint", "uniform", in call order."""

    def __init__(self, draws):
        self.draws = [(str(k), v) for k, v in draws]
        self.used = 0

    def _next(self, kind):
        if self.used >= len(self.draws):
            raise RuntimeError("RecordedPipelineDraws: all %d recorded draws are used" % len(self.draws))
        k, v = self.draws[self.used]
        if k != kind:
            raise RuntimeError("RecordedPipelineDraws: draw %d is a %s, the call asks for a %s" % (self.used, k, kind))
        self.used += 1
        return v

    def rand(self):
        return float(self._next("rand"))

    def randint(self, low, high):
        if high <= low:                     # what np.random.randint raises for an empty range (transforms.py:169-170)
            raise ValueError("low >= high")
        return int(self._next("randint"))

    def uniform(self, a, b):
        return float(self._next("uniform"))


class Plan:
    """What a sequence of hflip / crop / resize items does to one map of ``h`` x ``w`` pixels, reduced to the form the
    kernel takes: resampling stages ``(in_h, in_w, out_h, out_w)`` and, before, between and after them, an integer index
    map ``[row_off, col_off, step]``: window pixel (i, j) is pixel (row_off + i, col_off + step * j) of the image below
    (step -1 = flipped).  Flips and crops compose into the last map; a resize closes it and opens a new one."""

    def __init__(self, h, w):
        self.h, self.w = int(h), int(w)
        self.stages = []
        self.maps = [[0, 0, 1]]

    def flip(self):
        m = self.maps[-1]
        m[1] += m[2] * (self.w - 1)
        m[2] = -m[2]

    def crop(self, top, left, h, w):
        """``tensor[:, :, top : top + h, left : left + w]`` with Python's slice rules (a window that leaves the map is
        clipped, a negative ``top`` counts from the end), as the reference's slicing behaves (transforms.py:175-178)"""
        r0, r1, _ = slice(top, top + h).indices(self.h)
        c0, c1, _ = slice(left, left + w).indices(self.w)
        if r1 <= r0 or c1 <= c0:
            raise ValueError("crop [%d:%d, %d:%d] of a %d x %d map is empty" % (top, top + h, left, left + w, self.h, self.w))
        m = self.maps[-1]
        m[0] += r0
        m[1] += m[2] * c0
        self.h, self.w = r1 - r0, c1 - c0

    def resize(self, h, w):
        self.stages.append((self.h, self.w, int(h), int(w)))
        self.maps.append([0, 0, 1])
        self.h, self.w = int(h), int(w)

    def launches(self):
        """The plan as ``ops.data_transform`` plans of at most two stages each: ``(stages, maps, (out_h, out_w))``.  More
        than two resizes go through intermediate maps: every launch but the last writes the whole output of its second
        stage, and the next one starts with the map that lay on it."""
        maps = [(m[0], m[1], m[2] < 0) for m in self.maps]
        n = len(self.stages)
        out = []
        lo = 0
        while True:
            hi = min(lo + 2, n)
            if hi == n:
                out.append((self.stages[lo:hi], maps[lo:hi + 1], (self.h, self.w)))
                return out
            out.append((self.stages[lo:hi], maps[lo:hi] + [(0, 0, False)], self.stages[hi - 1][2:]))
            lo = hi


class RawSource:
    """A ``d``, ``m``, ``s`` or ``x`` source as the image decoder left it: the raw device array and what it encodes.  The
    gather decodes the pixels it reads (``ops.data_transform(kind=...)``, csrc/data_tf.hip), so nothing passes over the whole
    source on the host; the one thing that has to see every pixel -- the min / max of a normalised depth, of ``x``, and the
    mask's "max > 127" -- is two launches on the raw bytes (``ops.data_source_minmax``) unless the caller knows it.

    ``kind``:
      "unity_d"    uint8 [H, W, 3 or 4]: Unity's depth code (tutils.py:237-293), with ``far``, ``log``, ``normalize``
      "kitti_d"    uint16 [H, W]: centimetres (tutils.py:207-217), with ``log``, ``normalize``
      "f32_d"      float32 [H, W]: the real domain's depth, min-max normalised (tutils.py:197-201)
      "mask"       uint8 [H, W] or [H, W, C]: ``> 127`` when the file's max is above 127, channel 0 (data.py:391-397);
                   ``threshold`` = that flag when the caller knows it
      "kitti_s"    uint8 [H, W, 3]: ``process_kitti_seg`` (data.py:129-148), float64 class ids
      "palette_s"  uint8 [H, W, 4] RGBA: ``encode_segmap`` (data.py:231-252) for ``domain`` "s" or "r", fp32 class ids
      "x"          uint8 [H, W, 3 or 4]: ``arr -= arr.min(); arr /= arr.max()`` (data.py:385-387), read by the bilinear mode
                   as ``((float)v - min) / (max - min)``: a quarter of the upload of the fp32 tensor, the same bits
    ``minmax`` = the known (min, max) of the decoded map (of the raw bytes for "x").  A fourth channel of "x" and "mask" is
    dropped first, as tensor_loader does (data.py:382-383).  Dtype, dimensions and channel counts: ``ops.RAW_KINDS``."""

    def __init__(self, arr, kind, far=1000, log=False, normalize=False, minmax=None, threshold=None, palette=None):
        if kind not in ops.RAW_KINDS:
            raise ValueError("RawSource: kind %r; one of %s" % (kind, sorted(ops.RAW_KINDS)))
        assert not (normalize and log)                                          # tutils.py:196
        code, self.task, _, dims, chans = ops.RAW_KINDS[kind]
        if arr.dtype != ops.raw_dtype(code) or arr.dim() not in dims:
            raise RuntimeError("RawSource: %r is a %s array of %s dimensions, got %s %s"
                               % (kind, ops.raw_dtype(code), " or ".join(map(str, dims)), tuple(arr.shape), arr.dtype))
        if chans is not None and arr.shape[2] not in chans:
            raise RuntimeError("RawSource: %r has %s channels, got %d" % (kind, " or ".join(map(str, chans)), arr.shape[2]))
        if kind in ("x", "mask") and arr.dim() == 3 and arr.shape[2] == 4:
            arr = arr[:, :, :3]
        if self.task == "s" and palette is None:
            raise ValueError("RawSource: %r needs its palette (climategan_amd.data builds it)" % kind)
        self.t, self.kind, self.code, self.palette = arr, kind, code, palette
        self.far, self.log = float(far), bool(log)
        self.normalize = bool(normalize) or kind == "f32_d"
        self.threshold = None
        self.min = self.range = None
        self.set_known(minmax, threshold)

    def set_known(self, minmax=None, threshold=None):
        """What the caller knows of the whole source, so that no launch has to look for it: ``minmax`` and, for a mask,
        ``threshold`` (see the class docstring); None leaves a value as it is."""
        if threshold is not None:
            self.threshold = bool(threshold)
        if minmax is not None:
            # ``t - min`` then ``/ max(t - min)``: the divisor is the fp32 difference
            self.min = float(np.float32(minmax[0]))
            self.range = float(np.float32(minmax[1]) - np.float32(minmax[0]))
        return self

    @classmethod
    def from_numpy(cls, arr, kind, device, **kw):
        return cls(torch.from_numpy(np.ascontiguousarray(arr)).to(device), kind, **kw)

    @property
    def shape(self):
        return (1, 3 if self.kind == "x" else 1, int(self.t.shape[0]), int(self.t.shape[1]))

    @property
    def needs_stats(self):
        """Whether the launch needs this sample's whole-source min / max from the device"""
        if self.kind == "mask":
            return self.threshold is None
        if self.kind == "x" or (self.normalize and self.kind in ("unity_d", "kitti_d", "f32_d")):
            return self.min is None
        return False

    @property
    def flags(self):
        return ((ops.DTF_DEC_LOG if self.log else 0) | (ops.DTF_DEC_NORMALIZE if self.normalize and self.kind != "f32_d" else 0)
                | (ops.DTF_DEC_THRESHOLD if self.threshold else 0))

    @property
    def decode(self):
        """This sample's record for ``ops.data_transform(kind=...)``"""
        return ops.DataDecode(self.flags, self.far, None if self.min is None else (self.min, self.range))

    def to_tensor(self):
        """``tensor_loader``'s [1, C, H, W] tensor: the identity plan through the same kernel"""
        _, _, h, w = self.shape
        return _run_raw([self], [Plan(h, w).launches()[0]])


def _run_raw(sources, plans, dense=True, **kw):
    """One launch over raw sources of one kind (plus the two min / max launches when a sample needs them)"""
    first = sources[0]
    table = None if first.palette is None else bytes(first.palette)
    if any(s.kind != first.kind or (None if s.palette is None else bytes(s.palette)) != table for s in sources):
        raise TypeError("BatchTransform: one launch reads one kind of source with one palette, got %s"
                        % sorted({s.kind for s in sources}))
    arrays = [s.t for s in sources]
    stats = None
    if any(s.needs_stats for s in sources):
        stats = ops.data_source_minmax(arrays, first.code, far=[s.far for s in sources])
    return ops.data_transform(arrays, plans, _mode(first.task), kind=first.code, decode=[s.decode for s in sources],
                              palette=first.palette, stats=stats, dense=dense, **kw)


def _hw(v):
    return tuple(int(a) for a in v.shape[-2:])


def _lead(data):
    """The entry that decides sizes and windows for every task: ``x`` when the sample has one, else its first entry
    (transforms.py:124, :165)"""
    return data["x"] if "x" in data else next(iter(data.values()))


def _pair(size, what):
    """(h, w) from an int (both sides) or a sequence of two"""
    if isinstance(size, int):
        return size, size
    assert isinstance(size, (tuple, list)) and len(size) == 2, "%s: an int or (h, w), got %r" % (what, size)
    return size[0], size[1]


def _tensors_only(data, who):
    """The per-sample classes read device tensors; a ``RawSource`` belongs to the batch form (or ``to_tensor()`` first)"""
    for task, v in data.items():
        if isinstance(v, RawSource):
            raise TypeError("%s: %r is a RawSource; the per-sample transforms take tensors -- call .to_tensor() first, or use "
                            "compile_transforms, which reads the raw array directly" % (who, task))


def _run_one(tensor, plan, mode, **kw):
    """One sample through its plan in one launch (the per-sample classes never chain more than two resizes)"""
    launches = plan.launches()
    assert len(launches) == 1
    return ops.data_transform([tensor], [launches[0]], mode, **kw)


class Resize:
    """reference transforms.py:29-147: an int or (h, w) target, a dict ``{"default": n, task: n}`` of per-task sizes, or an
    int with ``keep_aspect_ratio`` (the smallest side becomes the target).  Attributes as in the reference: ``h`` / ``w``
    (not for a dict), ``default_h`` / ``default_w``, ``sizes`` = {task: {"h": n, "w": n}}, ``keep_aspect_ratio``."""

    def __init__(self, target_size, keep_aspect_ratio=False):
        self.keep_aspect_ratio = keep_aspect_ratio
        self.sizes = {}
        if isinstance(target_size, dict):
            assert not keep_aspect_ratio, "per-task sizes (a dict target_size) cannot keep the aspect ratio"
            self.sizes = {task: {"h": n, "w": n} for task, n in target_size.items() if task != "default"}
            self.default_h = self.default_w = int(target_size["default"])
            return
        assert isinstance(target_size, int) or not keep_aspect_ratio, "keep_aspect_ratio takes one int: the short side"
        self.h, self.w = _pair(target_size, "Resize")
        self.default_h, self.default_w = int(self.h), int(self.w)

    def compute_new_default_size(self, tensor):
        """(new_h, new_w) for a source of ``tensor.shape[-2:]``"""
        if not self.keep_aspect_ratio:
            return (self.default_h, self.default_w)
        src_h, src_w = tensor.shape[-2:]
        # the short side becomes the target, the long one int(target * long / short) in Python floats (transforms.py:90-96);
        # a square source counts as portrait
        if src_h < src_w:
            return (self.h, int(self.default_h * src_w / src_h))
        return (int(self.default_h * src_h / src_w), self.default_w)

    def compute_new_size_for_task(self, task):
        assert not self.keep_aspect_ratio, "per-task sizes and keep_aspect_ratio exclude each other"
        own = self.sizes.get(task)
        return (self.default_h, self.default_w) if own is None else (own["h"], own["w"])

    def new_sizes(self, shapes):
        """{task: (h, w)} for a dict of objects with ``.shape``.  Without per-task sizes the new size comes from ``x``
        (else the first entry) and goes to EVERY task whatever that task's own size (transforms.py:121-130); with
        per-task sizes nobody's own size matters, ``x``'s included (:132-136)."""
        if not self.sizes:
            new_size = self.compute_new_default_size(_lead(shapes))
            return {task: new_size for task in shapes}
        return {task: self.compute_new_size_for_task(task) for task in shapes}

    def __call__(self, data):
        _tensors_only(data, "Resize")
        out = {}
        for task, new_size in self.new_sizes(data).items():
            plan = Plan(*_hw(data[task]))
            plan.resize(*new_size)
            out[task] = _run_one(data[task], plan, _mode(task))
        return out


class RandomCrop:
    """reference transforms.py:150-178.  The window comes from ``x`` (else the first entry) and is cut out of every task
    whatever its own size (:164-178); ``np.random.randint(0, H - h)`` never returns the last offset and raises ValueError
    when ``H <= h`` (:169-170).  The result is a view, as in the reference."""

    def __init__(self, size, center=False):
        h, w = _pair(size, "RandomCrop")
        self.h, self.w = int(h), int(w)
        self.center = center
        self.draws = PipelineDraws()

    def window(self, H, W):
        """(top, left) in an H x W map: centred, or drawn -- top first, then left"""
        if self.center:
            return (H - self.h) // 2, (W - self.w) // 2
        top = self.draws.randint(0, H - self.h)
        return top, self.draws.randint(0, W - self.w)

    def __call__(self, data):
        _tensors_only(data, "RandomCrop")
        top, left = self.window(*_hw(_lead(data)))
        return {task: tensor[:, :, top:top + self.h, left:left + self.w] for task, tensor in data.items()}


class RandomHorizontalFlip:
    """reference transforms.py:181-189: flips every task iff ``not (np.random.rand() > p)``"""

    def __init__(self, p=0.5):
        self.p = p
        self.draws = PipelineDraws()

    def drawn(self):
        return not (self.draws.rand() > self.p)

    def __call__(self, data):
        _tensors_only(data, "RandomHorizontalFlip")
        if not self.drawn():
            return data
        out = {}
        for task, tensor in data.items():
            plan = Plan(*_hw(tensor))
            plan.flip()
            out[task] = _run_one(tensor, plan, ops.DTF_NEAREST)   # a pure gather, any element type
        return out


class Normalize:
    """reference transforms.py:214-237: ``(x - mean) / std`` per channel on ``x`` (0.5 / 0.5, or the ImageNet constants
    when ``data.normalization == "HRNet"``), the identity on everything else; EVERY task loses its batch dimension (:235)."""

    def __init__(self, opts):
        if opts.data.normalization == "HRNet":
            self.mean, self.std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
        else:                                       # "default", or no such key in a hand-made ``config.Opts``
            self.mean, self.std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)

    def __call__(self, data):
        _tensors_only(data, "Normalize")
        out = {}
        for task, tensor in data.items():
            if task == "x":
                tensor = _run_one(tensor, Plan(*_hw(tensor)), ops.DTF_BILINEAR, normalize=(self.mean, self.std))
            out[task] = tensor.squeeze(0)
        return out


def _jitter_factors(values, device):
    """[n, 2] fp32 (f, 1 - f): torchvision's ``_blend`` forms ``1.0 - ratio`` in a Python float before it meets the image"""
    return torch.tensor([[f, 1.0 - f] for f in values], dtype=torch.float32).to(device)


class _RandJitter:
    op = None

    def __init__(self):
        self.draws = PipelineDraws()

    def factor(self):
        return self.draws.uniform(0.5, 1.5)

    def __call__(self, data):
        _tensors_only(data, type(self).__name__)
        out = {}
        for task, tensor in data.items():
            if task == "x":
                tensor = ops.data_jitter(tensor, self.op, _jitter_factors([self.factor()], tensor.device))
            out[task] = tensor
        return out


class RandBrightness(_RandJitter):
    """reference transforms.py:240-245 -> :501-507: ``clamp(f x, 0, 1)``, f from ``random.uniform(0.5, 1.5)``, then the
    dummy pixels ``[0, 0] = 1``, ``[-1, -1] = 0`` (torchvision's documented formula, see the module docstring)"""
    op = ops.JIT_BRIGHTNESS


class RandSaturation(_RandJitter):
    """reference transforms.py:248-253 -> :518-524: ``clamp(f x + (1 - f) gray, 0, 1)``, then the dummy pixels"""
    op = ops.JIT_SATURATION


class RandContrast(_RandJitter):
    """reference transforms.py:256-261 -> :535-541: ``clamp(f x + (1 - f) mean(gray), 0, 1)``, then the dummy pixels"""
    op = ops.JIT_CONTRAST


class BucketizeDepth:
    """reference transforms.py:264-289: with ``gen.d.classify.enable`` in the domains ``s`` and ``kitti``, ``d`` becomes
    ``torch.bucketize(d, linspace(min, max, buckets - 1), right=True, out_int32=True)``; otherwise the identity."""

    def __init__(self, opts, domain):
        self.domain = domain
        self.buckets = None
        classify = opts.gen.d.classify          # absent in a hand-made ``config.Opts``: reads as disabled
        if classify.enable and domain in {"s", "kitti"}:
            self.buckets = torch.linspace(classify.linspace.min, classify.linspace.max, classify.linspace.buckets - 1)
        self._on_device = {}

    def boundaries(self, device):
        if device not in self._on_device:
            self._on_device[device] = self.buckets.to(device=device, dtype=torch.float32).contiguous()
        return self._on_device[device]

    def __call__(self, data):
        out = {}
        for task, tensor in data.items():
            if task == "d" and self.buckets is not None:
                shape = tuple(tensor.shape)
                tensor = _run_one(tensor if tensor.dim() >= 3 else tensor.unsqueeze(0), Plan(*_hw(tensor)),
                                  ops.DTF_NEAREST, boundaries=self.boundaries(tensor.device)).reshape(shape)
            out[task] = tensor
        return out


_ITEMS = {
    "crop": lambda item, mode: RandomCrop((item.height, item.width), center=item.center == mode),
    "resize": lambda item, mode: Resize(item.new_size, item.get("keep_aspect_ratio", False)),
    "hflip": lambda item, mode: RandomHorizontalFlip(p=item.p or 0.5),
    "brightness": lambda item, mode: RandBrightness(),
    "saturation": lambda item, mode: RandSaturation(),
    "contrast": lambda item, mode: RandContrast(),
}


def get_transform(transform_item, mode):
    """reference transforms.py:424-468: the transform of one ``opts.data.transforms`` item; None for an item whose
    ``ignore`` is True or names this mode; ValueError for an unknown item that is not ignored."""
    ignored = transform_item.ignore is True or transform_item.ignore == mode
    if ignored:
        return None
    if transform_item.name in _ITEMS:
        return _ITEMS[transform_item.name](transform_item, mode)
    raise ValueError("Unknown transform_item {}".format(transform_item))


_JITTER_ITEMS = ("brightness", "saturation", "contrast")


def get_transforms(opts, mode, domain, draws=None):
    """reference transforms.py:471-490: the geometric items of ``opts.data.transforms`` in their order, then (train mode
    without the Painter task only) the colour-jitter items in theirs, then ``Normalize`` and ``BucketizeDepth``; ignored
    items leave no entry.  ``draws``: the source of the random draws of every returned transform (default: the
    reference's numpy / random calls)."""
    items = list(opts.data.transforms)
    ordered = [item for item in items if item.name not in _JITTER_ITEMS]
    if mode == "train" and "p" not in opts.tasks:
        ordered += [item for item in items if item.name in _JITTER_ITEMS]
    built = (get_transform(item, mode) for item in ordered)
    transforms = [t for t in built if t is not None] + [Normalize(opts), BucketizeDepth(opts, domain)]
    if draws is not None:
        set_draws(transforms, draws)
    return transforms


def set_draws(transforms, draws):
    for t in transforms:
        if hasattr(t, "draws"):
            t.draws = draws


class Compose:
    """``torchvision.transforms.Compose`` for a list of the transforms above (what the reference's dataset builds)."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, data):
        for t in self.transforms:
            data = t(data)
        return data


class BatchTransform:
    """The transform list of ``get_transforms`` on a whole batch: ``batch(samples)`` with ``samples`` a list of N dicts
    ``{task: [1, C, H, W] device tensor}`` (or, for every sample of a task, a ``RawSource`` of its kind) returns
    ``{task: [N, C, h, w]}``, the reference's collated batch.  Per sample it makes the reference's draws in the reference's
    order and reduces every task's flips, crops and resizes to a ``Plan`` on the host; then each task is ONE launch for the
    whole batch (one more per two further resizes beyond the second), plus one launch per colour-jitter item on ``x`` (two
    for contrast: its mean)."""

    def __init__(self, transforms, draws=None):
        self.transforms = list(transforms)
        if draws is not None:
            set_draws(self.transforms, draws)
        seen_pixel_op = False
        for t in self.transforms:
            if isinstance(t, (Resize, RandomCrop, RandomHorizontalFlip)):
                if seen_pixel_op:
                    raise NotImplementedError("BatchTransform: flips, crops and resizes come before the colour jitter, "
                                              "Normalize and BucketizeDepth, as get_transforms orders them")
            elif isinstance(t, (_RandJitter, Normalize, BucketizeDepth)):
                seen_pixel_op = True
            else:
                raise NotImplementedError("BatchTransform: no batch form of %r" % (t,))

    def plan_sample(self, shapes):
        """One sample's draws and plans: ``shapes`` = {task: object with .shape}; returns ({task: Plan}, [jitter factors])"""
        plans = {task: Plan(*_hw(v)) for task, v in shapes.items()}
        factors = []
        for t in self.transforms:
            if isinstance(t, RandomHorizontalFlip):
                if t.drawn():
                    for p in plans.values():
                        p.flip()
            elif isinstance(t, RandomCrop):
                lead = _lead(plans)
                top, left = t.window(lead.h, lead.w)
                for p in plans.values():
                    p.crop(top, left, t.h, t.w)
            elif isinstance(t, Resize):
                for task, size in t.new_sizes({k: _Shape(p.h, p.w) for k, p in plans.items()}).items():
                    plans[task].resize(*size)
            elif isinstance(t, _RandJitter) and "x" in plans:
                factors.append(t.factor())
        return plans, factors

    def __call__(self, samples):
        if not samples:
            raise ValueError("BatchTransform: an empty batch")
        tasks = list(samples[0])
        if any(list(s) != tasks for s in samples):
            raise ValueError("BatchTransform: every sample of a batch holds the same tasks in the same order")
        planned = [self.plan_sample(s) for s in samples]
        jitter = [t for t in self.transforms if isinstance(t, _RandJitter)]
        norm = next((t for t in self.transforms if isinstance(t, Normalize)), None)
        bucket = next((t for t in self.transforms if isinstance(t, BucketizeDepth) and t.buckets is not None), None)
        out = {}
        for task in tasks:
            sources = [s[task] for s in samples]
            n_raw = sum(isinstance(v, RawSource) for v in sources)
            if n_raw not in (0, len(sources)) or any(isinstance(v, RawSource) and v.task != task for v in sources):
                raise TypeError("BatchTransform: %r is a RawSource in %d of %d samples, or of another task's kind; one "
                                "launch reads one kind of source" % (task, n_raw, len(sources)))
            chunks = [p[task].launches() for p, _ in planned]
            mode = _mode(task)
            for i in range(len(chunks[0])):
                last = i == len(chunks[0]) - 1
                kw = {}
                if last and task == "x" and norm is not None and not jitter:
                    kw["normalize"] = (norm.mean, norm.std)
                if last and task == "d" and bucket is not None:
                    kw["boundaries"] = bucket.boundaries((sources[0].t if n_raw and i == 0 else sources[0]).device)
                if n_raw and i == 0:        # the decode belongs to the launch that reads the source
                    sources = _run_raw(sources, [c[i] for c in chunks], dense=last, **kw)
                else:
                    sources = ops.data_transform(sources, [c[i] for c in chunks], mode, dense=last, **kw)
            y = sources
            if task == "x":
                for k, t in enumerate(jitter):
                    f = _jitter_factors([fs[k] for _, fs in planned], y.device)
                    y = ops.data_jitter(y, t.op, f, normalize=(norm.mean, norm.std)
                                        if norm is not None and k == len(jitter) - 1 else None)
            out[task] = y
        return out


class _Shape:
    def __init__(self, h, w):
        self.shape = (1, 1, h, w)


def compile_transforms(opts, mode, domain, draws=None):
    """``BatchTransform(get_transforms(opts, mode, domain))``: the batch form of the reference's per-sample pipeline."""
    return BatchTransform(get_transforms(opts, mode, domain), draws=draws)
