"""Mirror of the reference's differentiable augmentation (DiffAugment, ``climategan/transforms.py:494-626``): the
``rand_*`` functions with the reference's signatures and ``DiffTransforms``, the transform ``Trainer`` applies to the
Painter discriminator's inputs when ``gen.p.diff_aug.use`` is on (trainer.py:772-773, 1079-1081, 1319-1321).

The random draws are the reference's own torch calls, with the same shapes, dtypes, devices and order (``TorchDraws``), so
that the same generator state gives the same draws; the arithmetic is one HIP kernel pair per batch (``ops.diffaug`` /
``autograd.DiffAugFn``: forward and backward, all ops of the transform fused).  The source of the draws is replaceable
(``RecordedDraws`` replays recorded values) so that tests can compare against the reference's recorded runs.

The non-DiffAugment branches of ``rand_brightness / rand_contrast / rand_saturation`` (``is_diff_augment=False``:
torchvision's ``adjust_*`` on a single image, reference data pipeline) are not part of this package and raise.
"""
from typing import NamedTuple, Optional, Tuple

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
                              "(reference transforms.py:494-541), not part of this package" % name)


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
