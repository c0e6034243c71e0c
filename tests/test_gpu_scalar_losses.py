"""The four GAN-side scalar losses through their autograd functions (autograd.bce_logits_loss, mse_const_loss, hinge_loss,
l1_loss: one ``_ScalarLossFn``, one pointwise kernel with a term per loss, the tuned L1 kernel) against torch float64 on
the same 16-bit-rounded inputs: value, gradient, zero pad channels, the no-gradient path and the AMP gradient scale.

Shapes (logical NCHW) and what each can get wrong: (1,1,5,7) one partial block, 7 pad channels; (2,3,9,11) pad channels
inside a group; (1,9,17,19) two channel groups, the second with 7 pad channels (``i % cg_total``); (3,16,16,16) no pad,
1536 groups = 6 blocks (the cross-block atomic).

Tolerances are those of test_gpu_backward.py.  The weights are the production ones, 1 / numel: the smallest gradient
magnitude that matters, 1 / 12288 = 8.1e-5, is a normal fp16 number, and an entry below fp16's normal range is off by at
most 2^-25 = 3.0e-8, i.e. 4e-4 of the largest entry -- inside TOL[float16] = 1e-3."""
import functools

import pytest
import torch
import torch.nn.functional as F

from climategan_amd import fill
from test_gpu_backward import DTYPES, TOL, q, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 5, 7), (2, 3, 9, 11), (1, 9, 17, 19), (3, 16, 16, 16)]
TARGETS = [1.0, 0.0, 0.87]
HINGE_MODES = [(True, True), (False, True), (True, False)]       # (target_is_real, for_discriminator): the reference allows no other


@functools.lru_cache(maxsize=None)
def inputs(dt, shape):
    """(a, b): 16-bit-rounded fp32 NCHW maps; a holds exact +1 / -1 entries (the hinge's ties), first and last element
    included, and b equals a in a few places (sign(0) = 0 in the L1 gradient)."""
    a = q(fill.uniform(shape, 4100 + shape[1], -4, 4), dt)
    b = q(fill.uniform(shape, 4200 + shape[1], -4, 4), dt)
    fa, fb = a.view(-1), b.view(-1)
    fa[0::7] = 1.0
    fa[3::11] = -1.0
    fa[-1] = 1.0
    fb[5::13] = fa[5::13]
    return a, b


def hinge_ref(x, real, disc):
    """reference losses.py:568-579"""
    if not disc:
        return -torch.mean(x)
    return -torch.mean(torch.min((x if real else -x) - 1, torch.zeros_like(x)))


def cases(kind, b_map, b_ref):
    """[(label, device loss of an ops.NHWC map with weight w, float64 reference of an NCHW tensor)]"""
    from climategan_amd import autograd as ag
    if kind == "bce":
        return [("t=%g" % t, lambda m, w, t=t: ag.bce_logits_loss(m, t, w),
                 lambda x, t=t: F.binary_cross_entropy_with_logits(x, torch.full_like(x, t))) for t in TARGETS]
    if kind == "mse":
        return [("t=%g" % t, lambda m, w, t=t: ag.mse_const_loss(m, t, w), lambda x, t=t: ((x - t) ** 2).mean())
                for t in TARGETS]
    if kind == "hinge":
        return [("real=%d disc=%d" % (r, d), lambda m, w, r=r, d=d: ag.hinge_loss(m, r, d, w),
                 lambda x, r=r, d=d: hinge_ref(x, r, d)) for r, d in HINGE_MODES]
    return [("", lambda m, w: ag.l1_loss(m, b_map, w), lambda x: F.l1_loss(x, b_ref))]


def run(loss_fn, a, dt, c, w, requires_grad=True):
    """-> (value, gradient as fp32 NCHW on the host, raw NHWC gradient) of the device loss on the map of ``a``"""
    from climategan_amd import ops
    t = ops.nchw_to_nhwc(a.cuda(), dt).t.requires_grad_(requires_grad)
    val = loss_fn(ops.NHWC(t, c), w)
    if not requires_grad:
        return val, None, None
    val.backward()
    return val, ops.nhwc_to_nchw(ops.NHWC(t.grad, c)).cpu(), t.grad


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["bce", "mse", "hinge", "l1"])
def test_scalar_loss_value_grad_and_scale(dt, shape, kind, monkeypatch):
    from climategan_amd import autograd as ag
    from climategan_amd import ops
    a, b = inputs(dt, shape)
    c, w = shape[1], 1.0 / a.numel()
    b_map = ops.nchw_to_nhwc(b.cuda(), dt)
    for label, loss_fn, ref_fn in cases(kind, b_map, b.double()):
        x = a.double().requires_grad_(True)
        ref = ref_fn(x)
        ref.backward()
        ref, ref_grad = ref.item(), x.grad.float()

        val, grad, raw = run(loss_fn, a, dt, c, w)
        err_v, err_g = abs(val.item() - ref), rel_err(grad, ref_grad)
        print("%s %s %s %s: value %.9g ref %.9g (err %.3g), grad rel_err %.3g" % (kind, label, dt, shape, val.item(), ref, err_v, err_g))
        assert err_v <= 1e-5 * max(1.0, abs(ref))
        assert err_g <= TOL[dt]
        if raw.shape[-1] > c:
            assert raw[..., c:].abs().max().item() == 0

        # an input that wants no gradient: the same value, nothing allocated for a gradient and nothing kept for backward
        made = []
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_empty_like", lambda t, _orig=ops._empty_like: made.append(t.shape) or _orig(t))
            val0, _, _ = run(loss_fn, a, dt, c, w, requires_grad=False)
        assert made == [] and val0.grad_fn is None and not val0.requires_grad
        assert abs(val0.item() - val.item()) <= 1e-6 * abs(val.item())

        # the AMP gradient scale (a power of two): the value stays, the gradient comes out multiplied
        try:
            ag.set_grad_scale(1024.0)
            val_s, grad_s, raw_s = run(loss_fn, a, dt, c, w)
        finally:
            ag.set_grad_scale(1.0)
        print("    scaled: value %.9g, grad rel_err %.3g" % (val_s.item(), rel_err(grad_s, 1024.0 * ref_grad)))
        assert abs(val_s.item() - val.item()) <= 1e-6 * abs(val.item())
        if dt == torch.bfloat16:
            assert torch.equal(raw_s, raw * 1024.0)       # a power of two moves only the exponent
        else:
            assert rel_err(grad_s, 1024.0 * ref_grad) <= TOL[dt]   # small unscaled fp16 entries are subnormal
