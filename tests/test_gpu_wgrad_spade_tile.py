"""The column-walking spatially tiled 3 x 3 weight-gradient kernel (conv_wgrad_col3x3_kernel: all input channels and taps
in one workgroup, rolling x row ring, double-buffered dy) on the smallest shapes that reach each of its paths, forced with
knob 3: against torch's fp32 gradient of the 16-bit-rounded operands (3e-4, the bound of every weight-gradient path) and
against the per-tap kernels (knob 0; 1e-5), the bias gradient, and bit-identical repeats."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from climategan_amd import fill

pytestmark = pytest.mark.gpu


def q(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).float()


def rel_err(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


CASES = [
    (128, 80, 2, 8, 32),     # one column, two tiles per image, two images: zero halo rows, ring carried within an image only
    (128, 40, 1, 12, 64),    # two columns, three tiles: interior horizontal halo, three co tiles
    (64, 80, 1, 8, 32),      # one ci block (four waves)
    (128, 160, 1, 8, 64),    # two co groups
    (128, 130, 1, 8, 32),    # padded channel tail (cs 136), co tiles past cout_s skipped
    (128, 8, 2, 4, 32),      # a single co tile, a single tile per image
    (192, 80, 1, 8, 32),     # preconditions not met (cin_s 192): the plan falls back
    (128, 80, 1, 10, 32),    # preconditions not met (H no tile multiple): the plan falls back
]


@pytest.mark.usefixtures("dev_lib")
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_column_tiled_3x3_wgrad(dt, case):
    from climategan_amd import _lib, ops
    cin, cout, B, H, W = case
    lib = _lib.load()
    x = q(fill.uniform((B, cin, H, W), 900 + cin), dt)
    w = q(fill.uniform((cout, cin, 3, 3), 901 + cout, -0.05, 0.05), dt).requires_grad_(True)
    y = F.conv2d(x, w, None, padding=1)
    dy = q(fill.uniform(tuple(y.shape), 902 + W), dt)
    y.backward(dy)
    db_ref = dy.float().sum((0, 2, 3))
    xg, dyg = ops.nchw_to_nhwc(x.cuda(), dt), ops.nchw_to_nhwc(dy.cuda(), dt)
    try:
        lib.cgan_debug_set_wgrad_tile3x3(ctypes.c_int(0))
        dw_old, _ = ops.conv2d_bwd_weight(xg, dyg, (cout, cin, 3, 3), pad=1)
        lib.cgan_debug_set_wgrad_tile3x3(ctypes.c_int(3))
        # the plan really takes the kernel under test (3 = conv_wgrad_col3x3_kernel) / really falls back
        desc = ops._conv_desc(xg.dtype_id, B, H, W, cin, cout, 3, 3, 1, 1, 1, ops.PAD_ZERO)
        kind = lib.cgan_debug_wgrad_plan_kind(ctypes.byref(desc))
        eligible = cin in (64, 128) and H % 4 == 0 and W % 32 == 0
        assert (kind == 3) == eligible, (kind, case)
        for splits in (0, 1, 3, 1000):      # 1000 > columns x images (and > tiles): clamped
            lib.cgan_debug_set_wgrad(ctypes.c_int(-splits), ctypes.c_int(0))
            dw, db = ops.conv2d_bwd_weight(xg, dyg, (cout, cin, 3, 3), pad=1)
            dw2, db2 = ops.conv2d_bwd_weight(xg, dyg, (cout, cin, 3, 3), pad=1)
            e1, e2, e3 = rel_err(dw.cpu(), w.grad), rel_err(dw.cpu(), dw_old.cpu()), rel_err(db.cpu(), db_ref)
            print(case, dt, splits, "vs torch %.3g  vs per-tap %.3g  bias %.3g" % (e1, e2, e3))
            assert e1 <= 3e-4, ("vs torch fp32", splits)
            assert e2 <= 1e-5, ("vs per-tap kernels", splits)
            assert e3 <= 3e-4, ("bias gradient", splits)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), ("not bit-identical", splits)
    finally:
        lib.cgan_debug_set_wgrad(ctypes.c_int(0), ctypes.c_int(0))
        lib.cgan_debug_set_wgrad_tile3x3(ctypes.c_int(1))
