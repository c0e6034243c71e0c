"""The device JPEG encoder (csrc/jpeg.hip) against the host model ``tests/jpeg_model.py`` (pinned to libjpeg by
``test_jpeg_host.py``):

transform   ``ops.jpeg_coefficients`` equals the model's float64 coefficients except where the model's unrounded quotient lies
            within BAND of a rounding boundary (fp32 against fp64: measured quotient error at most 6e-5); at most 2 % of a
            case's coefficients may lie there
coding      the file of ``ops.jpeg_encode`` is, byte for byte, the model's ``write`` and ``cgan_jpeg_scan_host`` of the device's
            own coefficients
decoding    PIL loads every file; its pixels equal those of the model's file in every MCU without a band coefficient (4:2:0:
            and without one in a neighbouring MCU, because libjpeg's chroma upsampling reads across the MCU's border)
"""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as jm
from climategan_amd import _lib, ops

pytestmark = pytest.mark.gpu

BAND = 2e-3
BAND_SHARE = 0.02
SIZES = (1, 7, 8, 9, 16, 17, 33)
QUALITIES = (25, 90, 100)
MODES = [(1, "444"), (1, "420"), (3, "444"), (3, "420")]


def band_of(quot):
    return np.abs(np.abs(quot - np.floor(quot)) - 0.5) < BAND


@functools.lru_cache(maxsize=None)
def case_image(kind, h, w, c):
    """The case's image.  The band share is a condition on the case, decided by the model alone: the first seed of
    ``make_image`` is taken at which it holds for every quality and subsampling of the grid (a 64-coefficient case leaves
    the 2 % with its second band coefficient, which a tenth of all noise seeds have; the 0 / 255 patterns cut by an edge put
    several quotients exactly on a tie).  Seeds stay below 60, so that the checker keeps its DC differences of category 11
    and p44 its AC value of category 10."""
    for seed in range(60):
        img = jm.make_image(kind, h, w, c, seed)
        if all(band_of(jm.transform(img, q, sub)[1]).mean() <= BAND_SHARE for q in QUALITIES for sub in ("444", "420")[:c]):
            return img
    raise AssertionError("no seed meets the band-share condition for %s %d x %d x %d" % (kind, h, w, c))


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def scan_host(coef, h, w, c, quality, sub):
    lib = _lib.load()
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    cap = lib.cgan_jpeg_bound_bytes(h, w, c, int(sub))
    out = np.zeros(cap, dtype=np.uint8)
    size = C.c_size_t(0)
    _lib.check(lib.cgan_jpeg_scan_host(coef.ctypes.data, h, w, c, quality, int(sub), out.ctypes.data, cap, C.addressof(size)),
               "cgan_jpeg_scan_host")
    return out[:size.value].tobytes()


def device_run(batch, quality, sub):
    """uint8 [N, H, W, C] array -> (coefficients int16 [N, blocks * 64], list of N files)."""
    x = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    coef = ops.jpeg_coefficients(x, quality, sub)
    buf, sizes = ops.jpeg_encode(x, quality, sub)
    sizes = sizes.cpu().tolist()
    assert max(sizes) <= ops.jpeg_bound_bytes(*batch.shape[1:], sub) == buf.shape[1]
    buf = buf[:, :max(sizes)].cpu().numpy()
    return coef.cpu().numpy(), [buf[i, :k].tobytes() for i, k in enumerate(sizes)]


def mcu_any(g, flags):
    """per-coefficient flags (the coefficient layout) -> bool [mcus_y, mcus_x]: the MCU holds a flagged coefficient."""
    out = np.zeros((g.mcus_y, g.mcus_x), dtype=bool)
    for k, comp in enumerate(g.split(flags)):
        per_block = comp.any(axis=2)
        v = g.v if k == 0 else 1
        out |= per_block.reshape(g.mcus_y, v, g.mcus_x, v).any(axis=(1, 3))
    return out


def check_case(img, quality, sub, got_coef, got_file, what):
    h, w, c = img.shape
    g = jm.Geometry(h, w, c, sub)
    want_coef, quot = jm.transform(img, quality, sub)
    band = band_of(quot)
    assert band.mean() <= BAND_SHARE, (what, "band share", band.mean())
    differs = got_coef != want_coef
    assert not (differs & ~band).any(), (what, "coefficients differ outside the band", int((differs & ~band).sum()),
                                         np.abs(got_coef.astype(int) - want_coef)[~band].max())
    assert np.abs(got_coef.astype(int) - want_coef).max() <= 1, what
    mine = jm.write(got_coef, h, w, c, quality, sub)
    assert got_file == mine, (what, "the file is not the model's coding of the device's coefficients")
    assert got_file == scan_host(got_coef, h, w, c, quality, sub), (what, "cgan_jpeg_scan_host")
    pixels = decode(got_file)
    assert pixels.shape == ((h, w, 3) if c == 3 else (h, w)), what
    if differs.any():
        model_pixels = decode(jm.write(want_coef, h, w, c, quality, sub))
        dirty = mcu_any(g, band)
        if g.v == 2:                                  # the chroma upsampling reads the neighbouring MCUs' samples
            p = np.pad(dirty, 1)
            dirty = np.stack([p[1 + dy:1 + dy + g.mcus_y, 1 + dx:1 + dx + g.mcus_x] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]).any(0)
        clean = np.repeat(np.repeat(~dirty, g.mcu, axis=0), g.mcu, axis=1)[:h, :w]
        assert np.array_equal(pixels[clean], model_pixels[clean]), what


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("c,sub", MODES)
def test_grid(c, sub, quality):
    for h in SIZES:
        for w in SIZES:
            batch = np.stack([case_image(kind, h, w, c) for kind in jm.CONTENTS])
            coef, files = device_run(batch, quality, sub)
            for i, kind in enumerate(jm.CONTENTS):
                check_case(batch[i], quality, sub, coef[i], files[i], (kind, h, w, c, sub, quality))


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("c,sub", MODES)
@pytest.mark.parametrize("h,w", [(136, 24), (16, 640), (8, ops.JPEG_MAX_WIDTH)])
def test_long_and_wide(h, w, c, sub, quality):
    """17 MCU rows (RST7 wraps to RST0); rows of 3 and of 16 segments with bits carried between them."""
    batch = np.stack([case_image(kind, h, w, c) for kind in jm.CONTENTS])
    coef, files = device_run(batch, quality, sub)
    for i, kind in enumerate(jm.CONTENTS):
        check_case(batch[i], quality, sub, coef[i], files[i], (kind, h, w, c, sub, quality))


def test_batch_independence():
    batch = np.stack([jm.make_image("noise", 33, 41, 3, seed=s) for s in (1, 2, 3)])
    _, together = device_run(batch, 90, "420")
    _, again = device_run(batch, 90, "420")
    assert together == again
    for i in range(3):
        assert device_run(batch[i:i + 1], 90, "420")[1][0] == together[i]
    assert len(set(together)) == 3


def test_refusals():
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros(1, 8, 8, 2, dtype=torch.uint8, device="cuda"),
                torch.zeros(1, 8, ops.JPEG_MAX_WIDTH + 1, 3, dtype=torch.uint8, device="cuda"),
                torch.zeros(1, 8, 8, 3, dtype=torch.uint8),
                torch.zeros(1, 8, 8, 3, dtype=torch.int8, device="cuda"),
                torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")):
        for fn in (ops.jpeg_encode, ops.jpeg_coefficients):
            with pytest.raises(RuntimeError):
                fn(bad)
    for fn in (ops.jpeg_encode, ops.jpeg_coefficients):
        for q in (0, 101, 90.0):
            with pytest.raises(RuntimeError):
                fn(x, q)
        with pytest.raises(RuntimeError):
            fn(x, 90, "422")
    # the C ABI refuses the same before any launch, with a message
    lib = _lib.load()
    p = C.c_void_p(x.data_ptr())
    for args in ((1, 8, 8, 2, 90, 444), (1, 8, 8, 3, 0, 444), (1, 8, 8, 3, 101, 444), (1, 8, 4097, 3, 90, 444),
                 (1, 8, 8, 3, 90, 422), (65536, 8, 8, 3, 90, 444)):
        assert lib.cgan_jpeg_coefficients_u8(p, *args, p, None) != 0
        assert lib.cgan_jpeg_encode_u8(p, *args, p, 1 << 30, p, p, 1 << 30, None) != 0
        assert lib.cgan_last_error()
    torch.cuda.synchronize()
