"""The wide unfilter's shape list for test_png_unfilter_wide_host.py, test_gpu_png_unfilter_wide.py and
tools/png_unfilter_wide_asan.cpp's input: for a workgroup of ``nw`` waves and a lag of ``lag`` steps, files whose heights and
widths sit on every edge of the schedule -- one row, one wave's rows +- 1, one pass's rows +- 1, two passes and a bit; one
pixel, a chunk of the prefetch +- 1, a wave's width, the distance between two waves +- 1 -- in the four pixel kinds, the five
filters cycling, half of them row-framed.  Everything is made here, deterministically, from ``png_rows_cases`` and
``png_decode_corpus``, which are imported, not changed."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

import jpeg_model as jm
import png_decode_corpus as pc
import png_decode_model as pm
import png_rows_cases as rc
from climategan_amd import _lib

MODES = rc.MODES
WAVES, LAGS_IN_PREFETCHES = (1, 2, 4, 16), (1, 2)
ERR_INTERNAL = -5


@functools.lru_cache(maxsize=None)
def compiled():
    """(waves, lag, prefetch) of the kernel in the library."""
    v = [C.c_int32(0) for _ in range(3)]
    _lib.load().cgan_png_unfilter_wide_params(*[C.addressof(x) for x in v])
    return tuple(x.value for x in v)


def prefetch():
    return compiled()[2]


def lags():
    return tuple(k * prefetch() for k in LAGS_IN_PREFETCHES)


def heights(nw):
    return (1, 63, 64, 65, 64 * nw - 1, 64 * nw, 64 * nw + 1, 2 * 64 * nw + 3)


def widths(lag):
    return (1, 2, prefetch() - 1, prefetch(), 63, 64 + lag, 64 + lag + 1, 200)


@functools.lru_cache(maxsize=None)
def _file(h, w, mode, framed, filters=(0, 1, 2, 3, 4)):
    kind = jm.CONTENTS[1 + (h + w) % 3]                                          # noise, sinusoid, checker
    img = rc.image(kind, h, w, mode)
    data = rc.flushed_file(img, filters, level=1) if framed else pm.write(img, filters, level=1)
    return img, data


@functools.lru_cache(maxsize=None)
def files(nw, lag):
    """[(name, the array the file holds, the file's bytes)] for one (waves, lag)."""
    out = []
    for ih, h in enumerate(sorted(set(heights(nw)))):
        for iw, w in enumerate(sorted(set(widths(lag)))):
            mode, framed = MODES[(ih + iw) % 4], (ih + 2 * iw) % 3 == 0
            img, data = _file(h, w, mode, framed)
            out.append(("%dx%d-%s%s" % (h, w, mode, "-framed" if framed else ""), img, data))
    h, w = 64 * nw + 1, 64 + lag + 1
    out.append(("all-paeth-%dx%d-RGB" % (h, w),) + _file(h, w, "RGB", False, (4,)))
    out.append(("all-average-%dx%d-RGBA" % (h, w),) + _file(h, w, "RGBA", False, (3,)))
    return tuple(out + list(extremes()))


@functools.lru_cache(maxsize=None)
def extremes():
    """The most passes a file can take, and the widest row."""
    return (("8192x3-L",) + _file(8192, 3, "L", False), ("2x8192-RGBA-framed",) + _file(2, 8192, "RGBA", True))


def tiny():
    return ("1x1-L",) + _file(1, 1, "L", False)


@functools.lru_cache(maxsize=None)
def broken(nw, lag):
    """[(name, bytes)]: files whose deflate streams are valid and whose unfilter stage must report CORRUPT -- a byte of the
    filtered rows changed under the original's Adler-32, in a row of the second wave (the first, for one wave) and in the
    second pass; a filter byte of 5 in the last row."""
    h, w = 64 * nw + 1, 64 + lag + 1
    img = rc.image("sinusoid", h, w, "RGB")
    px, bpp, _, _ = pm.image_bytes(img)
    raw = pm.filter_rows(px, bpp, (0, 1, 2, 3, 4))
    row_len = 1 + px.shape[1]
    out = []
    for name, y in (("changed-byte-wave-1", min(64, h - 2) + 3 if nw > 1 else 3), ("changed-byte-pass-1", h - 1)):
        changed = bytearray(raw)
        changed[y * row_len + 1 + row_len // 2] ^= 0x55
        stream = zlib.compress(bytes(changed), 1)[:-4] + struct.pack(">I", zlib.adler32(raw))
        out.append((name, pm.frame(img, stream)))
    five = bytearray(raw)
    five[(h - 1) * row_len] = 5
    out.append(("filter-byte-5", pm.frame(img, zlib.compress(bytes(five), 1))))
    return tuple(out)


def shaped(pixels, d):
    return pixels.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else pixels.reshape(d.height, d.width, d.channels)


def wide_host(data, nw, lag):
    """The serial twin, then the wide twin on its inflated bytes -> (wide pixels, wide status, return code, serial pixels,
    serial status)."""
    lib = _lib.load()
    d, status, why = pc.parse_host(data)
    assert status == pc.OK, why
    stream = pc.stream_host(data, d)
    inflated, serial_px, serial_status, _ = pc.decode_host(stream, d)
    src = np.frombuffer(inflated, dtype=np.uint8).copy()
    pixels = np.full(serial_px.nbytes, 0xAA, dtype=np.uint8)
    wide_status = C.c_int32(-1)
    code = lib.cgan_png_unfilter_wide_host(C.addressof(d), src.ctypes.data, int.from_bytes(stream[-4:], "big"), nw, lag,
                                           pixels.ctypes.data, C.addressof(wide_status))
    return shaped(pixels, d), wide_status.value, code, serial_px, serial_status
