"""The files the JPEG decoder's tests share (test_jpeg_decode_host.py, test_gpu_jpeg_decode.py, tools/jpeg_decode_asan.cpp's
input), and the ctypes calls of the host entry points.  Every file is made here, deterministically, by PIL or by
``jpeg_model.write``; the model reader's result of each is computed once and kept."""
import ctypes as C
import functools
import io

import numpy as np
from PIL import Image

import jpeg_decode_model as dm
import jpeg_model as jm
from climategan_amd import _lib

QUALITIES = (25, 90, 100)
SUBS = {"444": 0, "422": 1, "420": 2}
# restart settings as PIL's save() takes them
RESTARTS = ({}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3})
OK, UNSUPPORTED, CORRUPT, NOT_CONVERGED = 0, 1, 2, 4


def pil_file(img, quality, sub, optimize=False, **restart):
    b = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(b, "JPEG", quality=quality, subsampling=SUBS[sub],
                                                                     optimize=optimize, **restart)
    return b.getvalue()


def _cycled(images):
    """(name, bytes) per image x quality x subsampling; ``optimize`` and the restart setting cycle with the running index
    so that every value of each meets every subsampling and quality."""
    out, n = [], 0
    for kind, h, w, c in images:
        for q in QUALITIES:
            for sub in (SUBS if c == 3 else ("444",)):
                opt, restart = bool(n % 2), RESTARTS[(n // 2) % 4]
                n += 1
                name = "%s-%dx%dx%d-q%d-%s-%s-%s" % (kind, h, w, c, q, sub, "opt" if opt else "std",
                                                       "+".join("%s%d" % (k[15:], v) for k, v in restart.items()) or "norst")
                out.append((name, pil_file(jm.make_image(kind, h, w, c), q, sub, opt, **restart)))
    return out


@functools.lru_cache(maxsize=None)
def host_corpus():
    """test_jpeg_host.py's images through PIL, a case with more than 8 restart intervals, and ``jpeg_model.write``'s files."""
    from test_jpeg_host import IMAGES

    files = _cycled(IMAGES)
    files.append(("noise-136x24x3-q90-444-rows", pil_file(jm.make_image("noise", 136, 24, 3), 90, "444", restart_marker_rows=1)))
    for kind, h, w, c, q, sub in (("noise", 33, 41, 3, 90, "420"), ("sinusoid", 33, 41, 3, 100, "444"),
                                  ("checker", 24, 17, 1, 100, "444"), ("ripple77", 24, 17, 1, 25, "444")):
        coef, _ = jm.transform(jm.make_image(kind, h, w, c), q, sub)
        files.append(("model-%s-%dx%dx%d-q%d-%s" % (kind, h, w, c, q, sub), jm.write(coef, h, w, c, q, sub)))
    return tuple(files)


SMALL = (1, 7, 8, 9, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def gpu_sizes_corpus():
    """H, W in SMALL x SMALL plus three long shapes, contents cycling, everything else cycling as in ``host_corpus``."""
    shapes = [(h, w) for h in SMALL for w in SMALL] + [(136, 24), (16, 640), (8, 4096)]
    images = [(jm.CONTENTS[i % len(jm.CONTENTS)], h, w, 1 if i % 5 == 4 else 3) for i, (h, w) in enumerate(shapes)]
    out, n = [], 0
    for kind, h, w, c in images:
        q, sub = QUALITIES[n % 3], (list(SUBS)[(n // 3) % 3] if c == 3 else "444")
        opt, restart = bool((n // 2) % 2), RESTARTS[(n // 4) % 4]
        n += 1
        out.append(("%s-%dx%dx%d-q%d-%s-%d-%s" % (kind, h, w, c, q, sub, opt, sorted(restart)),
                    pil_file(jm.make_image(kind, h, w, c), q, sub, opt, **restart)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def big_file():
    """The smallest case whose scan spans many workgroups' worth of subsequences."""
    return pil_file(jm.make_image("noise", 600, 900, 3), 90, "420")


_MODEL = {}


def model(data):
    """``jpeg_decode_model.read`` of a file, computed once."""
    if data not in _MODEL:
        _MODEL[data] = dm.read(data)
    return _MODEL[data]


@functools.lru_cache(maxsize=None)
def broken_files():
    """One file cut at 5 points (inside the headers, inside the scan, before EOI) and with one scan byte changed at 20 seeded
    positions: (name, bytes)."""
    data = pil_file(jm.make_image("sinusoid", 33, 41, 3), 90, "420", restart_marker_blocks=3)
    r = model(data)
    s0, s1 = r["scan_offset"], r["scan_offset"] + r["scan_bytes"]
    out = [("cut@%d" % at, data[:at]) for at in (30, s0 - 5, s0 + 7, (s0 + s1) // 2, len(data) - 2)]
    rng = np.random.RandomState(20)
    for at in sorted(rng.choice(np.arange(s0, s1), size=20, replace=False).tolist()):
        changed = bytearray(data)
        changed[at] ^= int(rng.randint(1, 256))
        out.append(("changed@%d" % at, bytes(changed)))
    return tuple(out)


def unsupported_files():
    img = jm.make_image("sinusoid", 33, 41, 3)

    def save(im, **kw):
        b = io.BytesIO()
        im.save(b, "JPEG", **kw)
        return b.getvalue()

    two_by_two_chroma = bytearray(pil_file(img, 90, "444"))
    at = two_by_two_chroma.index(b"\xff\xc0")
    two_by_two_chroma[at + 4 + 6 + 3 + 1] = 0x22                      # SOF0: the second component's sampling factors
    return (("progressive", save(Image.fromarray(img), quality=90, progressive=True)),
            ("cmyk", save(Image.fromarray(img).convert("CMYK"), quality=90)),
            ("chroma-2x2", bytes(two_by_two_chroma)))


# ---- the host entry points ---------------------------------------------------------------------------------------------
def parse_host(data):
    """-> (descriptor, status, reason)."""
    lib = _lib.load()
    d, status = _lib.JpegDesc(), C.c_int32(-1)
    buf = np.frombuffer(data, dtype=np.uint8).copy()                   # exactly len(data) bytes: nothing behind them to read
    _lib.check(lib.cgan_jpeg_parse_host(buf.ctypes.data, len(data), C.addressof(d), C.addressof(status)), "cgan_jpeg_parse_host")
    return d, status.value, (lib.cgan_last_error().decode() if status.value else "")


def blocks_of(d):
    mx, my = -(-d.width // (8 * d.hs)), -(-d.height // (8 * d.vs))
    return mx * my * (d.hs * d.vs + (2 if d.ncomp == 3 else 0))


def decode_host(data, d, subseq=0, round_cap=0):
    """-> (coefficients, status, rounds)."""
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    coef = np.full(64 * blocks_of(d), 0x5555, dtype=np.int16)
    rounds, status = C.c_int32(0), C.c_int32(-1)
    _lib.check(lib.cgan_jpeg_decode_coefficients_host(buf.ctypes.data, len(data), C.addressof(d), subseq, round_cap,
                                                      coef.ctypes.data, coef.size, C.addressof(rounds), C.addressof(status)),
               "cgan_jpeg_decode_coefficients_host")
    return coef, status.value, rounds.value


def codes_of_hufftab(t):
    """A cgan_jpeg_hufftab back to {symbol: (code, length)}: what the decode form says, for the comparison with the DHT."""
    out, prev = {}, 0
    for length in range(1, 17):
        first, end = prev >> (16 - length), t.limit[length] >> (16 - length)
        for code in range(first, end):
            out[t.vals[(code + t.offset[length]) & 255]] = (code, length)
        prev = t.limit[length]
    return out
