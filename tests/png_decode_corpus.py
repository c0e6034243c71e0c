"""The files the PNG decoder's tests share (test_png_decode_host.py, test_gpu_png_decode.py, tools/png_decode_asan.cpp's input),
and the ctypes calls of the host entry points.  Every file is made here, deterministically, by PIL, by
``png_decode_model.write`` or token by token; the model reader's result of each is computed once and kept."""
import ctypes as C
import functools
import io
import zlib

import numpy as np
from PIL import Image

import jpeg_model as jm
import png_decode_model as pm
from climategan_amd import _lib

OK, UNSUPPORTED, CORRUPT = 0, 1, 2
LEVELS = (0, 1, 6, 9)
TOKEN_LIMIT = 300 * 1024        # the pure-Python inflate runs on files that inflate to no more than this


def as_mode(img, mode):
    """A test image [h, w, c] uint8 in one of PIL's modes -> the array the file holds: [h, w, 1 | 3 | 4] uint8, [h, w, 1] uint16."""
    if mode == "RGBA":
        alpha = (img[..., :1].astype(np.int32) * 7 + 13) % 256
        return np.concatenate([img, alpha.astype(np.uint8)], axis=-1)
    if mode == "I;16":
        return (img.astype(np.uint16) * 257 + (img.astype(np.uint16) >> 3)).astype(np.uint16)
    return img


def pil_file(arr, **kw):
    b = io.BytesIO()
    Image.fromarray(arr[..., 0] if arr.shape[2] == 1 else arr).save(b, "PNG", **kw)
    return b.getvalue()


def _pil_files():
    from test_jpeg_host import IMAGES

    out, n = [], 0
    for kind, h, w, c in list(IMAGES) + [("noise", 160, 160, 3)]:
        for mode in (("RGB", "RGBA") if c == 3 else ("L", "I;16")):
            level, opt = LEVELS[n % 4], (n // 4) % 3 == 2
            if (h, w) == (160, 160):
                level, opt = 0, False                      # 77 KB of stored blocks: several blocks, several IDAT chunks
            n += 1
            arr = as_mode(jm.make_image(kind, h, w, c), mode)
            kw = {"optimize": True} if opt else {"compress_level": level}
            out.append(("pil-%s-%dx%d-%s-%s" % (kind, h, w, mode, "opt" if opt else "l%d" % level), pil_file(arr, **kw)))
    return out


def _model_files():
    img = jm.make_image("sinusoid", 33, 41, 3)
    grey = jm.make_image("noise", 24, 17, 1)
    rgba = as_mode(jm.make_image("sinusoid", 33, 41, 3), "RGBA")
    deep = as_mode(jm.make_image("sinusoid", 24, 17, 1), "I;16")
    out = [("model-filter%d" % f, pm.write(img, (f,))) for f in range(5)]
    out += [("model-filters-cycling-%s" % name, pm.write(a, (0, 1, 2, 3, 4))) for name, a in
            (("rgb", img), ("grey", grey), ("rgba", rgba), ("deep", deep))]
    out += [("model-fixed", pm.write(img, (4,), strategy=zlib.Z_FIXED)), ("model-rle", pm.write(img, (1,), strategy=zlib.Z_RLE)),
            ("model-huffman-only", pm.write(img, (2,), strategy=zlib.Z_HUFFMAN_ONLY)),
            ("model-wbits9", pm.write(rgba, (3, 4), wbits=9)),
            ("model-full-flush", pm.write(img, (0, 1, 2, 3, 4), flush_rows=5)),
            ("model-idat-1", pm.write(grey, (1, 4), idat=1)), ("model-idat-7", pm.write(img, (2, 3), idat=7)),
            ("model-idat-empty", pm.write(img, (4,), idat=[0, 5, 0, 1])),
            ("model-trns-gama", pm.write(img, (1,), extra=[(b"gAMA", (45455).to_bytes(4, "big")), (b"tRNS", bytes(6))])),
            ("model-trns-grey", pm.write(grey, (0,), extra=[(b"tRNS", bytes(2))]))]
    return out


def _hand_built():
    """Streams no compressor emits: a match at the farthest distance, a 15-bit code with a single distance code, the three
    block kinds in one file."""
    out = []
    # 9 x 4096 grey, every row filter 0; the bytes from 32768 on repeat the first 258
    rng = np.random.RandomState(7)

    def grey_rows(rows):
        raw = bytearray(pm.filter_rows(rng.randint(0, 256, size=(rows, 4096)).astype(np.uint8), 1, (0,)))
        raw[8] = 0
        return raw

    def grey_file(name, raw, blocks):
        rows = len(raw) // 4097
        shown = pm.unfilter(bytes(raw), rows, 4096, 1).reshape(rows, 4096, 1)
        out.append((name, pm.frame(shown, pm.zlib_stream(blocks, bytes(raw)))))

    raw = grey_rows(9)
    raw[32768:32768 + 258] = raw[0:258]
    tokens = [("lit", v) for v in raw[:32768]] + [("match", 258, 32768)] + [("lit", v) for v in raw[32768 + 258:]]
    grey_file("hand-far-match", raw, [("fixed", tokens)])
    # a match 32 468 back, and literals right behind it that lie 32 768 behind ... its source: whoever keeps a 32 KiB window
    # and writes those literals before the match has read loses the source (the match is the 9th of 64 tokens, they follow)
    raw = grey_rows(9)
    at = 32768 + 200
    raw[at:at + 258] = raw[at - 32468:at - 32468 + 258]
    tokens = [("lit", v) for v in raw[:at]] + [("match", 258, 32468)] + [("lit", v) for v in raw[at + 258:]]
    grey_file("hand-match-then-literals", raw, [("fixed", tokens)])
    # a stored run longer than the window, literals behind it
    raw = grey_rows(10)
    grey_file("hand-stored-then-literals", raw, [("stored", bytes(raw[:40000])), ("fixed", [("lit", v) for v in raw[40000:]])])
    # bytes 0 .. 13 have codes of 1 .. 14 bits, end-of-block and length symbol 265 (11 bytes) fifteen: a complete code;
    # one distance code of one bit
    px = np.minimum(rng.geometric(0.5, size=(7, 65, 1)) - 1, 13).astype(np.uint8)
    px[:, 40:60] = 3
    raw = pm.filter_rows(px.reshape(7, 65), 1, (0,))
    lit = [v + 1 for v in range(14)] + [0] * 242 + [15] + [0] * 8 + [15]
    tokens, at = [], 0
    while at < len(raw):
        if at >= 1 and raw[at:at + 11] == raw[at - 1:at] * 11:
            tokens.append(("match", 11, 1))
            at += 11
        else:
            tokens.append(("lit", raw[at]))
            at += 1
    assert any(t[0] == "match" for t in tokens)
    out.append(("hand-long-codes", pm.frame(px, pm.zlib_stream([("dynamic", tokens, lit, [1])], raw))))
    # stored + fixed + dynamic (literals 0 .. 254 in 8 bits, 255 and end-of-block in 9, two distance codes)
    img = jm.make_image("sinusoid", 24, 17, 1)
    raw = pm.filter_rows(img.reshape(24, 17), 1, (0, 2))
    blocks = [("stored", raw[:100]), ("fixed", [("lit", v) for v in raw[100:200]]),
              ("dynamic", [("lit", v) for v in raw[200:]], [8] * 255 + [9, 9], [1, 1])]
    out.append(("hand-three-kinds", pm.frame(img, pm.zlib_stream(blocks, raw))))
    return out


def _size_files():
    sizes = (1, 2, 7, 64, 65, 129)
    shapes = [(h, w) for h in sizes for w in sizes] + [(136, 24), (8, 4096)]
    modes = ("RGB", "L", "RGBA", "I;16")
    out = []
    for i, (h, w) in enumerate(shapes):
        mode = modes[i % 4]
        kind = jm.CONTENTS[i % len(jm.CONTENTS)]
        arr = as_mode(jm.make_image(kind, h, w, 3 if mode in ("RGB", "RGBA") else 1), mode)
        filters = ((0, 1, 2, 3, 4), (4,), (3,), (4, 3, 1), (2, 4))[i % 5]
        out.append(("size-%s-%dx%d-%s-f%s" % (kind, h, w, mode, "".join(map(str, filters))), pm.write(arr, filters, level=LEVELS[1 + i % 3])))
    return out


@functools.lru_cache(maxsize=None)
def big_file():
    """600 x 900 RGB noise: a stream of many blocks."""
    return pil_file(jm.make_image("noise", 600, 900, 3))


@functools.lru_cache(maxsize=None)
def corpus():
    return tuple(_pil_files() + _model_files() + _hand_built() + _size_files() + [("pil-noise-600x900-RGB", big_file())])


_MODEL = {}


def model(data):
    """``png_decode_model.read`` of a file, computed once; with the tokens where the file is small enough."""
    if data not in _MODEL:
        r = pm.read(data)
        if len(r["inflated"]) <= TOKEN_LIMIT:
            r = pm.read(data, tokens=True)
        _MODEL[data] = r
    return _MODEL[data]


def reframed(data, stream):
    """The file with its IDAT chunks replaced by one that holds ``stream``."""
    cs = pm.chunks(data)
    head = [c for c in cs if c[0] not in (b"IDAT", b"IEND")]
    return pm.SIGNATURE + b"".join(pm.chunk(k, p) for k, p, _ in head) + pm.chunk(b"IDAT", stream) + pm.chunk(b"IEND", b"")


def broken_base():
    return pm.write(jm.make_image("sinusoid", 33, 41, 3), (0, 1, 2, 3, 4), level=6)


CHANGED_SEED = 20


@functools.lru_cache(maxsize=None)
def broken_files():
    """One file's zlib stream cut at 5 points and re-framed as a valid chunk, and with one stream byte changed at 20 seeded
    positions: (name, bytes).  PIL refuses every one of them (test_png_decode_host.py asserts it)."""
    data = broken_base()
    stream = model(data)["stream"]
    n = len(stream)
    out = [("cut@%d" % at, reframed(data, stream[:at])) for at in (2, 9, n // 4, n // 2, n - 9)]
    rng = np.random.RandomState(CHANGED_SEED)
    for at in sorted(rng.choice(np.arange(2, n - 4), size=20, replace=False).tolist()):
        changed = bytearray(stream)
        changed[at] ^= int(rng.randint(1, 256))
        out.append(("changed@%d" % at, reframed(data, bytes(changed))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def corrupt_streams():
    """Every cause of CORRUPT in DESIGN 4.21's list as a hand-built zlib stream of a 4 x 7 grey image: (name, stream)."""
    raw = pm.filter_rows(jm.make_image("noise", 4, 7, 1).reshape(4, 7), 1, (0,))
    lits = [("lit", v) for v in raw]
    good_lit = [8] * 255 + [9, 9]

    def header(lit=None, dist=None, **kw):
        return ("raw", lambda bw, last: pm.put_dynamic_header(bw, last, lit, dist, **kw))

    def open_block(bw, last):
        bw.bits(0, 1)
        bw.bits(1, 2)
        pm.put_tokens(bw, lits, pm.FIXED_LIT, pm.FIXED_DIST)

    bad_filter = bytearray(raw)
    bad_filter[8] = 5
    s = pm.zlib_stream
    out = [("block-type-3", s([("raw", lambda bw, last: (bw.bits(last, 1), bw.bits(3, 2)))], raw)),
           ("len-nlen", s([("raw", lambda bw, last: (bw.bits(last, 1), bw.bits(0, 2), bw.align(), bw.bits(32, 16), bw.bits(32, 16),
                                                     bw.out.extend(raw)))], raw)),
           ("cl-over-subscribed", s([header(cl=[4] * 16 + [0, 5, 5], symbols=[], hlit=257, hdist=1)], raw)),
           ("cl-incomplete", s([header(cl=[1] + [0] * 18, symbols=[], hlit=257, hdist=1)], raw)),
           ("lit-over-subscribed", s([header([1, 1, 1] + [0] * 253 + [1], [1, 1])], raw)),
           ("lit-incomplete", s([header([2, 2] + [0] * 254 + [2], [1, 1])], raw)),
           ("dist-over-subscribed", s([header(good_lit, [1, 1, 1])], raw)),
           ("dist-incomplete", s([header(good_lit, [2, 2])], raw)),
           ("dist-single-two-bits", s([header(good_lit, [2])], raw)),
           ("repeat-nothing", s([header(symbols=[(16, 0)], hlit=257, hdist=1)], raw)),
           ("repeat-overrun", s([header(symbols=[(18, 127), (18, 127)], hlit=257, hdist=1)], raw)),
           ("no-end-of-block", s([header([8] * 256 + [0], [1, 1])], raw)),
           ("literal-286", s([("fixed", lits[:5] + [("sym", 286)])], raw)),
           ("literal-287", s([("fixed", lits[:5] + [("sym", 287)])], raw)),
           ("distance-30", s([("fixed", lits[:5] + [("dsym", 3, 30)])], raw)),
           ("distance-31", s([("fixed", lits[:5] + [("dsym", 3, 31)])], raw)),
           ("distance-too-far", s([("fixed", lits[:2] + [("match", 3, 3)])], raw)),
           ("too-much-output", s([("fixed", lits + [("lit", 0)])], raw + b"\0")),
           ("too-much-output-match", s([("fixed", lits + [("match", 258, 1)])], raw + raw[-1:] * 258)),
           ("too-little-output", s([("fixed", lits[:-1])], raw[:-1])),
           ("no-final-block", s([("raw", open_block)], raw)[:-4]),
           ("adler", s([("fixed", lits)], raw, adler=zlib.adler32(raw) ^ 0x10000)),
           ("filter-byte-5", s([("fixed", [("lit", v) for v in bad_filter])], bytes(bad_filter)))]
    return tuple(out), s([("fixed", lits)], raw)


def interlaced_file():
    return pm.write_interlaced(jm.make_image("sinusoid", 33, 41, 3))


@functools.lru_cache(maxsize=None)
def unsupported_files():
    img = jm.make_image("sinusoid", 33, 41, 3)
    grey = img[..., :1]
    good = pm.read(pm.write(img))["stream"]

    def save(im, **kw):
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        return b.getvalue()

    return (("interlaced", interlaced_file()),
            ("palette", save(Image.fromarray(img).convert("P"))),
            ("grey-alpha", save(Image.fromarray(grey[..., 0]).convert("LA"))),
            ("depth-1", save(Image.fromarray(grey[..., 0] > 128))),
            ("depth-2", pm.frame(grey, good, depth=2)),
            ("depth-4", pm.frame(grey, good, depth=4)),
            ("rgb-16", pm.frame(img, good, depth=16)),
            ("apng", pm.write(img, extra=[(b"acTL", bytes(8))])),
            ("wide", pm.frame(img, good, size=(33, 8193))),
            ("high", pm.frame(img, good, size=(8193, 41))),
            ("jpeg", save_jpeg(img)),
            ("empty", b""))


def save_jpeg(img):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG")
    return b.getvalue()


# ---- the host entry points ---------------------------------------------------------------------------------------------
def parse_host(data):
    """-> (descriptor, status, reason)."""
    lib = _lib.load()
    d, status = _lib.PngDesc(), C.c_int32(-1)
    buf = np.frombuffer(data + b"\0", dtype=np.uint8)[:len(data)].copy()                # exactly len(data) bytes
    _lib.check(lib.cgan_png_parse_host(buf.ctypes.data, len(data), C.addressof(d), C.addressof(status)), "cgan_png_parse_host")
    return d, status.value, (lib.cgan_last_error().decode() if status.value else "")


def stream_host(data, d):
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    dst = np.full(d.stream_bytes, 0x55, dtype=np.uint8)
    _lib.check(lib.cgan_png_stream_host(buf.ctypes.data, len(data), C.addressof(d), dst.ctypes.data, dst.size), "cgan_png_stream_host")
    return dst.tobytes()


def decode_host(stream, d):
    """The twin on a zlib stream -> (inflated bytes, pixels as the model shapes them, status, reason)."""
    lib = _lib.load()
    bpp = d.channels * d.bit_depth // 8
    src = np.frombuffer(stream, dtype=np.uint8).copy()
    inflated = np.full(d.height * (1 + d.width * bpp), 0x55, dtype=np.uint8)
    pixels = np.full(d.height * d.width * bpp, 0x55, dtype=np.uint8)
    status = C.c_int32(-1)
    _lib.check(lib.cgan_png_decode_host(src.ctypes.data, C.addressof(d), inflated.ctypes.data, pixels.ctypes.data,
                                        C.addressof(status)), "cgan_png_decode_host")
    px = pixels.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else pixels.reshape(d.height, d.width, d.channels)
    return inflated.tobytes(), px, status.value, (lib.cgan_last_error().decode() if status.value else "")


def stream_desc(stream, h, w, c=1, depth=8):
    """A descriptor for a hand-built stream."""
    d = _lib.PngDesc()
    d.width, d.height, d.channels, d.bit_depth, d.stream_bytes = w, h, c, depth, len(stream)
    return d
