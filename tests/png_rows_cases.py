"""Row-framed PNG files for test_png_rows_host.py, test_gpu_png_rows.py and tools/png_rows_asan.cpp's input:
files with one IDAT chunk per row from ``zlib.compressobj`` with a Z_FULL_FLUSH behind every row and from the model's deflate
writer, candidates the row path must refuse (the serial path then decodes them exactly), broken candidates, and the ctypes
calls of the new host entry points.  Everything is made here, deterministically; the files of the device encoder are made in
the GPU tests.  ``png_decode_model`` and ``png_decode_corpus`` are imported, not changed."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

import jpeg_model as jm
import png_decode_corpus as pc
import png_decode_model as pm
from climategan_amd import _lib

SERIAL, ROWS, REFUSED = 0, 1, 2
MODES = ("L", "RGB", "RGBA", "I;16")
WRITERS = (("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED))
TOKEN_LIMIT = 48 * 1024         # the pure-Python inflate (tokens, blocks) runs on files that inflate to no more than this


def image(kind, h, w, mode):
    return pc.as_mode(jm.make_image(kind, h, w, 3 if mode in ("RGB", "RGBA") else 1), mode)


def row_parts(raw, row_len, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=zlib.Z_FULL_FLUSH):
    """The filtered bytes -> the zlib stream in H + 1 parts: row k compressed and flushed (part 0 begins with the zlib header),
    and the tail (the final block and the Adler-32)."""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    parts = [co.compress(raw[at:at + row_len]) + co.flush(flush) for at in range(0, len(raw), row_len)]
    return parts + [co.flush()]


def framed(img, parts):
    """One IDAT chunk per part."""
    return pm.frame(img, b"".join(parts), idat=[len(p) for p in parts])


def flushed_file(img, filters=(0, 1, 2, 3, 4), **kw):
    px, bpp, _, _ = pm.image_bytes(img)
    return framed(img, row_parts(pm.filter_rows(px, bpp, filters), 1 + px.shape[1], **kw))


def _zlib_files():
    out, n = [], 0
    for h in (1, 2, 65):
        for w in (1, 7, 86, 640):
            for mode in MODES:
                name, level, strategy = WRITERS[n % 3]
                kind = jm.CONTENTS[n % len(jm.CONTENTS)]
                n += 1
                out.append(("zlib-%s-%dx%d-%s-%s" % (kind, h, w, mode, name),
                            flushed_file(image(kind, h, w, mode), level=level, strategy=strategy)))
    out.append(("zlib-sinusoid-3x4096-RGB-l1", flushed_file(image("sinusoid", 3, 4096, "RGB"), level=1)))     # the encoder's widest row
    out.append(("zlib-noise-2x8192-RGBA-l1", flushed_file(image("noise", 2, 8192, "RGBA"), level=1)))       # a row of 32 769 bytes
    return out


def _blocks(blocks, first=False):
    """Hand-built blocks (as ``pm.zlib_stream`` takes them, none final) -> their bytes; they must end on a byte, as a stored
    block does.  first: with the zlib header in front."""
    bw = pm.BitWriter()
    if first:
        bw.bits(0x78, 8)
        bw.bits(0x01, 8)
    for blk in blocks:
        if blk[0] == "stored":
            bw.bits(0, 3)
            bw.align()
            bw.bits(len(blk[1]), 16)
            bw.bits(len(blk[1]) ^ 0xFFFF, 16)
            bw.out += blk[1]
        elif blk[0] == "fixed":
            bw.bits(0, 1)
            bw.bits(1, 2)
            pm.put_tokens(bw, blk[1], pm.FIXED_LIT, pm.FIXED_DIST)
        else:
            pm.put_dynamic_header(bw, 0, blk[2], blk[3])
            pm.put_tokens(bw, blk[1], blk[2], blk[3])
    assert blocks[-1][0] == "stored" and bw.n == 0
    return bytes(bw.out)


def _hand_file():
    """6 x 640 grey, every row filter 0, each row coded its own way by the model's deflate writer."""
    h, w = 6, 640
    px = jm.make_image("noise", h, w, 1).reshape(h, w).copy()
    px[1, :] = 7                                          # a run: matches of 258 bytes at distance 1
    px[2, :] = np.tile(np.array([3, 200], dtype=np.uint8), w // 2)      # a repeat of two bytes
    raw = pm.filter_rows(px, 1, (0,))
    rows = [raw[k * (w + 1):(k + 1) * (w + 1)] for k in range(h)]
    lits = [[("lit", v) for v in r] for r in rows]
    dyn_lit, dyn_dist = [8] * 255 + [9, 9], [1, 1]
    parts = [
        # several blocks: fixed, then dynamic, then the empty stored block
        _blocks([("fixed", lits[0][:300]), ("dynamic", lits[0][300:], dyn_lit, dyn_dist), ("stored", b"")], first=True),
        _blocks([("fixed", lits[1][:2] + [("match", 258, 1), ("match", 258, 1), ("match", 123, 1)]), ("stored", b"")]),
        _blocks([("fixed", lits[2][:3] + [("match", 200, 2), ("match", 258, 2), ("match", 180, 2)]), ("stored", b"")]),
        # the last stored block carries bytes
        _blocks([("fixed", lits[3][:100]), ("stored", rows[3][100:])]),
        # stored blocks only, one of them empty in the middle
        _blocks([("stored", rows[4][:11]), ("stored", b""), ("stored", rows[4][11:])]),
        _blocks([("dynamic", lits[5], dyn_lit, dyn_dist), ("fixed", []), ("stored", b"")]),
        b"\x03\x00" + struct.pack(">I", zlib.adler32(raw))]
    return framed(px.reshape(h, w, 1), parts)


@functools.lru_cache(maxsize=None)
def framed_files():
    """Files every row of which satisfies the row rule: the row path decodes them (path 1)."""
    return tuple(_zlib_files() + [("hand-6x640-L", _hand_file())])


def _identical_rows():
    row = jm.make_image("noise", 1, 86, 3)
    return np.repeat(row, 5, axis=0)


@functools.lru_cache(maxsize=None)
def refused_files():
    """Candidates by their chunks whose streams break the row rule: the row path refuses them, the serial path decodes them."""
    same = _identical_rows()
    px, bpp, _, _ = pm.image_bytes(same)
    sync = framed(same, row_parts(pm.filter_rows(px, bpp, (0,)), 1 + px.shape[1], flush=zlib.Z_SYNC_FLUSH))
    img = image("sinusoid", 5, 86, "RGB")
    stream = pm.read(pc.pil_file(img))["stream"]
    assert len(stream) > 40
    cut = pm.frame(img, stream, idat=[5, 9, 1, 13, 2])                     # five chunks and the rest: H + 1
    px, bpp, _, _ = pm.image_bytes(img)
    p = row_parts(pm.filter_rows(px, bpp, (0, 1, 2, 3, 4)), 1 + px.shape[1])
    half = len(p[3]) // 2
    shifted = framed(img, [p[0] + p[1], p[2], p[3][:half], p[3][half:], p[4], p[5]])
    return (("sync-flush-identical-rows", sync), ("pil-stream-cut-into-chunks", cut), ("full-flush-shifted-chunks", shifted))


def broken_base():
    return flushed_file(image("sinusoid", 5, 86, "RGB"), level=6)


@functools.lru_cache(maxsize=None)
def broken_files():
    """A framed file with one thing wrong: (name, bytes)."""
    data = broken_base()
    idats = [(p, off) for k, p, off in pm.chunks(data) if k == b"IDAT"]

    def changed(chunk, at, fn):
        b = bytearray(data)
        off = idats[chunk][1] + (at if at >= 0 else len(idats[chunk][0]) + at)
        b[off] = fn(b[off])
        return bytes(b)                                    # the IDAT CRC is now wrong, which nobody looks at (4.21)

    return (("changed-byte-in-row-2", changed(2, len(idats[2][0]) // 2, lambda v: v ^ 0x55)),
            ("wrong-adler", changed(5, -1, lambda v: v ^ 1)),
            ("bfinal-in-row-3", changed(3, 0, lambda v: v | 1)))


_MODEL = {}


def model(data):
    """``png_decode_model.read`` of a file, once; with tokens and blocks where the file is small enough."""
    if data not in _MODEL:
        r = pm.read(data)
        if len(r["inflated"]) <= TOKEN_LIMIT:
            r = pm.read(data, tokens=True)
        _MODEL[data] = r
    return _MODEL[data]


def idat_lengths(data):
    return [len(p) for k, p, _ in pm.chunks(data) if k == b"IDAT"]


def expected_table(data):
    """What cgan_png_row_table_host must give: the chunks' cumulative lengths, row 0 behind the zlib header."""
    n = idat_lengths(data)
    return [2] + np.cumsum(n[:-1]).tolist()


def tokens_by_row(r):
    """The model's tokens row by row: [(tokens of the row, [(token, the row's bytes before it)])] -- a token never crosses a row
    in a file that satisfies the row rule."""
    row_len = len(r["inflated"]) // r["h"]
    rows, at = [[] for _ in range(r["h"] + 1)], 0
    for t in r["tokens"]:
        n = 1 if t[0] == "lit" else t[1]
        rows[min(at // row_len, r["h"])].append((t, at % row_len))
        at += n
    return rows


def blocks_by_row(r, table):
    """The model's block kinds per chunk."""
    edges = [8 * v for v in table] + [8 * len(r["stream"])]
    out = [[] for _ in table]
    for b in r["blocks"]:
        k = max(i for i in range(len(table)) if edges[i] <= b["start"])
        out[k].append(b["kind"])
    return out


# ---- the host entry points ---------------------------------------------------------------------------------------------
def row_table_host(data, d):
    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    table = np.full(d.rows + 1, 0x55555555, dtype=np.uint32)
    _lib.check(lib.cgan_png_row_table_host(buf.ctypes.data, len(data), C.addressof(d), table.ctypes.data), "cgan_png_row_table_host")
    return table


def decode_rows_host(data):
    """The row twin on a file -> (pixels as the model shapes them, status, path, descriptor, table or None)."""
    lib = _lib.load()
    d, status, why = pc.parse_host(data)
    assert status == pc.OK, why
    stream = np.frombuffer(pc.stream_host(data, d), dtype=np.uint8).copy()
    table = row_table_host(data, d) if d.rows else None
    bpp = d.channels * d.bit_depth // 8
    inflated = np.full(d.height * (1 + d.width * bpp), 0x55, dtype=np.uint8)
    pixels = np.full(d.height * d.width * bpp, 0x55, dtype=np.uint8)
    status, path = C.c_int32(-1), C.c_int32(-1)
    _lib.check(lib.cgan_png_decode_rows_host(stream.ctypes.data, C.addressof(d), table.ctypes.data if d.rows else None,
                                             inflated.ctypes.data, pixels.ctypes.data, C.addressof(status), C.addressof(path)),
               "cgan_png_decode_rows_host")
    px = pixels.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else pixels.reshape(d.height, d.width, d.channels)
    return px, status.value, path.value, d, table


def serial_status(data):
    d, status, why = pc.parse_host(data)
    assert status == pc.OK, why
    return pc.decode_host(pc.stream_host(data, d), d)[2]
