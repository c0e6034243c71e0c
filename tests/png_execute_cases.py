"""Tiny hand-built files aimed at the execute step all inflate kernels share (csrc/png_decode.hip's ``execute_tokens``), for
test_gpu_png_execute.py: grey, 3 rows of 600 pixels, every row coded by the model's deflate writer so that its tokens meet
the step where it can go wrong.  Each file comes row-framed (one IDAT chunk per row, every row ended by a stored block) and
ordinary (the same blocks in one stream, an empty final block behind them)."""
import functools
import struct
import zlib

import png_decode_model as pm
import png_rows_cases as rc

W, H = 600, 3
ROW = 1 + W
DYN_LIT, DYN_DIST = [8] * 255 + [9, 9], [1, 1]           # literals and the end-of-block symbol alone


def _lits(row, at, n):
    """n literals for the bytes at .. at + n of row `row`; a row's first byte is its filter byte, 0."""
    return [("lit", 0 if at + k == 0 else (7 * (at + k) + 31 * row) % 251 + 1) for k in range(n)]


def _stored(row, at, n):
    return bytes(t[1] for t in _lits(row, at, n))


def _row_bytes(blocks, before=b""):
    """What a row's blocks inflate to behind the bytes `before`."""
    out = bytearray(before)
    for blk in blocks:
        if blk[0] == "stored":
            out += blk[1]
            continue
        for t in blk[1]:
            for _ in range(1 if t[0] == "lit" else t[1]):
                out.append(t[1] if t[0] == "lit" else out[-t[2]])
    row = bytes(out[len(before):])
    assert len(row) == ROW and row[0] == 0, len(row)
    return row


def _rounds_rows():
    """Row 0: 126 literals -- a second round, `pos` carried over -- then a match of 258 at distance 1 and one that reaches
    back over it: 128 tokens, so that row 1 begins a round in the whole stream too.  Row 1: a match as token 64 of a round and
    one as token 63 of the next, each reading literals of its own round, the first as a repeat.  Row 2: 70 matches in a row,
    more than a round holds."""
    row0 = [("fixed", _lits(0, 0, 126) + [("match", 258, 1), ("match", 217, 300)]), ("stored", b"")]
    row1 = [("fixed", _lits(1, 0, 63) + [("match", 50, 40)] + _lits(1, 113, 62) + [("match", 40, 60)] + _lits(1, 215, ROW - 215)),
            ("stored", b"")]
    row2 = [("fixed", _lits(2, 0, 3) + [("match", 9 if k < 38 else 8, 1 + k % 3) for k in range(70)]), ("stored", b"")]
    return [row0, row1, row2]


def _stored_rows():
    """Row 0: a stored block with bytes between two coded blocks.  Row 1: one stored block.  Row 2: stored, coded, and the
    stored block that ends the row carries bytes."""
    row0 = [("fixed", _lits(0, 0, 200)), ("stored", _stored(0, 200, 150)), ("dynamic", _lits(0, 350, 100), DYN_LIT, DYN_DIST),
            ("fixed", [("match", 151, 300)]), ("stored", b"")]
    row1 = [("stored", _stored(1, 0, ROW))]
    row2 = [("stored", _stored(2, 0, 11)), ("fixed", [("match", 258, 1), ("match", 258, 5)] + _lits(2, 527, 20)),
            ("stored", _stored(2, 547, 54))]
    return [row0, row1, row2]


def _reaching_rows():
    """Row 1 has a match whose distance reaches one byte in front of the row: valid in the stream, not inside the row."""
    rows = _rounds_rows()
    rows[1] = [("fixed", _lits(1, 0, 10) + [("match", 20, 11)] + _lits(1, 30, ROW - 30)), ("stored", b"")]
    return rows


def _files(rows):
    """The rows, each a list of blocks -> (the framed file, the ordinary file)."""
    raw = b""
    for blocks in rows:
        raw += _row_bytes(blocks, raw)
    shown = pm.unfilter(raw, H, W, 1).reshape(H, W, 1)
    parts = [rc._blocks(blocks, first=k == 0) for k, blocks in enumerate(rows)] + [b"\x03\x00" + struct.pack(">I", zlib.adler32(raw))]
    ordinary = pm.frame(shown, pm.zlib_stream([blk for blocks in rows for blk in blocks] + [("fixed", [])], raw))
    return rc.framed(shown, parts), ordinary


@functools.lru_cache(maxsize=None)
def intact():
    """((name, framed file, ordinary file), ...): every row of the framed ones satisfies the row rule."""
    return tuple((name,) + _files(rows) for name, rows in (("rounds", _rounds_rows()), ("stored", _stored_rows())))


@functools.lru_cache(maxsize=None)
def reaching_back():
    """(name, framed file): a candidate whose row 1 the row path must refuse; the whole-stream path decodes it."""
    return "match-in-front-of-row-1", _files(_reaching_rows())[0]
