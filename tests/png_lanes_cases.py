"""The files the lane-parallel inflate's tests share (test_png_lanes_host.py, test_gpu_png_lanes.py,
tools/png_lanes_asan.cpp's input): the files of ``png_decode_corpus``, hand-built files from the model's deflate writer that
put a token, a block's end or the stream's end where the window rule has a case of its own, and the broken files.  The model
of every file (``png_lanes_model.inflate_lanes``) is computed once per (subsequence bits, lane tokens) and kept; the
conditions that make a hand-built file what its name says are asserted from it in test_png_lanes_host.py."""
import ctypes as C
import functools

import numpy as np

import jpeg_model as jm
import png_decode_corpus as pc
import png_decode_model as pm
import png_lanes_model as lm
from climategan_amd import _lib

SETTINGS = ((32, 4), (64, 8))            # beside the compiled defaults
MODEL_LIMIT = 64 * 1024                  # the pure-Python window rule runs on files that inflate to no more than this


def defaults():
    bits, tokens = C.c_int32(0), C.c_int32(0)
    _lib.load().cgan_png_inflate_lanes_params(C.addressof(bits), C.addressof(tokens))
    return bits.value, tokens.value


def all_settings():
    return SETTINGS + (defaults(),)


def grey_file(raw, w, blocks):
    """A grey file of rows of 1 + w bytes around a hand-built stream of ``blocks`` that inflates to ``raw``."""
    h = len(raw) // (1 + w)
    shown = pm.unfilter(bytes(raw), h, w, 1).reshape(h, w, 1)
    return pm.frame(shown, pm.zlib_stream(blocks, bytes(raw)))


def _windows(data, S, cap):
    r = pm.read(data)
    return lm.inflate_lanes(r["stream"], S, cap, len(r["inflated"]))[3]


# ---- the hand-built files -------------------------------------------------------------------------------------------------
SKEWED = [v + 1 for v in range(14)]      # symbols 0 .. 13 in 1 .. 14 bits; two more symbols of 15 bits complete the code


def long_token_file():
    """A token of 48 bits: length symbol 284 in 15 bits + 5 extra bits, distance symbol 29 in 15 bits + 13 extra bits.  At
    subsequences of 32 bits it begins in the upper half of one lane's bits and runs through the whole of the next lane's,
    which then has nothing to begin.  Literal v has v + 1 bits, so two literals in front of the token place it."""
    w, h = 127, 200
    size = (1 + w) * h
    first = bytes([0] + [((7 * k) % 13) + 1 for k in range(99)] + [0] * 29)   # the first row, something to read, and one zero
    lit = SKEWED + [0] * 242 + [15] + [0] * 27 + [15]                         # end-of-block and 284 in 15 bits
    dist = SKEWED + [0] * 14 + [15, 15]                                       # 28 and 29 in 15 bits
    for v in range(1, 14):
        tokens, at = [("lit", b) for b in first], len(first)
        while at < 24800:                                                     # zeros by the shortest way: 21 bits for 257 bytes
            tokens.append(("match", 257, 1))
            at += 257
        assert at % (1 + w) not in (0, 1)                                     # no filter byte among the two literals
        tokens += [("lit", v), ("lit", v - 1), ("lit", 0), ("match", 227, 24577)]
        at += 3 + 227
        while at + 257 <= size:
            tokens.append(("match", 257, 1))
            at += 257
        tokens += [("lit", 0)] * (size - at)
        raw = bytearray()
        for t in tokens:
            for _ in range(1 if t[0] == "lit" else t[1]):
                raw.append(t[1] if t[0] == "lit" else raw[-t[2]])
        data = grey_file(raw, w, [("dynamic", tokens, lit, dist)])
        if any(win["empty"] for win in _windows(data, 32, 4)):
            return data
    raise AssertionError("no pair of literals places the 48-bit token")


def block_kinds_file():
    """Short blocks, so that end-of-block symbols stand in the middle of windows: behind them a dynamic, a fixed and a stored
    block, twice over."""
    img = jm.make_image("sinusoid", 24, 17, 1)
    raw = pm.filter_rows(img.reshape(24, 17), 1, (0, 2))
    lit = [8] * 255 + [9, 9]
    blocks, at = [], 0
    for k, n in enumerate((40, 37, 30, 25, 41, 33, 28, 50)):
        piece = raw[at:at + n]
        at += n
        tokens = [("lit", v) for v in piece]
        blocks.append((("fixed", tokens), ("dynamic", tokens, lit, [1, 1]), ("fixed", tokens), ("stored", piece))[k % 4])
    blocks.append(("fixed", [("lit", v) for v in raw[at:]]))
    return pm.frame(img, pm.zlib_stream(blocks, raw))


@functools.lru_cache(maxsize=None)
def final_block_files():
    """One fixed block of literals in one row: its end-of-block symbol begins in lane 0 of a window, in lane 63, and ends
    exactly where a lane's bits end (all three at subsequences of 32 bits).  The number of 8-bit and of 9-bit literals is
    searched until the model says so."""
    found = {}
    for nine in range(0, 9):
        for w in range(250, 520):
            raw = bytes([0] + [200] * nine + [((5 * k) % 140) + 1 for k in range(w - nine)])
            data = grey_file(raw, w, [("fixed", [("lit", v) for v in raw])])
            last = _windows(data, 32, 4)[-1]
            assert last["flag"] == lm.EOB
            if last["lanes"] == 1:
                found.setdefault("lanes-final-in-lane0", data)
            if last["lanes"] == 64:
                found.setdefault("lanes-final-in-lane63", data)
            if last["exit"] == last["start"] + 32 * last["lanes"]:
                found.setdefault("lanes-final-on-boundary", data)
            if len(found) == 3:
                return tuple(sorted(found.items()))
    raise AssertionError("only %s found" % sorted(found))


def cap_file():
    """Literal 0 in one bit: 128 tokens in 128 bits, more than any lane's slots."""
    w, h = 127, 8
    raw = bytes((1 + w) * h)
    lit = SKEWED + [0] * 242 + [15] + [0] * 27 + [15]
    return grey_file(raw, w, [("dynamic", [("lit", 0)] * len(raw), lit, [1, 1])])


def wrong_phase_file():
    """A fixed block of bytes below 144 only: every literal has 8 bits.  The bits of literal 37 are 01010101, so a decode that
    starts 4 bits off reads the same literals and never meets the right one.  One match of 12 bits in lane 0 puts every other
    lane's own first bit 4 bits off: each pass corrects one lane, and the window needs as many passes as it has lanes."""
    w = 1100
    raw = bytes([0] + [37] * w)
    tokens = [("lit", 0), ("lit", 37), ("lit", 37), ("match", 3, 1)] + [("lit", 37)] * (w - 5)
    return grey_file(raw, w, [("fixed", tokens)])


@functools.lru_cache(maxsize=None)
def hand_built():
    return (("lanes-48-bit-token", long_token_file()), ("lanes-block-kinds", block_kinds_file())) + final_block_files() + (
        ("lanes-cap", cap_file()), ("lanes-wrong-phase", wrong_phase_file()))


@functools.lru_cache(maxsize=None)
def cases():
    """Every intact file: (name, bytes)."""
    return tuple(pc.corpus()) + hand_built()


@functools.lru_cache(maxsize=None)
def broken():
    """Every broken file, (name, bytes): each cause of CORRUPT as a stream of its own -- among them a distance in front of the
    output's start and output past the extent's end, which the commit finds, and invalid symbols, which a committed lane
    reports -- and the corpus' cut and changed streams."""
    grey = np.zeros((4, 7, 1), dtype=np.uint8)
    bad, _ = pc.corrupt_streams()
    return tuple((name, pm.frame(grey, stream)) for name, stream in bad) + tuple(pc.broken_files())


_MODEL = {}


def model(data, S, cap):
    """``png_lanes_model.inflate_lanes`` of an intact file -> (bytes, tokens, stats, windows, blocks), computed once."""
    key = (data, S, cap)
    if key not in _MODEL:
        r = pc.model(data)
        _MODEL[key] = lm.inflate_lanes(r["stream"], S, cap, len(r["inflated"]))
    return _MODEL[key]


def small(data):
    return len(pc.model(data)["inflated"]) <= MODEL_LIMIT


# ---- the host entry point ----------------------------------------------------------------------------------------------------
STATS = ("windows", "passes", "max_passes", "full_windows", "tokens")


def inflate_lanes_host(stream, d, S, cap):
    """The twin on a zlib stream -> (inflated bytes, trailer, stats as the model names them, status, return code)."""
    lib = _lib.load()
    bpp = d.channels * d.bit_depth // 8
    src = np.frombuffer(stream, dtype=np.uint8).copy()
    inflated = np.full(d.height * (1 + d.width * bpp), 0x55, dtype=np.uint8)
    trailer, status, stats = C.c_uint32(0), C.c_int32(-1), (C.c_uint32 * 5)()
    rc = lib.cgan_png_inflate_lanes_host(src.ctypes.data, C.addressof(d), S, cap, inflated.ctypes.data, C.addressof(trailer), stats,
                                         C.addressof(status))
    return inflated.tobytes(), trailer.value, dict(zip(STATS, stats)), status.value, rc
