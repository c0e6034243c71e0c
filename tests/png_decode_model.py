"""The PNG decoder's definition in numpy and pure Python: a chunk walker, a small inflate that also reports the
tokens and the blocks it met (checked against ``zlib.decompress`` wherever it runs), the unfilter, and the other direction
for the tests' sake: a PNG writer over ``zlib.compressobj`` that can force a filter type per row, a strategy, ``wbits``,
flush points and IDAT chunk sizes, and a deflate writer for hand-built streams (given tokens, given code lengths, or raw
bits) that no compressor emits."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 6: 4}
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ALL = [4] * 13 + [5] * 6     # a complete code-length code that has all 19 symbols


# ---- chunks ------------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def chunks(data):
    """-> [(type, payload, offset of the payload in the file)] up to and including IEND."""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind = data[at + 4:at + 8]
        assert at + 12 + n <= len(data)
        out.append((kind, data[at + 8:at + 8 + n], at + 8))
        at += 12 + n
        if kind == b"IEND":
            break
    return out


# ---- inflate -----------------------------------------------------------------------------------------------------------
class Corrupt(Exception):
    pass


def canonical_codes(lengths):
    """{symbol: (code, length)} of a canonical Huffman code, the code's first bit its most significant."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def _reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2)


def _table(lengths):
    """The next `most` bits of the stream (first bit lowest) -> (symbol, length), None where no code matches; zlib's rules."""
    left = 1
    for n in range(1, 16):
        left = (left << 1) - sum(1 for v in lengths if v == n)
        if left < 0:
            raise Corrupt("over-subscribed code")
    used = [v for v in lengths if v]
    if left > 0 and not (len(used) == 0 or used == [1]):
        raise Corrupt("incomplete code")
    most = max(used, default=1)
    table = [None] * (1 << most)
    for s, (code, n) in canonical_codes(lengths).items():
        for at in range(_reverse(code, n), 1 << most, 1 << n):
            table[at] = (s, n)
    return table, most


class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos                  # pos in bits

    def peek(self, n):
        at, sh = self.pos >> 3, self.pos & 7
        return (int.from_bytes(self.data[at:at + 4], "little") >> sh) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        if self.pos > 8 * len(self.data):
            raise Corrupt("the stream ends early")
        return v

    def symbol(self, table, most):
        e = table[self.peek(most)]
        if e is None:
            raise Corrupt("no such code")
        self.pos += e[1]
        if self.pos > 8 * len(self.data):
            raise Corrupt("the stream ends early")
        return e[0]


def inflate(stream, limit=None):
    """A zlib stream -> (bytes, tokens, blocks).  tokens: ("lit", byte), ("match", length, distance), ("stored", length);
    blocks: dicts with kind ("stored", "fixed", "dynamic"), start (the bit its header starts at), and for dynamic blocks
    longest (the longest literal/length or distance code), cl (the code-length symbols used) and ndist (distance codes
    used).  Raises ``Corrupt`` for everything DESIGN 4.21 lists."""
    if len(stream) < 2 or stream[0] & 15 != 8 or stream[0] >> 4 > 7 or stream[1] & 0x20 or (stream[0] * 256 + stream[1]) % 31:
        raise Corrupt("bad zlib header")
    b, out, tokens, blocks = _Bits(stream, 16), bytearray(), [], []
    while True:
        start = b.pos
        last, kind = b.take(1), b.take(2)
        if kind == 3:
            raise Corrupt("block type 3")
        if kind == 0:
            b.pos = (b.pos + 7) & ~7
            n, nn = b.take(16), b.take(16)
            if n ^ nn != 0xFFFF:
                raise Corrupt("LEN and NLEN disagree")
            at = b.pos >> 3
            if at + n > len(stream):
                raise Corrupt("the stream ends early")
            out += stream[at:at + n]
            b.pos += 8 * n
            tokens.append(("stored", n))
            blocks.append({"kind": "stored", "start": start})
        else:
            info = {"kind": "fixed" if kind == 1 else "dynamic", "start": start}
            if kind == 1:
                lit, dist = FIXED_LIT, FIXED_DIST[:30]
                lt, dt = _table(lit), _table(FIXED_DIST)
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise Corrupt("too many symbols")
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = b.take(3)
                if sum(1 for v in cl if v) == 0 or sum(2 ** (15 - v) for v in cl if v) != 2 ** 15:
                    raise Corrupt("the code-length code is not complete")
                ct, lens, seen = _table(cl), [], set()
                while len(lens) < hlit + hdist:
                    s = b.symbol(*ct)
                    seen.add(s)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16 and not lens:
                        raise Corrupt("nothing to repeat")
                    v, rep = (lens[-1], 3 + b.take(2)) if s == 16 else ((0, 3 + b.take(3)) if s == 17 else (0, 11 + b.take(7)))
                    if len(lens) + rep > hlit + hdist:
                        raise Corrupt("a repeat runs past the lengths")
                    lens += [v] * rep
                if lens[256] == 0:
                    raise Corrupt("no end-of-block code")
                lit, dist = lens[:hlit], lens[hlit:]
                lt, dt = _table(lit), _table(dist)
                info.update(longest=max(lit + dist), cl=seen, ndist=sum(1 for v in dist if v))
            blocks.append(info)
            while True:
                s = b.symbol(*lt)
                if s < 256:
                    out.append(s)
                    tokens.append(("lit", s))
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise Corrupt("length symbol %d" % s)
                    n = LENGTH_BASE[s - 257] + b.take(LENGTH_EXTRA[s - 257])
                    ds = b.symbol(*dt)
                    if ds > 29:
                        raise Corrupt("distance symbol %d" % ds)
                    d = DIST_BASE[ds] + b.take(DIST_EXTRA[ds])
                    if d > len(out):
                        raise Corrupt("a distance in front of the output's start")
                    for _ in range(n):
                        out.append(out[-d])
                    tokens.append(("match", n, d))
                if limit is not None and len(out) > limit:
                    raise Corrupt("more output than the image has")
        if limit is not None and len(out) > limit:
            raise Corrupt("more output than the image has")
        if last:
            break
    b.pos = (b.pos + 7) & ~7
    adler = 0
    for _ in range(4):
        adler = (adler << 8) | b.take(8)
    if limit is not None and len(out) != limit:
        raise Corrupt("less output than the image has")
    if adler != zlib.adler32(bytes(out)):
        raise Corrupt("Adler-32 mismatch")
    return bytes(out), tokens, blocks


# ---- filters -----------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, h, row_bytes, bpp):
    """The inflated bytes (a filter byte and row_bytes bytes per row) -> uint8 [h, row_bytes]."""
    if len(raw) != h * (1 + row_bytes):
        raise Corrupt("%d inflated bytes, %d expected" % (len(raw), h * (1 + row_bytes)))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + row_bytes)
    out = np.zeros((h, row_bytes), dtype=np.uint8)
    up = np.zeros(row_bytes, dtype=np.uint8)
    for y in range(h):
        f, x = int(rows[y, 0]), rows[y, 1:]
        if f == 0:
            cur = x.copy()
        elif f == 1:
            cur = np.cumsum(x.reshape(-1, bpp).astype(np.uint64), axis=0).astype(np.uint8).reshape(-1)
        elif f == 2:
            cur = x + up
        elif f in (3, 4):
            xs, us, o = x.tolist(), up.tolist(), [0] * row_bytes
            for i in range(row_bytes):
                a = o[i - bpp] if i >= bpp else 0
                c = us[i - bpp] if i >= bpp else 0
                o[i] = (xs[i] + ((a + us[i]) >> 1 if f == 3 else _paeth(a, us[i], c))) & 255
            cur = np.array(o, dtype=np.uint8)
        else:
            raise Corrupt("filter byte %d" % f)
        out[y] = cur
        up = cur
    return out


def filter_rows(px, bpp, filters):
    """uint8 [h, row_bytes] -> the bytes to deflate, row y filtered with filters[y % len(filters)]."""
    h, rb = px.shape
    p = px.astype(np.int64)
    a = np.zeros_like(p)
    a[:, bpp:] = p[:, :-bpp] if rb > bpp else 0
    b = np.zeros_like(p)
    b[1:] = p[:-1]
    c = np.zeros_like(p)
    c[1:, bpp:] = p[:-1, :-bpp] if rb > bpp else 0
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    pred = [np.zeros_like(p), a, b, (a + b) >> 1, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))]
    out = bytearray()
    for y in range(h):
        f = filters[y % len(filters)]
        out.append(f)
        out += ((p[y] - pred[f][y]) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def image_bytes(img):
    """uint8 [h, w, c] or uint16 [h, w, 1] -> (uint8 [h, row_bytes] as the file orders them, bpp, colour type, bit depth)."""
    h, w, c = img.shape
    if img.dtype == np.uint16:
        assert c == 1
        return img.astype(">u2").view(np.uint8).reshape(h, 2 * w), 2, 0, 16
    assert img.dtype == np.uint8
    return img.reshape(h, w * c), c, {1: 0, 3: 2, 4: 6}[c], 8


# ---- the writers -------------------------------------------------------------------------------------------------------
def frame(img, stream, idat=None, extra=(), interlace=0, colour=None, depth=None, size=None):
    """The file around a zlib stream.  idat: None = one chunk; an int = chunks of that many bytes; a list = those sizes in
    turn, then the rest (0 gives an empty chunk).  extra: chunks [(type, payload)] between IHDR and the first IDAT."""
    h, w = img.shape[:2] if size is None else size
    _, _, ct, bd = image_bytes(img)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bd if depth is None else depth,
                                                  ct if colour is None else colour, 0, 0, interlace))
    for kind, payload in extra:
        out += chunk(kind, payload)
    sizes = [len(stream)] if idat is None else (list(idat) if isinstance(idat, (list, tuple)) else None)
    at = 0
    if sizes is None:
        for at in range(0, len(stream), idat):
            out += chunk(b"IDAT", stream[at:at + idat])
    else:
        for n in sizes:
            out += chunk(b"IDAT", stream[at:at + n])
            at += n
        if at < len(stream):
            out += chunk(b"IDAT", stream[at:])
    return out + chunk(b"IEND", b"")


def write(img, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_rows=None, mem_level=8, **framing):
    """A PNG file of ``img`` with the given filter per row (cycling).  flush_rows: a Z_FULL_FLUSH after every that many rows."""
    px, bpp, _, _ = image_bytes(img)
    raw = filter_rows(px, bpp, filters)
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    if flush_rows:
        step, stream = flush_rows * (1 + px.shape[1]), b""
        for at in range(0, len(raw), step):
            stream += co.compress(raw[at:at + step]) + co.flush(zlib.Z_FULL_FLUSH)
        stream += co.flush()
    else:
        stream = co.compress(raw) + co.flush()
    return frame(img, stream, **framing)


ADAM7 = ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1))   # y0, x0, dy, dx


def write_interlaced(img, filters=(0, 1, 2, 3, 4)):
    """An Adam7 file: what the decoder refuses and PIL reads."""
    raw = b""
    for y0, x0, dy, dx in ADAM7:
        sub = img[y0::dy, x0::dx]
        if sub.size:
            px, bpp, _, _ = image_bytes(np.ascontiguousarray(sub))
            raw += filter_rows(px, bpp, filters)
    return frame(img, zlib.compress(raw), interlace=1)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        """n bits of v, the lowest first."""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """A Huffman code, its most significant bit first."""
        self.bits(_reverse(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def put_tokens(bw, tokens, lit, dist, end=True):
    """tokens as ``inflate`` reports them (no stored ones), or ("sym", literal/length symbol) and ("dsym", length, distance
    symbol) for symbols no compressor writes; lit / dist: code lengths."""
    lc, dc = canonical_codes(lit), canonical_codes(dist)
    for t in tokens:
        if t[0] == "lit":
            bw.code(*lc[t[1]])
        elif t[0] == "sym":
            bw.code(*lc[t[1]])
        else:
            n = t[1]
            s = max(k for k in range(29) if LENGTH_BASE[k] <= n)
            bw.code(*lc[257 + s])
            bw.bits(n - LENGTH_BASE[s], LENGTH_EXTRA[s])
            if t[0] == "dsym":
                bw.code(*dc[t[2]])
                continue
            ds = max(k for k in range(30) if DIST_BASE[k] <= t[2])
            bw.code(*dc[ds])
            bw.bits(t[2] - DIST_BASE[ds], DIST_EXTRA[ds])
    if end:
        bw.code(*lc[256])


def put_dynamic_header(bw, last, lit, dist, cl=None, symbols=None, hlit=None, hdist=None):
    """BFINAL, BTYPE = 2 and the code lengths.  By default every length is sent as itself under ``CL_ALL``; ``cl`` (19
    lengths) and ``symbols`` ([(symbol, extra bits' value)]) replace that for streams that must be wrong."""
    bw.bits(last, 1)
    bw.bits(2, 2)
    hlit, hdist = hlit or len(lit), hdist or len(dist)
    if symbols is None:
        symbols = [(v, 0) for v in list(lit) + list(dist)]
    if cl is None:
        cl = CL_ALL
    codes = canonical_codes(cl)
    hclen = max(k for k in range(19) if cl[CL_ORDER[k]]) + 1
    bw.bits(hlit - 257, 5)
    bw.bits(hdist - 1, 5)
    bw.bits(max(hclen, 4) - 4, 4)
    for k in range(max(hclen, 4)):
        bw.bits(cl[CL_ORDER[k]], 3)
    for s, extra in symbols:
        bw.code(*codes[s])
        if s >= 16:
            bw.bits(extra, {16: 2, 17: 3, 18: 7}[s])


def zlib_stream(blocks, data=None, wbits=15, adler=None):
    """A zlib stream of hand-built blocks: ("stored", bytes), ("fixed", tokens), ("dynamic", tokens, lit lengths, dist
    lengths) or ("raw", function(bit writer, last)).  data: what the stream inflates to, for the Adler-32."""
    bw = BitWriter()
    cmf = 8 | ((wbits - 8) << 4)
    bw.bits(cmf, 8)
    bw.bits(31 - (cmf * 256) % 31 if (cmf * 256) % 31 else 0, 8)
    for k, blk in enumerate(blocks):
        last = int(k == len(blocks) - 1)
        if blk[0] == "stored":
            bw.bits(last, 1)
            bw.bits(0, 2)
            bw.align()
            bw.bits(len(blk[1]), 16)
            bw.bits(len(blk[1]) ^ 0xFFFF, 16)
            bw.out += blk[1]
        elif blk[0] == "fixed":
            bw.bits(last, 1)
            bw.bits(1, 2)
            put_tokens(bw, blk[1], FIXED_LIT, FIXED_DIST)
        elif blk[0] == "dynamic":
            put_dynamic_header(bw, last, blk[2], blk[3])
            put_tokens(bw, blk[1], blk[2], blk[3])
        else:
            blk[1](bw, last)
    bw.align()
    value = zlib.adler32(data) if adler is None else adler
    return bw.bytes() + struct.pack(">I", value)


# ---- the reader --------------------------------------------------------------------------------------------------------
def read(data, tokens=False):
    """A file -> dict: h, w, c, depth, stream, inflated, pixels (uint8 [h, w, c] or uint16 [h, w, 1]); with ``tokens`` the
    pure-Python inflate runs (and is held to ``zlib.decompress``) and its tokens and blocks are added."""
    cs = chunks(data)
    assert cs[0][0] == b"IHDR"
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    assert (comp, filt, interlace) == (0, 0, 0) and colour in CHANNELS and depth in (8, 16)
    c, stream = CHANNELS[colour], b"".join(p for kind, p, _ in cs if kind == b"IDAT")
    bpp = c * depth // 8
    out = {"h": h, "w": w, "c": c, "depth": depth, "stream": stream}
    if tokens:
        raw, out["tokens"], out["blocks"] = inflate(stream, h * (1 + w * bpp))
        assert raw == zlib.decompress(stream)
    else:
        try:
            raw = zlib.decompress(stream)
        except zlib.error as e:
            raise Corrupt(str(e))
    px = unfilter(raw, h, w * bpp, bpp)
    out["inflated"] = raw
    out["pixels"] = px.view(">u2").astype(np.uint16).reshape(h, w, 1) if depth == 16 else px.reshape(h, w, c)
    return out
