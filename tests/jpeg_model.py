"""Host model of the device JPEG encoder (csrc/jpeg.hip): numpy and pure Python, no library of the project.

``transform``  pixels -> quantised coefficients in float64 (and the unrounded quotients)
``write``      coefficients -> the complete file: the entropy coder and the container
``read``       a baseline file -> its segments, tables and coefficients (markers, DQT, DHT, DRI, un-stuffing, Huffman decode)

Coefficient layout (``cgan_jpeg_coefficients_u8``): the components Y, Cb, Cr one after the other; each its 8 x 8 blocks in
raster order over the frame padded to whole MCUs; each block 64 values in natural (row-major) order.
"""
import numpy as np

# ITU-T T.81 Annex K.1 / K.2, natural order
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return order


ZIGZAG = _zigzag()            # scan position -> natural index
assert ZIGZAG[:10] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and ZIGZAG[-3:] == [55, 62, 63]

# Annex K.3: the number of codes of each length 1 .. 16, the symbols in code order
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8"
    "a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
# (class << 4 | identifier) -> (bits[16], symbols), in the order the DHT segments are written
HUFFMAN = [
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(_AC_LUMA_VALS)),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(_AC_CHROMA_VALS)),
]
assert all(sum(b) == len(v) for _, b, v in HUFFMAN) and len(_AC_LUMA_VALS) == len(_AC_CHROMA_VALS) == 162


def quant_tables(quality):
    """The two Annex K tables under libjpeg's quality rule, natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (BASE_LUMA, BASE_CHROMA))


def codes_of(bits, vals):
    """symbol -> (code, length) of a table given as in a DHT segment (Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


class Geometry:
    def __init__(self, h, w, c, subsampling):
        self.h, self.w, self.c = h, w, c
        self.v = 2 if (c == 3 and str(subsampling) == "420") else 1
        self.mcu = 8 * self.v
        self.mcus_x, self.mcus_y = -(-w // self.mcu), -(-h // self.mcu)
        # per component: (block rows, block columns)
        self.shapes = [(self.mcus_y * self.v, self.mcus_x * self.v)] + [(self.mcus_y, self.mcus_x)] * (c - 1)
        self.blocks = sum(a * b for a, b in self.shapes)

    def split(self, flat):
        """flat [blocks * 64] -> one [rows, cols, 64] view per component."""
        flat = np.asarray(flat).reshape(self.blocks, 64)
        out, at = [], 0
        for a, b in self.shapes:
            out.append(flat[at:at + a * b].reshape(a, b, 64))
            at += a * b
        return out

    def mcu_blocks(self, my, mx):
        """(component, block row, block column) of the MCU's blocks in scan order."""
        out = [(0, my * self.v + i, mx * self.v + j) for i in range(self.v) for j in range(self.v)]
        return out + [(k, my, mx) for k in range(1, self.c)]


_DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
                 for u in range(8)])


def transform(img, quality, subsampling):
    """uint8 [H, W, C] -> (coefficients int16 [blocks * 64], unrounded quotients float64 [blocks * 64]); float64
    throughout, rounding to nearest (ties to even), AC clamped to +-1023."""
    img = np.asarray(img)
    h, w, c = img.shape
    g = Geometry(h, w, c, subsampling)
    ph, pw = g.mcus_y * g.mcu, g.mcus_x * g.mcu
    px = np.pad(img.astype(np.float64), ((0, ph - h), (0, pw - w), (0, 0)), mode="edge")
    if c == 1:
        planes = [px[..., 0] - 128.0]
    else:
        r, gr, b = px[..., 0], px[..., 1], px[..., 2]
        planes = [0.299 * r + 0.587 * gr + 0.114 * b - 128.0,
                  -0.168736 * r - 0.331264 * gr + 0.5 * b,
                  0.5 * r - 0.418688 * gr - 0.081312 * b]
        if g.v == 2:
            planes[1:] = [p.reshape(ph // 2, 2, pw // 2, 2).mean(axis=(1, 3)) for p in planes[1:]]
    tables = quant_tables(quality)
    quot = []
    for k, p in enumerate(planes):
        blocks = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        f = _DCT @ blocks @ _DCT.T
        quot.append((f / np.array(tables[min(k, 1)], dtype=np.float64).reshape(8, 8)).reshape(-1, 64))
    quot = np.concatenate(quot).reshape(-1)
    coef = np.rint(quot).reshape(-1, 64)
    coef[:, 1:] = np.clip(coef[:, 1:], -1023, 1023)
    return coef.astype(np.int16).reshape(-1), quot


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def headers(h, w, c, quality, subsampling):
    """SOI .. SOS, the segments in libjpeg's order."""
    g = Geometry(h, w, c, subsampling)
    tables = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if c == 3 else 1):
        out += _segment(0xDB, [t] + [tables[t][ZIGZAG[k]] for k in range(64)])
    sof = [8] + list(h.to_bytes(2, "big")) + list(w.to_bytes(2, "big")) + [c]
    for i in range(c):
        sof += [i + 1, (g.v << 4 | g.v) if i == 0 else 0x11, 0 if i == 0 else 1]
    out += _segment(0xC0, sof)
    for tc_th, bits, vals in HUFFMAN[:4 if c == 3 else 2]:
        out += _segment(0xC4, [tc_th] + bits + vals)
    out += _segment(0xDD, g.mcus_x.to_bytes(2, "big"))
    sos = [c]
    for i in range(c):
        sos += [i + 1, 0x00 if i == 0 else 0x11]
    return out + _segment(0xDA, sos + [0, 63, 0])


def _category(v):
    return int(abs(int(v))).bit_length()


def block_tokens(block, prev_dc, dc_codes, ac_codes, symbols=None):
    """The codes of one block as a list of bit strings; ``symbols`` (a list) receives ("DC" | "AC", symbol) per code."""
    out = []

    def put(kind, table, sym, value):
        code, length = table[sym]
        s = sym & 15
        extra = (value - 1 if value < 0 else value) & ((1 << s) - 1)
        out.append(format((code << s) | extra, "b").zfill(length + s))
        if symbols is not None:
            symbols.append((kind, sym))

    diff = int(block[0]) - prev_dc
    put("DC", dc_codes, _category(diff), diff)
    run = 0
    for k in range(1, 64):
        v = int(block[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            put("AC", ac_codes, 0xF0, 0)
            run -= 16
        put("AC", ac_codes, (run << 4) | _category(v), v)
        run = 0
    if run:
        put("AC", ac_codes, 0x00, 0)
    return out


def write(coef, h, w, c, quality, subsampling, symbols=None):
    """The complete file from coefficients in the layout of ``transform``."""
    g = Geometry(h, w, c, subsampling)
    comps = g.split(coef)
    tabs = [codes_of(b, v) for _, b, v in HUFFMAN]
    out = [headers(h, w, c, quality, subsampling)]
    for my in range(g.mcus_y):
        dc = [0] * c
        bits = []
        for mx in range(g.mcus_x):
            for k, by, bx in g.mcu_blocks(my, mx):
                block = comps[k][by, bx]
                bits += block_tokens(block, dc[k], tabs[2 if k else 0], tabs[3 if k else 1], symbols)
                dc[k] = int(block[0])
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        out.append(int(s, 2).to_bytes(len(s) // 8, "big").replace(b"\xff", b"\xff\x00"))
        if my + 1 < g.mcus_y:
            out.append(bytes([0xFF, 0xD0 + (my & 7)]))
    out.append(b"\xff\xd9")
    return b"".join(out)


def read(data):
    """A baseline file -> dict: h, w, c, subsampling ("444" | "420"), qtables {id: 64 values, natural order}, the payloads
    ``dqt`` / ``dht`` (lists, file order), ``sof``, ``dri``, ``sos``, ``scan`` (the bytes from the SOS marker to EOI inclusive),
    ``rst`` (the m of every RSTm met) and ``coef`` (int16, the layout of ``transform``)."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    r = {"dqt": [], "dht": [], "qtables": {}, "dri": None, "rst": []}
    huff = {}
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected at %d" % i
        marker = data[i + 1]
        length = int.from_bytes(data[i + 2:i + 4], "big")
        payload = data[i + 4:i + 2 + length]
        if marker == 0xDB:
            r["dqt"].append(payload)
            at = 0
            while at < len(payload):
                assert payload[at] >> 4 == 0, "16-bit table"
                table = [0] * 64
                for k in range(64):
                    table[ZIGZAG[k]] = payload[at + 1 + k]
                r["qtables"][payload[at] & 15] = table
                at += 65
        elif marker == 0xC4:
            r["dht"].append(payload)
            at = 0
            while at < len(payload):
                bits = list(payload[at + 1:at + 17])
                vals = list(payload[at + 17:at + 17 + sum(bits)])
                huff[payload[at]] = {format(code, "b").zfill(n): sym for sym, (code, n) in codes_of(bits, vals).items()}
                at += 17 + sum(bits)
        elif marker == 0xC0:
            r["sof"] = payload
        elif marker == 0xDD:
            r["dri"] = payload
        elif marker == 0xDA:
            r["sos"] = payload
            r["scan"] = data[i:]
            i += 2 + length
            break
        else:
            assert marker == 0xE0 or 0xE1 <= marker <= 0xEF or marker == 0xFE, "marker %02X" % marker
        i += 2 + length
    sof = r["sof"]
    assert sof[0] == 8
    h, w, c = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    sampling = [sof[6 + 3 * k + 1] for k in range(c)]
    assert sampling[0] in (0x11, 0x22) and all(s == 0x11 for s in sampling[1:])
    sub = "420" if (c == 3 and sampling[0] == 0x22) else "444"
    r.update(h=h, w=w, c=c, subsampling=sub)
    g = Geometry(h, w, c, sub)
    sos = r["sos"]
    assert sos[0] == c and tuple(sos[1 + 2 * c:]) == (0, 63, 0)
    tables = [(huff[sos[2 + 2 * k] >> 4], huff[0x10 | (sos[2 + 2 * k] & 15)]) for k in range(c)]
    interval = int.from_bytes(r["dri"], "big") if r["dri"] else 0
    # the entropy-coded intervals between the markers
    pieces, start = [], i
    while True:
        j = data.index(b"\xff", i)
        nxt = data[j + 1]
        if nxt == 0x00:
            i = j + 2
            continue
        pieces.append(data[start:j].replace(b"\xff\x00", b"\xff"))
        if nxt == 0xD9:
            assert j + 2 == len(data), "bytes behind EOI"
            break
        assert 0xD0 <= nxt <= 0xD7, "marker %02X inside the scan" % nxt
        r["rst"].append(nxt - 0xD0)
        i = start = j + 2
    flat = np.zeros((g.blocks, 64), dtype=np.int16)
    comps = g.split(flat)
    mcus = [(my, mx) for my in range(g.mcus_y) for mx in range(g.mcus_x)]
    per = interval if interval else len(mcus)
    assert len(pieces) == -(-len(mcus) // per), "%d intervals for %d MCUs of interval %d" % (len(pieces), len(mcus), per)
    for n, piece in enumerate(pieces):
        bits = format(int.from_bytes(piece, "big"), "b").zfill(8 * len(piece)) if piece else ""
        pos = 0

        def symbol(table):
            nonlocal pos
            for n_bits in range(1, 17):
                s = table.get(bits[pos:pos + n_bits])
                if s is not None and pos + n_bits <= len(bits):
                    pos += n_bits
                    return s
            raise AssertionError("no code at bit %d" % pos)

        def value(s):
            nonlocal pos
            if s == 0:
                return 0
            v = int(bits[pos:pos + s], 2)
            pos += s
            return v if v >> (s - 1) else v - (1 << s) + 1

        dc = [0] * c
        for my, mx in mcus[n * per:(n + 1) * per]:
            for k, by, bx in g.mcu_blocks(my, mx):
                block = comps[k][by, bx]
                dc[k] += value(symbol(tables[k][0]))
                block[0] = dc[k]
                at = 1
                while at < 64:
                    rs = symbol(tables[k][1])
                    if rs == 0x00:
                        break
                    at += rs >> 4
                    if rs & 15:
                        block[ZIGZAG[at]] = value(rs & 15)
                    at += 1
        assert len(bits) - pos < 8 and set(bits[pos:]) <= {"1"}, "padding of interval %d" % n
    r["coef"] = flat.reshape(-1)
    return r


# ---- the test images ---------------------------------------------------------------------------------------------------
CONTENTS = ("constant", "noise", "sinusoid", "checker", "p44", "ripple77")


def make_image(kind, h, w, c, seed=0):
    """uint8 [h, w, c].  checker: 0 / 255 per 8 x 8 block (DC differences of category 11 at quality 100); p44: the sign
    pattern of the (4, 4) basis function (an AC value of category 10 at quality 100); ripple77: 128 plus a (7, 7) basis
    function small enough that the block's only non-zero coefficient is its last (three ZRL codes in a row).  ``seed``
    varies the content within its kind: the noise, the sinusoid's phase, the constant, the two levels of checker and p44
    (seed and 255 - seed), the ripple's amplitude."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "constant":
        a = np.full((h, w, c), 77.0 + seed)
    elif kind == "noise":
        return np.random.RandomState(seed + 1000 * h + w).randint(0, 256, size=(h, w, c)).astype(np.uint8)
    elif kind == "sinusoid":
        a = np.stack([128 + 100 * np.sin(2 * np.pi * (x / 23.0 + y / 17.0) + 0.9 * k + 0.37 * seed) for k in range(c)], axis=-1)
    elif kind == "checker":
        a = np.repeat(np.where((y // 8 + x // 8) % 2, 255.0 - seed, 0.0 + seed)[..., None], c, axis=-1)
    elif kind == "p44":
        s = np.cos((2 * (x % 8) + 1) * 4 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 4 * np.pi / 16)
        a = np.repeat(np.where(s > 0, 255.0 - seed, 0.0 + seed)[..., None], c, axis=-1)
    elif kind == "ripple77":
        s = _DCT[7][x % 8] * _DCT[7][y % 8]
        a = np.repeat((128 + (400 + 7 * seed) * s)[..., None], c, axis=-1)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)
