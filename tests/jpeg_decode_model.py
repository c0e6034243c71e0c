"""Host model of the device JPEG decoder (csrc/jpeg_decode.hip): numpy and pure Python, no library of the
project.

``read``         ``jpeg_model.read`` generalised: luma sampling 1x1, 2x1 (4:2:2) or 2x2, any tables, fill bytes before
                 markers, bytes behind EOI -> size, sampling, interval, tables and the coefficients
``reconstruct``  coefficients -> pixels, all integer: the definition the kernels are held to
``decode``       both

Coefficient layout: the components one after the other, each its 8 x 8 blocks in raster order over the frame padded to whole
MCUs (an MCU is hs x vs luma blocks and one block per chroma component), 64 values in natural order.

Reconstruction, the stages of libjpeg: coefficient x table entry; the 8 x 8 inverse DCT of jidctint (13-bit constants, int32,
columns first with 2 bits kept, rows descaled by 18); + 128 and clamp; chroma upsampled by the triangle filter ("fancy
upsampling": 3/4 nearest, 1/4 next nearest per halved direction, edges replicated over ceil(w / 2), ceil(h / 2); h2v2 rounds
(.. + 8) >> 4 in even and (.. + 7) >> 4 in odd columns, h2v1 (.. + 1) >> 2 and (.. + 2) >> 2; a chroma plane of at most 2
columns is replicated instead, as libjpeg does); YCbCr -> RGB in 16-bit fixed point.
"""
import numpy as np

import jpeg_model as jm

class Geometry:
    def __init__(self, h, w, c, hs, vs):
        self.h, self.w, self.c, self.hs, self.vs = h, w, c, hs, vs
        self.mcus_x, self.mcus_y = -(-w // (8 * hs)), -(-h // (8 * vs))
        self.shapes = [(self.mcus_y * vs, self.mcus_x * hs)] + [(self.mcus_y, self.mcus_x)] * (c - 1)
        self.blocks = sum(a * b for a, b in self.shapes)

    def split(self, flat):
        flat = np.asarray(flat).reshape(self.blocks, 64)
        out, at = [], 0
        for a, b in self.shapes:
            out.append(flat[at:at + a * b].reshape(a, b, 64))
            at += a * b
        return out

    def mcu_blocks(self, my, mx):
        out = [(0, my * self.vs + i, mx * self.hs + j) for i in range(self.vs) for j in range(self.hs)]
        return out + [(k, my, mx) for k in range(1, self.c)]


def read(data):
    """A baseline file -> dict: h, w, c, hs, vs, interval (0: none), qtables (per component, natural order), huff (per
    component (DC, AC), each (bits[16], symbols) as in the DHT segment), scan_offset, scan_bytes (up to EOI), rst, coef
    (int16), and the coverage figures ``stuffed`` (FF 00 pairs in the scan) and ``longest_block_bits``."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    qt, huff, interval, sof = {}, {}, 0, None
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected at %d" % i
        if data[i + 1] == 0xFF:
            i += 1
            continue
        marker = data[i + 1]
        length = int.from_bytes(data[i + 2:i + 4], "big")
        payload = data[i + 4:i + 2 + length]
        if marker == 0xDB:
            at = 0
            while at < len(payload):
                assert payload[at] >> 4 == 0, "16-bit table"
                table = [0] * 64
                for k in range(64):
                    table[jm.ZIGZAG[k]] = payload[at + 1 + k]
                qt[payload[at] & 15] = table
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(payload):
                bits = list(payload[at + 1:at + 17])
                vals = list(payload[at + 17:at + 17 + sum(bits)])
                huff[payload[at]] = (bits, vals)
                at += 17 + sum(bits)
        elif marker == 0xC0:
            sof = payload
        elif marker == 0xDD:
            interval = int.from_bytes(payload, "big")
        elif marker == 0xDA:
            sos = payload
            i += 2 + length
            break
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, "marker %02X" % marker
        i += 2 + length
    assert sof is not None and sof[0] == 8
    h, w, c = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    assert c in (1, 3)
    sampling = [sof[6 + 3 * k + 1] for k in range(c)]
    hs, vs = (1, 1) if c == 1 else (sampling[0] >> 4, sampling[0] & 15)
    assert (hs, vs) in ((1, 1), (2, 1), (2, 2)) and (c == 1 or all(s == 0x11 for s in sampling[1:]))
    g = Geometry(h, w, c, hs, vs)
    assert sos[0] == c and tuple(sos[1 + 2 * c:]) == (0, 63, 0)
    tables = [(huff[sos[2 + 2 * k] >> 4], huff[0x10 | (sos[2 + 2 * k] & 15)]) for k in range(c)]      # (bits, vals) each
    r = dict(h=h, w=w, c=c, hs=hs, vs=vs, interval=interval, qtables=[qt[sof[6 + 3 * k + 2]] for k in range(c)], huff=tables,
             scan_offset=i, rst=[], stuffed=0, longest_block_bits=0)
    pieces, start = [], i
    while True:
        j = data.index(b"\xff", i)
        nxt = data[j + 1]
        if nxt == 0x00:
            r["stuffed"] += 1
            i = j + 2
            continue
        pieces.append(data[start:j].replace(b"\xff\x00", b"\xff"))
        r["scan_bytes"] = j - r["scan_offset"]                          # final once EOI is met
        while nxt == 0xFF:
            j += 1
            nxt = data[j + 1]
        if nxt == 0xD9:
            break
        assert 0xD0 <= nxt <= 0xD7, "marker %02X inside the scan" % nxt
        r["rst"].append(nxt - 0xD0)
        i = start = j + 2
    flat = np.zeros((g.blocks, 64), dtype=np.int16)
    comps = g.split(flat)
    mcus = [(my, mx) for my in range(g.mcus_y) for mx in range(g.mcus_x)]
    per = interval if interval else len(mcus)
    assert len(pieces) == -(-len(mcus) // per), "%d intervals for %d MCUs of interval %d" % (len(pieces), len(mcus), per)
    luts = [(_lut(*dc), _lut(*ac)) for dc, ac in tables]
    for n, piece in enumerate(pieces):
        # win[p]: the 16 bits from bit p on, ones behind the piece's end
        bits = np.concatenate([np.unpackbits(np.frombuffer(piece, dtype=np.uint8)), np.ones(16, dtype=np.uint8)])
        bits = bits.astype(np.uint32)
        nbits = 8 * len(piece)
        win = np.zeros(nbits + 1, dtype=np.uint32)
        for k in range(16):
            win |= bits[k:k + nbits + 1] << (15 - k)
        win = win.tolist()
        pos = 0
        dc = [0] * c
        for my, mx in mcus[n * per:(n + 1) * per]:
            for k, by, bx in g.mcu_blocks(my, mx):
                block = comps[k][by, bx]
                begun = pos
                at = 0
                while at < 64:
                    assert pos < nbits, "interval %d ends inside a block" % n
                    e = luts[k][1 if at else 0][win[pos]]
                    assert e, "no code at bit %d" % pos
                    pos += e >> 8
                    run, size = (e & 255) >> 4, e & 15
                    if at and size == 0:
                        if run != 15:
                            assert run == 0, "EOBn"
                            break
                        at += 16
                        continue
                    at += run if at else 0
                    v = 0
                    if size:
                        assert pos + size <= nbits and at < 64
                        v = win[pos] >> (16 - size)
                        pos += size
                        v = v if v >> (size - 1) else v - (1 << size) + 1
                    if at == 0:
                        dc[k] += v
                        v = dc[k]
                    block[jm.ZIGZAG[at]] = v
                    at += 1
                r["longest_block_bits"] = max(r["longest_block_bits"], pos - begun)
        assert pos <= nbits and nbits - pos < 8 and all(bits[pos:nbits] == 1), "padding of interval %d" % n
    r["coef"] = flat.reshape(-1)
    return r


def _lut(bits, vals):
    """next 16 bits of the stream -> (code length << 8) | symbol, 0 where no code begins."""
    lut = np.zeros(65536, dtype=np.uint32)
    for sym, (code, n) in jm.codes_of(bits, vals).items():
        lut[code << (16 - n):(code + 1) << (16 - n)] = (n << 8) | sym
    return lut.tolist()


# ---- the integer reconstruction -------------------------------------------------------------------------------------------
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137,
          f1_961=16069, f2_053=16819, f2_562=20995, f3_072=25172)


def _idct8(x, shift):
    """x: int64 [..., 8] -> the 8 outputs of jidctint's one-dimensional pass, descaled by ``shift`` (values stay far inside
    int32, which is what the device computes in)."""
    f = _F
    z1 = (x[..., 2] + x[..., 6]) * f["f0_541"]
    t2, t3 = z1 - x[..., 6] * f["f1_847"], z1 + x[..., 2] * f["f0_765"]
    t0, t1 = (x[..., 0] + x[..., 4]) * 8192, (x[..., 0] - x[..., 4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * f["f1_175"]
    o0, o1, o2, o3 = o0 * f["f0_298"], o1 * f["f2_053"], o2 * f["f3_072"], o3 * f["f1_501"]
    z1, z2, z3, z4 = -z1 * f["f0_899"], -z2 * f["f2_562"], -z3 * f["f1_961"] + z5, -z4 * f["f0_390"] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    half = 1 << (shift - 1)
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(v + half) >> shift for v in out], axis=-1)


def idct_blocks(coef, table):
    """int16 [n, 64] natural order, 64 table entries -> uint8 [n, 8, 8]."""
    x = coef.astype(np.int64).reshape(-1, 8, 8) * np.asarray(table, dtype=np.int64).reshape(8, 8)
    cols = _idct8(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # along the columns
    assert np.abs(cols).max(initial=0) < 2 ** 31
    rows = _idct8(cols, 18)
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def _upsample(p, hs, vs, h, w):
    """A chroma plane (padded; true extent ceil(h / vs) x ceil(w / hs)) -> int64 [h, w]."""
    ch, cw = -(-h // vs), -(-w // hs)
    p = p[:ch, :cw].astype(np.int64)
    y, x = np.mgrid[0:h, 0:w]
    if hs == 1:
        return p[y, x]
    c = x >> 1
    if cw <= 2:
        return p[(y >> 1) if vs == 2 else y, c]
    cn = np.clip(np.where(x & 1, c + 1, c - 1), 0, cw - 1)
    if vs == 1:
        return (3 * p[y, c] + p[y, cn] + np.where(x & 1, 2, 1)) >> 2
    r = y >> 1
    rn = np.clip(np.where(y & 1, r + 1, r - 1), 0, ch - 1)
    near, far = 3 * p[r, c] + p[rn, c], 3 * p[r, cn] + p[rn, cn]
    return (3 * near + far + np.where(x & 1, 7, 8)) >> 4


def reconstruct(coef, h, w, c, hs, vs, qtables):
    """-> uint8 [h, w, c]."""
    g = Geometry(h, w, c, hs, vs)
    planes = []
    for k, blocks in enumerate(g.split(coef)):
        a, b = g.shapes[k]
        px = idct_blocks(blocks.reshape(-1, 64), qtables[k]).reshape(a, b, 8, 8)
        planes.append(px.transpose(0, 2, 1, 3).reshape(a * 8, b * 8))
    if c == 1:
        return planes[0][:h, :w, None].copy()
    y = planes[0][:h, :w].astype(np.int64)
    cb = _upsample(planes[1], hs, vs, h, w) - 128
    cr = _upsample(planes[2], hs, vs, h, w) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    gr = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, gr, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    r = read(data)
    return reconstruct(r["coef"], r["h"], r["w"], r["c"], r["hs"], r["vs"], r["qtables"])
