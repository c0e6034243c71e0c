"""The device PNG encoder (csrc/png.hip through ops.png_encode / climategan_amd.png) against independent decoders: PIL for
the pixels, zlib / struct for the container.  The encoder is never its own yardstick."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from climategan_amd import ops, png

pytestmark = pytest.mark.gpu

HEIGHTS = (1, 2, 3, 17)
WIDTHS = (1, 2, 5, 86, 87, 89, 640)      # 86 / 87 RGB pixels: 258 / 261 bytes = the longest match, and 258 + a tail below 3
RUN_LENGTHS = (2, 3, 4, 257, 258, 259, 260, 261)


def contents(h, w, c, seed):
    """The issue's list of contents for one shape -> uint8 [n, h, w, c]."""
    rng = np.random.default_rng(seed)
    L = w * c
    yy, xx, kk = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    out = [np.zeros((h, w, c)), np.full((h, w, c), 255),
           rng.integers(0, 256, (h, w, c)),               # 9-bit literals among them
           rng.integers(0, 144, (h, w, c)),               # 8-bit literals only
           (xx * 3 + kk * 40) % 256,                      # horizontal ramp
           (yy * 7 + kk) % 256 + 0 * xx,                  # vertical ramp: Up wins
           np.where(((xx // 8) + (yy // 8)) % 2 == 1, 200, 17)]
    for pos in (0, w // 2, w - 1):                        # constant rows but one pixel
        a = np.full((h, w, c), 77)
        a[:, pos, :] = np.arange(9, 9 + c)
        out.append(a)
    combos = [(n, at_end) for n in RUN_LENGTHS for at_end in (False, True)]
    for j in range(-(-len(combos) // h)):                 # every (run length, start / end) on some row
        a = rng.integers(0, 256, (h, L))
        for r in range(h):
            n, at_end = combos[(j * h + r) % len(combos)]
            n = min(n, L)
            if at_end:
                a[r, L - n:] = 50
            else:
                a[r, :n] = 50
        out.append(a.reshape(h, w, c))
    return np.stack(out).astype(np.uint8)


def decode(b, h, w, c):
    return np.asarray(Image.open(io.BytesIO(b))).reshape(h, w, c)


def chunks(b):
    """[(type, data)] of a PNG file, every CRC checked; the position behind IEND."""
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    p, out = 8, []
    while p < len(b):
        n, = struct.unpack(">I", b[p:p + 4])
        kind, data = bytes(b[p + 4:p + 8]), bytes(b[p + 8:p + 8 + n])
        crc, = struct.unpack(">I", b[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(kind + data), (kind, p)
        out.append((kind, data))
        p += 12 + n
        if kind == b"IEND":
            break
    return out, p


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("w", WIDTHS)
def test_exact_round_trip(w, c):
    for h in HEIGHTS:
        imgs = contents(h, w, c, seed=1000 * h + 10 * w + c)
        files = png.encode(torch.from_numpy(imgs).cuda())
        assert len(files) == len(imgs)
        for i, b in enumerate(files):
            assert np.array_equal(decode(b, h, w, c), imgs[i]), (h, w, c, i)


@pytest.mark.parametrize("h,w,c", [(2, 4096, 3), (2, 4096, 1), (300, 7, 3)])
def test_round_trip_at_the_limits(h, w, c):
    """The widest row (the row kernel's largest LDS request) and more rows than one tile of the offset scan."""
    rng = np.random.default_rng(w + c)
    imgs = np.stack([rng.integers(0, 256, (h, w, c)), np.full((h, w, c), 31)]).astype(np.uint8)
    files = png.encode(torch.from_numpy(imgs).cuda())
    for i, b in enumerate(files):
        assert len(b) <= ops.png_bound_bytes(h, w, c)
        assert np.array_equal(decode(b, h, w, c), imgs[i])


@pytest.mark.parametrize("h,w,c", [(1, 1, 1), (3, 87, 3), (17, 89, 3), (17, 640, 1), (2, 86, 3)])
def test_container(h, w, c):
    imgs = contents(h, w, c, seed=7)
    buf, sizes = ops.png_encode(torch.from_numpy(imgs).cuda())
    assert buf.dtype == torch.uint8 and buf.shape == (len(imgs), ops.png_bound_bytes(h, w, c)) and buf.is_cuda
    assert sizes.shape == (len(imgs),) and sizes.is_cuda
    buf, sizes = buf.cpu().numpy(), sizes.cpu().numpy()
    for i in range(len(imgs)):
        got, end = chunks(buf[i].tobytes())
        assert end == sizes[i]                            # the file's true length; what follows is not part of the result
        kinds = [k for k, _ in got]
        assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and len(kinds) >= 3
        assert all(k == b"IDAT" for k in kinds[1:-1])
        assert got[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)
        assert got[-1][1] == b""
        raw = zlib.decompress(b"".join(d for k, d in got if k == b"IDAT"))      # checks the Adler-32
        assert len(raw) == h * (1 + w * c)
        assert all(raw[r * (1 + w * c)] <= 4 for r in range(h))
        assert np.array_equal(decode(buf[i, :sizes[i]].tobytes(), h, w, c), imgs[i])


def test_really_compressed():
    """Both figures follow from the format: a row of zeros after filtering is its literals, eight matches of at most 258
    bytes (at most 18 bits each) and 12 + 4 + 2 bytes of framing -- a few dozen bytes against 1920; a literal costs at
    most 9 bits, and a row carries at most 12 + 4 + 2 + 2 bytes besides."""
    h = w = 640
    bound = ops.png_bound_bytes(h, w, 3)
    assert bound <= 1.13 * h * w * 3 + 64 * h + 1024
    const = np.empty((1, h, w, 3), dtype=np.uint8)
    const[...] = (12, 200, 99)
    noise = np.random.default_rng(3).integers(0, 256, (1, h, w, 3)).astype(np.uint8)
    files = png.encode(torch.from_numpy(np.concatenate([const, noise])).cuda())
    print("constant colour: %d bytes, noise: %d bytes, bound %d, raw %d" % (len(files[0]), len(files[1]), bound, h * w * 3))
    assert len(files[0]) < 0.05 * h * w * 3
    assert len(files[1]) <= bound
    assert np.array_equal(decode(files[0], h, w, 3), const[0])
    assert np.array_equal(decode(files[1], h, w, 3), noise[0])


def test_batch_independence_and_determinism():
    h, w, c = 17, 89, 3
    imgs = contents(h, w, c, seed=11)[[0, 2, 4, 5, 10]]
    x = torch.from_numpy(imgs).cuda()
    files = png.encode(x)
    assert png.encode(x) == files
    for i in range(5):
        assert png.encode(x[i:i + 1].contiguous()) == [files[i]]


def test_write(tmp_path):
    imgs = contents(3, 5, 3, seed=5)[:4]
    paths = [tmp_path / ("im%d.png" % i) for i in range(4)]
    png.write(torch.from_numpy(imgs).cuda(), paths)
    for i, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), imgs[i])
    with pytest.raises(ValueError, match="paths"):
        png.write(torch.from_numpy(imgs).cuda(), paths[:2])


def test_refusals():
    """All from the host, before any launch."""
    ok = torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device="cuda")
    for ch in (2, 4):
        with pytest.raises(RuntimeError, match="C = 1"):
            ops.png_encode(torch.zeros((1, 4, 6, ch), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="uint8"):
        ops.png_encode(ok.float())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.png_encode(torch.zeros((1, 4, 12, 3), dtype=torch.uint8, device="cuda")[:, :, ::2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.png_encode(ok.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode(ok.cpu())
    with pytest.raises(RuntimeError, match="width"):
        ops.png_encode(torch.zeros((1, 1, ops.PNG_MAX_WIDTH + 1, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="N, H, W, C"):
        ops.png_encode(ok[0])
