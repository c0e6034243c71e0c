"""Level 2 of the device PNG encoder (csrc/png.hip: per row the smallest of a fixed-Huffman, a dynamic-Huffman and a stored
block) against independent decoders: PIL for the pixels, zlib / struct for the container and as the yardstick for size.
The encoder is compared with itself only for "level 2 is never longer than level 1"."""
import functools
import heapq
import importlib.util
import json
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from climategan_amd import ops, png
from test_gpu_png import HEIGHTS, WIDTHS, chunks, contents, decode

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent
FIXED, DYNAMIC, STORED = 1, 2, 0


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def idats(b):
    """The IDAT payloads of a file (every chunk CRC checked): one per row, then the closing one."""
    got, end = chunks(b)
    assert end == len(b)
    return [d for k, d in got if k == b"IDAT"]


def row_blocks(b, h):
    """Per row: the deflate data of its chunk (the 2-byte zlib header of row 0 taken off)."""
    parts = idats(b)
    assert len(parts) == h + 1
    assert parts[0][:2] == b"\x78\x01"
    return [parts[0][2:]] + parts[1:h]


def btype(block):
    return (block[0] >> 1) & 3


def filtered(b):
    return zlib.decompress(b"".join(idats(b)))                      # checks the Adler-32


@functools.lru_cache(maxsize=None)
def grid(h, w, c):
    """The level-1 test's images of one shape and their files at both levels, encoded once."""
    imgs = contents(h, w, c, seed=1000 * h + 10 * w + c)
    x = cuda(imgs)
    return imgs, png.encode(x, level=1), png.encode(x, level=2)


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("w", WIDTHS)
def test_exact_round_trip_level2(w, c):
    for h in HEIGHTS:
        imgs, _, files = grid(h, w, c)
        assert len(files) == len(imgs)
        for i, b in enumerate(files):
            assert np.array_equal(decode(b, h, w, c), imgs[i]), (h, w, c, i)
            assert len(filtered(b)) == h * (1 + w * c)               # the Adler-32 and, in idats(), every chunk CRC


def test_level1_is_the_default():
    x = cuda(contents(17, 89, 3, seed=3))
    a, asz = ops.png_encode(x)
    b, bsz = ops.png_encode(x, level=1)
    assert torch.equal(asz, bsz)
    for i, k in enumerate(asz.tolist()):
        assert torch.equal(a[i, :k], b[i, :k])
    assert png.encode(x) == png.encode(x, level=1)


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("w", WIDTHS)
def test_never_longer_and_same_filtered_stream(w, c):
    for h in HEIGHTS:
        _, files1, files2 = grid(h, w, c)
        for i, (b1, b2) in enumerate(zip(files1, files2)):
            r1, r2 = row_blocks(b1, h), row_blocks(b2, h)
            assert all(len(q) <= len(p) for p, q in zip(r1, r2)), (h, w, c, i, [len(p) for p in r1], [len(q) for q in r2])
            assert all(btype(p) == FIXED for p in r1)
            assert filtered(b1) == filtered(b2), (h, w, c, i)          # the level changes the coding only


def test_block_type_one_pixel_rows_are_fixed():
    """Two filtered bytes: 3 + 2 x (8 or 9) + 7 bits fixed; stored takes 12 bytes, a dynamic header alone is longer."""
    imgs = np.random.default_rng(1).integers(0, 256, (8, 5, 1, 1)).astype(np.uint8)
    for b, img in zip(png.encode(cuda(imgs), level=2), imgs):
        assert [btype(p) for p in row_blocks(b, 5)] == [FIXED] * 5
        assert np.array_equal(decode(b, 5, 1, 1), img)


def test_block_type_noise_rows_are_stored_or_better():
    h, w, c = 2, 640, 3
    m = 1 + w * c
    img = np.random.default_rng(2).integers(0, 256, (1, h, w, c)).astype(np.uint8)
    b, = png.encode(cuda(img), level=2)
    blocks = row_blocks(b, h)
    print("noise rows: %s bytes of deflate data, block types %s, m = %d" % ([len(p) for p in blocks], [btype(p) for p in blocks], m))
    for p in blocks:
        assert len(p) + 12 <= m + 10 + 12
    assert np.array_equal(decode(b, h, w, c), img[0])


def no_runs(raw, c):
    """No 3-byte run at distance 1 or c anywhere in the filtered row: nothing the encoder's parse would match."""
    a = np.frombuffer(raw, dtype=np.uint8)
    for dist in {1, c}:
        eq = a[dist:] == a[:-dist]
        if np.any(eq[:-2] & eq[1:-1] & eq[2:]):
            return False
    return True


@pytest.mark.parametrize("w,c", [(640, 3), (640, 1), (87, 3)])
def test_block_type_skewed_row_without_runs_is_dynamic(w, c):
    rng = np.random.default_rng(4)
    L = w * c
    d = (np.arange(L) & 1) + 2 * (rng.geometric(0.5, L) - 1)            # d[i] differs from d[i - 1] and d[i - 3] in bit 0
    img = np.cumsum(d.reshape(w, c), axis=0).astype(np.uint8).reshape(1, 1, w, c)      # Sub gives d back
    b, = png.encode(cuda(img), level=2)
    raw = filtered(b)
    assert raw[0] == 1 and np.array_equal(np.frombuffer(raw, dtype=np.uint8)[1:], d.astype(np.uint8))
    assert no_runs(raw, c)
    block, = row_blocks(b, 1)
    assert btype(block) == DYNAMIC
    assert np.array_equal(decode(b, 1, w, c), img[0])


def huffman_depth(counts):
    heap = [(int(n), k, 0) for k, n in enumerate(counts) if n]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        k += 1
        heapq.heappush(heap, (a[0] + b[0], k, max(a[2], b[2]) + 1))
    return heap[0][2]


def fibonacci_row(L, nval):
    """L filtered bytes near 0 whose histogram, with the end of block as the first 1, is Fibonacci's 1, 1, 2, 3, 5, ...:
    nval byte values, the commonest taking what is left of the row.  The commonest value sits on even positions only and
    the even positions it leaves free are isolated, so that no 3-byte run at distance 1 or 3 exists."""
    fib = [1, 2]
    while len(fib) < nval:
        fib.append(fib[-1] + fib[-2])
    values = [(k + 1) // 2 * (1 if k % 2 else -1) for k in range(nval)][::-1]      # rarest first: ... 2, -1, 1, and 0 last
    rest = np.repeat(np.array(values[:-1]), fib[:-1])
    common = L - len(rest)
    assert fib[-2] < common and 2 * (L // 2 - common) <= L // 2
    np.random.default_rng(8).shuffle(rest)
    holes = np.round(np.linspace(0, L // 2 - 1, L // 2 - common)).astype(np.int64)             # even slots without it
    assert len(np.unique(holes)) == len(holes) and np.all(np.diff(holes) >= 2)
    d = np.full(L, -1000, dtype=np.int64)
    d[0::2] = values[-1]
    d[2 * holes] = -1000
    d[d == -1000] = rest
    return d


@pytest.mark.parametrize("c,nval", [(3, 18), (1, 16)])
def test_length_limiting(c, nval):
    """The 19-symbol Fibonacci histogram (the end of block and 18 byte values; the commonest takes what is left of the 12 288
    bytes) in an RGB row of 4096 pixels: the Huffman tree of the row's literals and its end of block has depth 18, above the
    15 bits a code may have, and the row holds no run to match, so that is the block's histogram (both asserted from the
    decoded stream).  A grey row's 4098 symbols cannot go deeper than 15 (depth 16 needs 4180): its 17 symbols sit exactly
    at the limit."""
    w = 4096
    d = fibonacci_row(w * c, nval)
    img = np.cumsum(d.reshape(w, c), axis=0).astype(np.uint8).reshape(1, 1, w, c)
    b, = png.encode(cuda(img), level=2)
    raw = filtered(b)
    assert raw[0] == 1 and np.array_equal(np.frombuffer(raw, dtype=np.uint8)[1:], d.astype(np.uint8))
    assert no_runs(raw, c)
    counts = np.bincount(np.frombuffer(raw, dtype=np.uint8), minlength=257)
    counts[256] = 1
    assert huffman_depth(counts) == (18 if c == 3 else 15)
    block, = row_blocks(b, 1)
    assert btype(block) == DYNAMIC
    assert np.array_equal(decode(b, 1, w, c), img[0])


@pytest.mark.parametrize("h,w,c", [(2, 4096, 3), (2, 4096, 1), (300, 7, 3)])
def test_round_trip_at_the_limits_level2(h, w, c):
    rng = np.random.default_rng(w + c)
    imgs = np.stack([rng.integers(0, 256, (h, w, c)), np.full((h, w, c), 31)]).astype(np.uint8)
    files = png.encode(cuda(imgs), level=2)
    for i, b in enumerate(files):
        assert len(b) <= ops.png_bound_bytes(h, w, c)
        assert np.array_equal(decode(b, h, w, c), imgs[i])
        assert len(filtered(b)) == h * (1 + w * c)


def photo_crop():
    spec = importlib.util.spec_from_file_location("time_png_write", ROOT.parent / "tools" / "time_png_write.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.photos(1, 640)[0][:16, :640]


def geometric_rows():
    rng = np.random.default_rng(9)
    d = rng.geometric(0.25, (16, 640, 3)) - rng.geometric(0.25, (16, 640, 3))     # two-sided geometric, p = 0.25
    return np.cumsum(d, axis=1).astype(np.uint8)


@pytest.mark.parametrize("name,make", [("photo", photo_crop), ("geometric", geometric_rows)])
def test_size_against_zlib(name, make):
    """IDAT payload <= 1.03 x the sum over rows of zlib's raw deflate (level 9, Z_RLE) of the same filtered row + 5 bytes
    (the empty stored block and the pad that zlib's stream lacks); zlib codes every such row as one dynamic block.
    Measured on an MI355X: photo 1.0004, geometric 1.0005 (every row a dynamic block)."""
    img = make()
    h, w, c = img.shape
    assert (h, w, c) == (16, 640, 3)
    b, = png.encode(cuda(img[None]), level=2)
    assert np.array_equal(decode(b, h, w, c), img)
    raw = filtered(b)
    m = 1 + w * c
    yard = 0
    for r in range(h):
        z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        s = z.compress(raw[r * m:(r + 1) * m]) + z.flush()
        assert s[0] & 7 == 1 | (DYNAMIC << 1), (r, s[0])                 # one final block, dynamic: never a stored yardstick
        yard += len(s) + 5
    payload = sum(len(p) for p in idats(b))
    types = [btype(p) for p in row_blocks(b, h)]
    print("%s: IDAT payload %d bytes, yardstick %d, ratio %.4f, block types %s" % (name, payload, yard, payload / yard, types))
    assert payload <= 1.03 * yard


def test_batch_independence_and_determinism_level2():
    h, w, c = 17, 89, 3
    imgs = contents(h, w, c, seed=11)[[0, 2, 4, 5, 10]]
    x = cuda(imgs)
    files = png.encode(x, level=2)
    assert png.encode(x, level=2) == files
    for i in range(5):
        assert png.encode(x[i:i + 1].contiguous(), level=2) == [files[i]]


def test_refusals_level2():
    """All from the host, before any launch."""
    ok = torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device="cuda")
    for level in (0, 3):
        with pytest.raises(RuntimeError, match="level"):
            ops.png_encode(ok, level=level)
        with pytest.raises(RuntimeError, match="level"):
            png.encode(ok, level=level)
    for ch in (2, 4):
        with pytest.raises(RuntimeError, match="C = 1"):
            ops.png_encode(torch.zeros((1, 4, 6, ch), dtype=torch.uint8, device="cuda"), level=2)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.png_encode(ok.float(), level=2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.png_encode(torch.zeros((1, 4, 12, 3), dtype=torch.uint8, device="cuda")[:, :, ::2], level=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.png_encode(ok.cpu(), level=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode(ok.cpu(), level=2)
    with pytest.raises(RuntimeError, match="width"):
        ops.png_encode(torch.zeros((1, 1, ops.PNG_MAX_WIDTH + 1, 3), dtype=torch.uint8, device="cuda"), level=2)
    with pytest.raises(RuntimeError, match="N, H, W, C"):
        ops.png_encode(ok[0], level=2)


def test_c_abi_refuses_other_levels():
    """cgan_png_encode_u8_level itself: CGAN_ERR_BAD_ARG with a message, nothing launched."""
    from climategan_amd import _lib

    x = torch.zeros((1, 4, 6, 3), dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    bound, nbytes = ops.png_bound_bytes(4, 6, 3), lib.cgan_png_workspace_bytes(1, 4, 6, 3)
    buf = torch.zeros((1, bound), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    for level in (0, 3, -1):
        rc = lib.cgan_png_encode_u8_level(x.data_ptr(), 1, 4, 6, 3, level, buf.data_ptr(), bound, sizes.data_ptr(),
                                          ws.data_ptr(), nbytes, None)
        assert rc != 0
        with pytest.raises(RuntimeError, match="level = %d" % level):
            _lib.check(rc, "cgan_png_encode_u8_level")
    torch.cuda.synchronize()
    assert sizes.item() == -7 and not buf.any()


def test_cli_png_level(tmp_path):
    """``--png_level 2``: the same file names, every file decodes to ``infer_all(numpy=True)``'s arrays, and the directory is
    no larger than a level-1 run's on the same photos.  The command runs in this process (``main(argv)``), because the
    wildfire's green level is drawn from ``random`` once per batch, as the reference draws it: seeded here before each run
    and before ``infer_all``, which a child process would not allow."""
    import random

    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.eval_masker import find_images
    from climategan_amd.trainer import Trainer
    import yaml

    from climategan_amd.config import Opts
    from climategan_amd import apply_events
    from test_gpu_apply_events_cli import SIZE, photo

    o = Opts(yaml.safe_load((ROOT / "golden" / "ckpt_small" / "opts.yaml").read_text()))       # the small saved run
    o.tasks = ["d", "s", "m", "p"]
    run = tmp_path / "run"
    o.output_path = str(run)
    T = Trainer(o, device="cuda").setup(inference=True)
    (run / "checkpoints").mkdir(parents=True)
    torch.save({"G": T.G.state_dict()}, run / "checkpoints" / "latest_ckpt.pth")
    (run / "opts.yaml").write_text(yaml.safe_dump(json.loads(json.dumps(o))))
    rng = np.random.default_rng(23)
    (tmp_path / "imgs").mkdir()
    for i, (h, w) in enumerate(((300, 400), (256, 700))):
        Image.fromarray(photo(rng, h, w)).save(tmp_path / "imgs" / ("im%d.png" % i))
    sizes = {}
    for level in (1, 2):
        out_dir = tmp_path / ("out%d" % level)
        argv = ["-i", tmp_path / "imgs", "-r", run, "-b", 2, "-t", SIZE, "--save_masks", "-s", "-o", out_dir, "--no_cloudy",
                "--no_time", "--no_conf", "--png_level", level]
        grad = torch.is_grad_enabled()
        random.seed(5)
        try:
            assert apply_events.main([str(a) for a in argv]) == out_dir.resolve()
        finally:
            torch.set_grad_enabled(grad)                             # main() turns autograd off for its process
        sizes[level] = {p.name: p.stat().st_size for p in out_dir.iterdir()}
    paths = find_images(tmp_path / "imgs")
    events = ("flood", "wildfire", "smog", "mask", "input")
    assert set(sizes[2]) == set(sizes[1]) == {"%s_%s_%d_no_cloudy.png" % (p.stem, e, SIZE) for p in paths for e in events}
    print("apply_events output: %d bytes at level 1, %d at level 2" % (sum(sizes[1].values()), sum(sizes[2].values())))
    assert sum(sizes[2].values()) <= sum(sizes[1].values())
    R = Trainer.resume_from_path(run, inference=True, new_exp=None, device="cuda")
    x = prepare_batch([np.asarray(Image.open(p)) for p in paths], to=SIZE)
    random.seed(5)
    want = R.infer_all(x, numpy=True, bin_value=0.5, cloudy=False, return_masks=True)
    want["mask"] = want["mask"][:, 0]
    want["input"] = ((x.cpu().numpy() + 1) / 2 * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    for i, p in enumerate(paths):
        for e in events:
            got = np.asarray(Image.open(tmp_path / "out2" / ("%s_%s_%d_no_cloudy.png" % (p.stem, e, SIZE))))
            assert got.shape == want[e][i].shape and np.array_equal(got, want[e][i]), (p.name, e)
