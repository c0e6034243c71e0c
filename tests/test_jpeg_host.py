"""The JPEG encoder's host side, no GPU: the tables and the entropy coder of ``tests/jpeg_model.py`` and of
``cgan_jpeg_tables`` / ``cgan_jpeg_scan_host`` (csrc/jpeg_tables.h: the functions the kernels run) against libjpeg as PIL
drives it, the model's transform against PIL's in picture quality and file size, and the conditions the GPU grid relies on.

Measured on the 78 cases below (``pytest -s`` prints every figure): PIL's decode of the model's file is at most 0.090 dB
below PIL's decode of PIL's own file at the same settings (sinusoid 33 x 41 x 3, quality 100, 4:2:0; the other way round the
model is up to 3.0 dB better), and the model's file is at most 1.0121 times as long as PIL's -- except where the frame has
whole padding blocks (4:2:0 with an odd number of 8-pixel blocks in a direction): there 1.1164 times (noise 136 x 24 x 3,
quality 25), because libjpeg codes such a block as a repeated DC with no AC values where the format here codes the
replicated pixels.  The assertions allow those figures plus 0.1 dB and plus 0.005.  Left out of the picture-quality
comparison, with its reason: p44 at quality 25, whose only AC coefficient is an exact rounding tie (1020 / 136 = 7.5), so that
the last bit of the DCT and not the encoder decides between 56 dB and 30 dB."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_model as jm
from climategan_amd import _lib
from climategan_amd.apply_events import parse_args

QUALITIES = (1, 10, 25, 49, 50, 75, 90, 95, 100)
# kind, h, w, c
IMAGES = [(kind, 33, 41, 3) for kind in jm.CONTENTS] + [(kind, 24, 17, 1) for kind in jm.CONTENTS] + [
    ("noise", 136, 24, 3), ("noise", 136, 24, 1), ("checker", 16, 48, 1), ("sinusoid", 64, 64, 3), ("noise", 1, 1, 3)]
CASES = [(kind, h, w, c, q, sub) for kind, h, w, c in IMAGES for q in (25, 90, 100)
         for sub in (("444", "420") if c == 3 else ("444",))]
PSNR_GAP_DB = 0.090 + 0.1        # the measured worst PSNR(PIL's file) - PSNR(model's file), plus the margin for PIL's integer DCT
SIZE_RATIO = 1.0121 + 0.005      # the measured worst len(model's file) / len(PIL's file), plus its margin
SIZE_RATIO_PADDED = 1.1164 + 0.005   # the same where the frame has whole padding blocks


def has_padding_blocks(h, w, c, sub):
    return c == 3 and sub == "420" and bool((-(-h // 8)) % 2 or (-(-w // 8)) % 2)


def pil_file(img, quality, sub):
    b = io.BytesIO()
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    im.save(b, "JPEG", quality=quality, subsampling=0 if sub == "444" else 2, optimize=False, restart_marker_rows=1)
    return b.getvalue()


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def scan_host(coef, h, w, c, quality, sub):
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    cap = _lib.load().cgan_jpeg_bound_bytes(h, w, c, int(sub))
    assert cap > 0
    out = np.zeros(cap, dtype=np.uint8)
    size = C.c_size_t(0)
    _lib.check(_lib.load().cgan_jpeg_scan_host(coef.ctypes.data, h, w, c, quality, int(sub), out.ctypes.data, cap,
                                               C.addressof(size)), "cgan_jpeg_scan_host")
    return out[:size.value].tobytes()


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("quality", QUALITIES)
def test_tables_are_libjpegs(quality):
    luma, chroma = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    _lib.check(_lib.load().cgan_jpeg_tables(quality, luma.ctypes.data, chroma.ctypes.data), "cgan_jpeg_tables")
    pil = decode(pil_file(jm.make_image("noise", 16, 16, 3), quality, "444")).quantization
    # Pillow hands the tables out in natural order (older versions: in the file's zig-zag order)
    for got in ((luma.tolist(), chroma.tolist()), jm.quant_tables(quality)):
        for t in range(2):
            assert list(got[t]) == list(pil[t]) or [got[t][jm.ZIGZAG[k]] for k in range(64)] == list(pil[t]), (quality, t)
    assert jm.read(pil_file(jm.make_image("noise", 16, 16, 3), quality, "444"))["qtables"] == {
        0: luma.tolist(), 1: chroma.tolist()}


def test_tables_refusals():
    buf = np.zeros(64, dtype=np.uint8)
    for q in (0, 101, -1):
        assert _lib.load().cgan_jpeg_tables(q, buf.ctypes.data, buf.ctypes.data) != 0


@pytest.mark.parametrize("kind,h,w,c,quality,sub", CASES)
def test_entropy_stage_is_libjpegs(kind, h, w, c, quality, sub):
    """``read`` recovers PIL's coefficients; ``write`` and ``cgan_jpeg_scan_host`` of them give PIL's bytes back."""
    ref = pil_file(jm.make_image(kind, h, w, c), quality, sub)
    r = jm.read(ref)
    assert (r["h"], r["w"], r["c"], r["subsampling"]) == (h, w, c, sub)
    mine = jm.write(r["coef"], h, w, c, quality, sub)
    m = jm.read(mine)
    assert m["scan"] == r["scan"]                      # SOS .. EOI: the coder, the stuffing, the padding, the RST cycle
    for key in ("dqt", "dht", "sof", "dri"):
        assert m[key] == r[key], key
    assert np.array_equal(m["coef"], r["coef"])
    assert scan_host(r["coef"], h, w, c, quality, sub) == mine


@pytest.mark.parametrize("kind,h,w,c,quality,sub", CASES)
def test_model_files_decode_and_compare_with_pil(kind, h, w, c, quality, sub):
    img = jm.make_image(kind, h, w, c)
    coef, _ = jm.transform(img, quality, sub)
    mine = jm.write(coef, h, w, c, quality, sub)
    im = decode(mine)
    assert im.size == (w, h) and im.mode == ("RGB" if c == 3 else "L")
    ref = pil_file(img, quality, sub)
    src = img[..., 0] if c == 1 else img
    p_mine, p_ref = psnr(np.asarray(im), src), psnr(np.asarray(decode(ref)), src)
    print("%s %dx%dx%d q%d %s: PSNR model %.3f PIL %.3f (gap %.3f dB), bytes model %d PIL %d (ratio %.4f)" % (
        kind, h, w, c, quality, sub, p_mine, p_ref, p_ref - p_mine, len(mine), len(ref), len(mine) / len(ref)))
    if not (kind == "p44" and quality == 25):           # an exact rounding tie: see the module's text
        assert p_ref - p_mine <= PSNR_GAP_DB
    assert len(mine) / len(ref) <= (SIZE_RATIO_PADDED if has_padding_blocks(h, w, c, sub) else SIZE_RATIO)


def symbols_of(kind, h, w, c, quality, sub="444"):
    coef, _ = jm.transform(jm.make_image(kind, h, w, c), quality, sub)
    symbols = []
    data = jm.write(coef, h, w, c, quality, sub, symbols)
    return coef, symbols, data


def test_coverage_conditions():
    """What the GPU grid's cases must exercise, asserted on the model so that the grid cannot go blind."""
    _, _, data = symbols_of("noise", 33, 33, 3, 100)
    assert b"\xff\x00" in jm.read(data)["scan"]                                        # a stuffed byte
    _, symbols, _ = symbols_of("checker", 16, 17, 1, 100)
    assert ("DC", 11) in symbols                                                       # the widest DC difference
    _, symbols, _ = symbols_of("p44", 8, 8, 1, 100)
    assert any(kind == "AC" and sym & 15 == 10 for kind, sym in symbols)               # the widest AC value
    coef, symbols, _ = symbols_of("ripple77", 8, 8, 1, 25)
    assert np.flatnonzero(coef).tolist() == [63]
    assert [s for _, s in symbols] == [0, 0xF0, 0xF0, 0xF0, (62 - 48) << 4 | jm._category(coef[63])]   # three ZRL in a row
    _, symbols, _ = symbols_of("constant", 17, 9, 3, 90)
    assert [s for kind, s in symbols if kind == "AC"] == [0] * (3 * 2 * 3)            # EOB-only blocks
    r = jm.read(symbols_of("noise", 136, 24, 3, 90)[2])
    assert r["rst"] == [k % 8 for k in range(16)]                                      # RST7 wraps to RST0


def test_scan_host_refusals():
    coef = np.zeros(64, dtype=np.int16)
    out = np.zeros(4096, dtype=np.uint8)
    size = C.c_size_t(0)
    lib = _lib.load()

    def call(coef, h=8, w=8, c=1, q=90, sub=444, cap=4096):
        return lib.cgan_jpeg_scan_host(coef.ctypes.data, h, w, c, q, sub, out.ctypes.data, cap, C.addressof(size))

    assert call(coef) == 0 and size.value > 0
    assert call(coef, c=2) != 0 and call(coef, q=0) != 0 and call(coef, sub=422) != 0 and call(coef, w=4097) != 0
    assert call(coef, cap=10) != 0
    bad = coef.copy()
    bad[5] = 1024
    assert call(bad) != 0
    assert lib.cgan_jpeg_bound_bytes(8, 8, 2, 444) == 0 and lib.cgan_jpeg_workspace_bytes(0, 8, 8, 3, 444) == 0


def test_format_options():
    base = ["-i", "x"]
    a = parse_args(base)
    assert (a.format, a.jpeg_quality, a.jpeg_subsampling) == ("png", 90, "444")
    assert "format" not in vars(a) and "jpeg_quality" not in vars(a) and "jpeg_subsampling" not in vars(a)
    a = parse_args(base + ["--format", "jpg", "--jpeg_quality", "75", "--jpeg_subsampling", "420"])
    assert (a.format, a.jpeg_quality, a.jpeg_subsampling) == ("jpg", 75, "420")
    for bad in (["--jpeg_quality", "80"], ["--jpeg_subsampling", "420"], ["--format", "png", "--jpeg_quality", "80"],
                ["--format", "jpg", "--jpeg_quality", "0"], ["--format", "jpg", "--jpeg_quality", "101"],
                ["--format", "gif"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
