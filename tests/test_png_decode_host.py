"""The PNG decoder's host side, no GPU: ``cgan_png_parse_host``, ``cgan_png_stream_host`` and
``cgan_png_decode_host`` (csrc/png_decode_core.h: the functions the kernels run, taken serially) against the model of
``tests/png_decode_model.py``, the model against ``PIL.Image.open``, and the refusals.  Every stage is integer: the tolerance
is 0 everywhere."""
import io
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import png_decode_corpus as pc
import png_decode_model as pm

ROOT = Path(__file__).resolve().parent.parent
CORPUS = pc.corpus()
IDS = [name for name, _ in CORPUS]


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def pil_raises(data):
    try:
        pil_pixels(data)
    except Exception:
        return True
    return False


@pytest.mark.parametrize("name,data", CORPUS, ids=IDS)
def test_model_equals_pil(name, data):
    r, ref = pc.model(data), pil_pixels(data)
    assert ref.dtype == r["pixels"].dtype and np.array_equal(ref.reshape(r["pixels"].shape), r["pixels"])


@pytest.mark.parametrize("name,data", CORPUS, ids=IDS)
def test_parser_and_twin_equal_the_model(name, data):
    r = pc.model(data)
    d, status, why = pc.parse_host(data)
    assert status == pc.OK, why
    assert (d.height, d.width, d.channels, d.bit_depth, d.stream_bytes) == (r["h"], r["w"], r["c"], r["depth"], len(r["stream"]))
    stream = pc.stream_host(data, d)
    assert stream == r["stream"]
    inflated, px, status, why = pc.decode_host(stream, d)
    assert status == pc.OK, why
    assert inflated == zlib.decompress(stream)
    ref = pil_pixels(data)
    assert px.dtype == ref.dtype and np.array_equal(px, ref.reshape(px.shape))


def test_coverage_conditions():
    """What the corpus must exercise, asserted from the model's token lists, so that the exactness above cannot go blind."""
    models = [pc.model(data) for _, data in CORPUS]
    tokens = [t for r in models if "tokens" in r for t in r["tokens"]]
    matches = {(t[1], t[2]) for t in tokens if t[0] == "match"}
    assert (258, 1) in matches                                                   # distance 1, length 258
    assert any(1 < d < n for n, d in matches)                                    # a repeat of more than one byte
    assert any(d == 32768 for _, d in matches)                                   # the farthest distance
    blocks = [b for r in models if "blocks" in r for b in r["blocks"]]
    dynamic = [b for b in blocks if b["kind"] == "dynamic"]
    assert any(b["longest"] == 15 for b in dynamic)                              # a code of 15 bits
    assert {16, 17, 18} <= set().union(*(b["cl"] for b in dynamic))              # the three repeat symbols
    assert any(b["ndist"] == 1 for b in dynamic)                                 # a single distance code
    assert any(b["start"] % 8 for b in blocks)                                   # a block boundary inside a byte
    assert any({b["kind"] for b in r["blocks"]} == {"stored", "fixed", "dynamic"} for r in models if "blocks" in r)
    stored = [r for r in models if "blocks" in r and sum(b["kind"] == "stored" for b in r["blocks"]) > 1]
    assert any(len(r["inflated"]) > 65535 for r in stored)                       # stored blocks beyond one block's 65 535 bytes
    assert any(any(t == ("stored", 0) for t in r["tokens"]) for r in models if "tokens" in r)    # an empty stored block
    idats = [[len(p) for k, p, _ in pm.chunks(data) if k == b"IDAT"] for _, data in CORPUS]
    assert any(len(i) > 1 and sum(i) > 65536 for i in idats)                     # PIL's own split of a long stream
    assert any(set(i) == {1} and len(i) > 1 for i in idats) and any(0 in i for i in idats) and any(7 in i for i in idats)
    filters = set()
    for r in models:
        filters |= set(np.frombuffer(r["inflated"], dtype=np.uint8).reshape(r["h"], -1)[:, 0].tolist())
    assert filters == {0, 1, 2, 3, 4}
    kinds = {(r["c"], r["depth"]) for r in models}
    assert kinds == {(1, 8), (3, 8), (4, 8), (1, 16)}
    assert len(pc.model(pc.big_file())["stream"]) > 1 << 20                      # the long stream: many blocks


def test_unsupported_files_are_refused():
    seen = set()
    for name, data in pc.unsupported_files():
        _, status, why = pc.parse_host(data)
        assert status == pc.UNSUPPORTED and why, name
        seen.add(why)
    assert len(seen) >= 9                                                          # each kind with its own reason


def zlib_header(cmf, flg=0):
    """The two bytes with a valid check value, so that the field under test is what is wrong."""
    return bytes([cmf, flg + (31 - (cmf * 256 + flg) % 31) % 31])


def test_parser_reports_corrupt():
    name, data = CORPUS[0]
    cs = pm.chunks(data)
    idat = b"".join(p for k, p, _ in cs if k == b"IDAT")
    ihdr = pm.chunk(b"IHDR", cs[0][1])
    end = pm.chunk(b"IEND", b"")
    bad_crc = bytearray(data)
    bad_crc[8 + 8 + 13] ^= 1
    cases = {"a chunk past the end": data[:-20],
             "no IHDR": pm.SIGNATURE + pm.chunk(b"IDAT", idat) + end,
             "no IDAT": pm.SIGNATURE + ihdr + end,
             "IDAT not consecutive": pm.SIGNATURE + ihdr + pm.chunk(b"IDAT", idat[:10]) + pm.chunk(b"tEXt", b"a\0b")
                                     + pm.chunk(b"IDAT", idat[10:]) + end,
             "bad IHDR CRC": bytes(bad_crc),
             "zlib CM": pc.reframed(data, zlib_header(0x77) + idat[2:]),
             "zlib CINFO": pc.reframed(data, zlib_header(0x88) + idat[2:]),
             "zlib FDICT": pc.reframed(data, zlib_header(0x78, 0x20) + idat[2:]),
             "zlib FCHECK": pc.reframed(data, bytes([0x78, 0x9D]) + idat[2:]),
             "one byte of stream": pc.reframed(data, idat[:1])}
    for what, bad in cases.items():
        _, status, why = pc.parse_host(bad)
        assert status == pc.CORRUPT and why, what
    # a wrong IDAT CRC is not looked at, as in PIL
    at = next(off + len(p) for k, p, off in cs if k == b"IDAT")
    wrong = bytearray(data)
    wrong[at] ^= 1
    assert pc.parse_host(bytes(wrong))[1] == pc.OK and not pil_raises(bytes(wrong))


def test_cut_and_changed_files_are_corrupt_and_pil_refuses_them():
    files = pc.broken_files()
    assert len(files) == 25
    for name, data in files:
        assert pil_raises(data), name                                              # inside what the reference decoder rejects
        d, status, why = pc.parse_host(data)
        assert status == pc.OK, (name, why)                                        # the chunks are valid: the stream is not
        inflated, px, status, why = pc.decode_host(pc.stream_host(data, d), d)
        assert status == pc.CORRUPT and why, name


def test_every_cause_of_corrupt():
    bad, good = pc.corrupt_streams()
    _, px, status, _ = pc.decode_host(good, pc.stream_desc(good, 4, 7))
    assert status == pc.OK and np.array_equal(px.reshape(4, 7), pm.unfilter(zlib.decompress(good), 4, 7, 1))
    assert len(bad) == 23
    for name, stream in bad:
        _, _, status, why = pc.decode_host(stream, pc.stream_desc(stream, 4, 7))
        assert status == pc.CORRUPT and why, name
        with pytest.raises(pm.Corrupt):                                            # the definition refuses it too
            pm.unfilter(pm.inflate(stream, 32)[0], 4, 7, 1)


def test_decode_host_refusals():
    import ctypes as C

    from climategan_amd import _lib

    lib = _lib.load()
    _, good = pc.corrupt_streams()
    d = pc.stream_desc(good, 4, 7)
    assert lib.cgan_png_decode_workspace_bytes(C.addressof(d), 1) > 0
    for field, value in (("width", 8193), ("height", 0), ("channels", 2), ("bit_depth", 4), ("stream_bytes", 1)):
        bad = type(d).from_buffer_copy(d)
        setattr(bad, field, value)
        src, buf, status = np.frombuffer(good, dtype=np.uint8).copy(), np.zeros(64, dtype=np.uint8), C.c_int32(0)
        assert lib.cgan_png_decode_host(src.ctypes.data, C.addressof(bad), buf.ctypes.data, buf.ctypes.data, C.addressof(status)) != 0
        assert lib.cgan_png_decode_workspace_bytes(C.addressof(bad), 1) == 0, field
    deep_rgb = type(d).from_buffer_copy(d)
    deep_rgb.channels, deep_rgb.bit_depth = 3, 16
    assert lib.cgan_png_decode_workspace_bytes(C.addressof(deep_rgb), 1) == 0
    assert lib.cgan_png_decode_workspace_bytes(C.addressof(d), 0) == 0


def test_cpu_call_raises_and_probe():
    from climategan_amd import png

    with pytest.raises(RuntimeError):
        png.decode([CORPUS[0][1]], device="cpu")
    d, why = png.probe(CORPUS[0][1])
    assert d is not None and why is None and (d.width, d.height, d.channels, d.bit_depth) == (41, 33, 3, 8)
    assert png.stream_of(CORPUS[0][1], d) == pc.model(CORPUS[0][1])["stream"]
    d, why = png.probe(pc.interlaced_file())
    assert d is None and "interlac" in why


def test_decode_option_says_png(capsys):
    from climategan_amd import apply_events

    assert "png.decode" in apply_events.__doc__ and "png.decode" in apply_events.read_images.__doc__
    with pytest.raises(SystemExit):
        apply_events.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "8-bit RGB PNG files are uploaded as bytes" in text
    assert apply_events.parse_args(["-i", "x"]).decode == "host"                  # the default stays


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no compiler")
def test_core_under_sanitizers(tmp_path):
    """tools/png_decode_asan.cpp (its own ``main``, the core header and nothing of the GPU) built with
    -fsanitize=address,undefined and run over every fourth corpus file and all cut, changed and unsupported ones."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "png_decode_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "climategan_amd" / "csrc"),
                    str(ROOT / "tools" / "png_decode_asan.cpp"), "-o", str(exe)], check=True, timeout=120)
    bad, _ = pc.corrupt_streams()
    grey = np.zeros((4, 7, 1), dtype=np.uint8)
    files = (list(CORPUS[::4]) + list(pc.broken_files()) + list(pc.unsupported_files())
             + [(name, pm.frame(grey, stream)) for name, stream in bad])
    for k, (_, data) in enumerate(files):
        (tmp_path / ("f%03d.png" % k)).write_bytes(data)
    out = subprocess.run([str(exe)] + sorted(str(p) for p in tmp_path.glob("f*.png")), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    n_ok = len(CORPUS[::4])
    assert "%d files: %d decoded, %d with a status from the decode, %d refused" % (
        len(files), n_ok, len(pc.broken_files()) + len(bad), len(pc.unsupported_files())) in out.stdout
