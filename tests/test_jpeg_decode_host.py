"""The JPEG decoder's host side, no GPU: ``cgan_jpeg_parse_host`` and ``cgan_jpeg_decode_coefficients_host``
(csrc/jpeg_decode_core.h: the functions the kernels run, their rounds taken serially) against the model reader of
``tests/jpeg_decode_model.py``, the model's integer reconstruction against ``PIL.Image.open``, and the refusals.

Model against PIL, measured on the corpus below with PIL 12.2 / libjpeg-turbo (``pytest -s`` prints the figures): the integer
model equals PIL's pixels exactly -- largest difference 0, mean 0 -- for grey, 4:4:4, 4:2:2 and 4:2:0 alike (a float64 model of
the same stages was up to 3 levels off for colour and 1 for grey).  The assertion allows 0 + 1 level, the margin for libjpeg
builds that pick another inverse DCT."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_corpus as jc
import jpeg_decode_model as dm
import jpeg_model as jm
from climategan_amd.apply_events import parse_args

ROOT = Path(__file__).resolve().parent.parent
CORPUS = jc.host_corpus()
IDS = [name for name, _ in CORPUS]
SUBSEQS = (4, 16, 0)
PIL_MAX_DIFF = 0 + 1


@pytest.mark.parametrize("name,data", CORPUS, ids=IDS)
def test_parse_agrees_with_the_model(name, data):
    r = jc.model(data)
    d, status, why = jc.parse_host(data)
    assert status == jc.OK, why
    assert (d.height, d.width, d.ncomp, d.hs, d.vs, d.restart_interval) == (r["h"], r["w"], r["c"], r["hs"], r["vs"], r["interval"])
    assert (d.scan_offset, d.scan_bytes) == (r["scan_offset"], r["scan_bytes"])
    for k in range(r["c"]):
        assert list(d.quant[k]) == r["qtables"][k]
        for mine, (bits, vals) in zip((d.dc[k], d.ac[k]), r["huff"][k]):
            assert jc.codes_of_hufftab(mine) == jm.codes_of(bits, vals)
    if name.startswith("model-"):
        assert np.array_equal(r["coef"], jm.read(data)["coef"])          # the generalised reader against the one it came from


@pytest.mark.parametrize("name,data", CORPUS, ids=IDS)
def test_coefficients_equal_the_models_at_every_subsequence_size(name, data):
    r = jc.model(data)
    d, _, _ = jc.parse_host(data)
    for subseq in SUBSEQS:
        coef, status, rounds = jc.decode_host(data, d, subseq)
        assert status == jc.OK, (subseq, status)
        assert np.array_equal(coef, r["coef"]), subseq
        assert rounds >= 1


def test_coverage_conditions():
    """What the corpus must exercise, so that the exactness above cannot go blind."""
    assert any(jc.model(data)["stuffed"] for _, data in CORPUS)                           # a stuffed FF 00
    assert any(jc.model(data)["longest_block_bits"] > 16 * 8 for _, data in CORPUS)       # a block longer than a subsequence
    most = max(jc.decode_host(data, jc.parse_host(data)[0], 4)[2] for _, data in CORPUS)
    print("most rounds to the fixpoint at 4 bytes per subsequence: %d" % most)
    assert most >= 3
    rsts = [jc.model(data)["rst"] for _, data in CORPUS]
    assert any(len(r) > 8 and r[:9] == [0, 1, 2, 3, 4, 5, 6, 7, 0] for r in rsts)         # RST7 -> RST0
    subs = {(jc.model(data)["c"], jc.model(data)["hs"], jc.model(data)["vs"]) for _, data in CORPUS}
    assert subs == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    intervals = {jc.model(data)["interval"] for _, data in CORPUS}
    assert {0, 1, 3} <= intervals and len(intervals) > 3                                   # none, 1 MCU, 3 MCUs, a row


def test_round_cap_reports_not_converged():
    name, data = max(CORPUS, key=lambda f: jc.decode_host(f[1], jc.parse_host(f[1])[0], 4)[2])
    d, _, _ = jc.parse_host(data)
    _, status, rounds = jc.decode_host(data, d, 4)
    assert status == jc.OK and rounds >= 3
    _, status, _ = jc.decode_host(data, d, 4, round_cap=1)
    assert status == jc.NOT_CONVERGED
    coef, status, _ = jc.decode_host(data, d, 4, round_cap=rounds)
    assert status == jc.OK and np.array_equal(coef, jc.model(data)["coef"])


def test_model_against_pil():
    """The integer model's pixels against ``PIL.Image.open``'s, per (components, subsampling): see the module's text."""
    worst, total, count = {}, {}, {}
    for name, data in CORPUS:
        r = jc.model(data)
        mine = dm.reconstruct(r["coef"], r["h"], r["w"], r["c"], r["hs"], r["vs"], r["qtables"])
        ref = np.asarray(Image.open(__import__("io").BytesIO(data))).reshape(mine.shape)
        diff = np.abs(mine.astype(np.int64) - ref.astype(np.int64))
        key = (r["c"], "%dx%d" % (r["hs"], r["vs"]))
        worst[key] = max(worst.get(key, 0), int(diff.max()))
        total[key], count[key] = total.get(key, 0) + int(diff.sum()), count.get(key, 0) + diff.size
    for key in sorted(worst):
        print("components %d, luma %s: largest difference %d, mean %.4f" % (key + (worst[key], total[key] / count[key])))
    assert len(worst) == 4 and max(worst.values()) <= PIL_MAX_DIFF


def test_unsupported_files_are_refused():
    for name, data in jc.unsupported_files():
        _, status, why = jc.parse_host(data)
        assert status == jc.UNSUPPORTED and why, name
    for data in (b"", b"\x89PNG\r\n\x1a\n" + bytes(32)):
        assert jc.parse_host(data)[1] == jc.CORRUPT


def test_cut_and_changed_files_give_a_status_or_a_result():
    good = 0
    for name, data in jc.broken_files():
        d, status, why = jc.parse_host(data)
        if status != jc.OK:
            assert status in (jc.UNSUPPORTED, jc.CORRUPT) and why, name
            continue
        for subseq in SUBSEQS:
            coef, status, _ = jc.decode_host(data, d, subseq)
            assert status in (jc.OK, jc.CORRUPT), (name, subseq)
            assert not np.any(coef == 0x5555) or status != jc.OK        # a decoded result fills every value
            good += status == jc.OK
    print("%d of the broken files' decodes ended with status 0" % good)


def test_decode_host_refusals():
    name, data = CORPUS[0]
    d, _, _ = jc.parse_host(data)
    from climategan_amd import _lib
    import ctypes as C

    lib = _lib.load()
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    coef = np.zeros(64 * jc.blocks_of(d), dtype=np.int16)
    rounds, status = C.c_int32(0), C.c_int32(0)

    def call(desc=d, nbytes=len(data), subseq=0, count=coef.size):
        return lib.cgan_jpeg_decode_coefficients_host(buf.ctypes.data, nbytes, C.addressof(desc), subseq, 0, coef.ctypes.data,
                                                      count, C.addressof(rounds), C.addressof(status))

    assert call() == 0
    assert call(subseq=3) != 0 and call(subseq=4097) != 0 and call(count=coef.size - 1) != 0
    assert call(nbytes=d.scan_offset + d.scan_bytes - 1) != 0
    for field, value in (("width", 8193), ("ncomp", 2), ("hs", 3), ("vs", 2 if d.ncomp == 1 else 4)):
        bad = type(d).from_buffer_copy(d)
        setattr(bad, field, value)
        assert call(desc=bad) != 0, field
    # the size query of the device calls refuses the same descriptors, without a GPU
    assert lib.cgan_jpeg_decode_workspace_bytes(C.addressof(d), 1, 0) > 0
    assert lib.cgan_jpeg_decode_workspace_bytes(C.addressof(d), 1, 3) == 0
    assert lib.cgan_jpeg_decode_workspace_bytes(C.addressof(bad), 1, 0) == 0


def test_decode_option():
    a = parse_args(["-i", "x"])
    assert a.decode == "host" and "decode" not in vars(a)
    assert parse_args(["-i", "x", "--decode", "device"]).decode == "device"
    with pytest.raises(SystemExit):
        parse_args(["-i", "x", "--decode", "gpu"])


def test_cpu_call_raises():
    from climategan_amd import jpeg

    with pytest.raises(RuntimeError):
        jpeg.decode([CORPUS[0][1]], device="cpu")
    d, why = jpeg.probe(CORPUS[0][1])
    assert d is not None and why is None and (d.width, d.height) == (41, 33)
    d, why = jpeg.probe(jc.unsupported_files()[0][1])
    assert d is None and "progressive" in why


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no compiler")
def test_core_under_sanitizers(tmp_path):
    """tools/jpeg_decode_asan.cpp (its own ``main``, the core header and nothing of the GPU) built with
    -fsanitize=address,undefined and run over the corpus files and the cut / changed ones."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "jpeg_decode_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "climategan_amd" / "csrc"),
                    str(ROOT / "tools" / "jpeg_decode_asan.cpp"), "-o", str(exe)], check=True, timeout=120)
    files = list(CORPUS[::4]) + list(jc.broken_files()) + list(jc.unsupported_files())
    for k, (_, data) in enumerate(files):
        (tmp_path / ("f%03d.jpg" % k)).write_bytes(data)
    out = subprocess.run([str(exe)] + sorted(str(p) for p in tmp_path.glob("f*.jpg")), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "%d files" % len(files) in out.stdout
