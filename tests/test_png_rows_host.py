"""The PNG decoder's row path on the host, no GPU: the parser's ``rows`` word, ``cgan_png_row_table_host``, the
row twin ``cgan_png_decode_rows_host`` (csrc/png_decode_core.h's functions row by row, then the serial fallback) against the
model of ``tests/png_decode_model.py`` and PIL, the table checks of ``cgan_png_decode_rows``'s host half, and the sanitizer
program.  Every stage is integer: the tolerance is 0 everywhere."""
import ctypes as C
import io
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import png_decode_corpus as pc
import png_decode_model as pm
import png_rows_cases as rc
from climategan_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
FRAMED, REFUSED, BROKEN = rc.framed_files(), rc.refused_files(), rc.broken_files()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def test_rows_word_and_table_agree_with_the_chunks():
    for name, data in FRAMED + REFUSED + BROKEN:
        d, status, why = pc.parse_host(data)
        n = rc.idat_lengths(data)
        assert status == pc.OK and d.rows == d.height == len(n) - 1, (name, why)
        table = rc.row_table_host(data, d).tolist()
        assert table == rc.expected_table(data) and table[-1] + n[-1] == d.stream_bytes == sum(n), name
    # what the candidate rule leaves out: a first chunk that is only the zlib header, an empty chunk in the middle, a chunk more
    name, data = FRAMED[20]
    r, n = rc.model(data), rc.idat_lengths(data)
    assert r["h"] == 2 and len(n) == 3
    img = r["pixels"]
    for idat in ([2, n[0] + n[1] - 2], [n[0], 0, n[1]], [n[0], n[1], 1]):
        d, status, _ = pc.parse_host(pm.frame(img, r["stream"], idat=idat))
        assert status == pc.OK and d.rows == 0, idat
    d, _, _ = pc.parse_host(pm.frame(img, r["stream"], idat=[n[0], n[1]]))
    assert d.rows == 2                                                              # an empty tail chunk is the row path's to refuse


def test_ordinary_files_are_no_candidates_or_still_decode():
    accidents = 0
    for name, data in pc.corpus():
        d, status, _ = pc.parse_host(data)
        assert status == pc.OK
        if d.rows == 0:
            continue
        accidents += 1                                                              # height + 1 chunks by accident
        px, status, path, _, _ = rc.decode_rows_host(data)
        want = pc.model(data)["pixels"]
        assert status == pc.OK and path in (rc.ROWS, rc.REFUSED) and px.dtype == want.dtype and np.array_equal(px, want), name
    assert accidents < len(pc.corpus()) // 10
    assert all(pc.parse_host(data)[0].rows == 0 for name, data in pc.corpus() if name.startswith("pil-"))


@pytest.mark.parametrize("name,data", FRAMED, ids=[n for n, _ in FRAMED])
def test_framed_files_go_by_rows(name, data):
    px, status, path, d, _ = rc.decode_rows_host(data)
    want, ref = rc.model(data)["pixels"], pil_pixels(data)
    assert status == pc.OK and path == rc.ROWS
    assert px.dtype == want.dtype == ref.dtype and np.array_equal(px, want) and np.array_equal(px, ref.reshape(px.shape))


@pytest.mark.parametrize("name,data", REFUSED, ids=[n for n, _ in REFUSED])
def test_refused_candidates_fall_back(name, data):
    px, status, path, d, _ = rc.decode_rows_host(data)
    want = rc.model(data)["pixels"]
    assert d.rows == d.height and status == pc.OK and path == rc.REFUSED
    assert np.array_equal(px, want) and np.array_equal(px, pil_pixels(data).reshape(px.shape))


def test_sync_flush_matches_reach_into_the_row_above():
    r = rc.model(dict(REFUSED)["sync-flush-identical-rows"])
    rows = rc.tokens_by_row(r)
    assert any(t[0] == "match" and t[2] > at for row in rows[1:r["h"]] for t, at in row)


def test_broken_candidates_get_the_serial_status():
    px, status, path, _, _ = rc.decode_rows_host(rc.broken_base())
    assert status == pc.OK and path == rc.ROWS
    paths = {}
    for name, data in BROKEN:
        _, status, paths[name], _, _ = rc.decode_rows_host(data)
        assert status == rc.serial_status(data) == pc.CORRUPT, name
    assert paths["wrong-adler"] == rc.ROWS and paths["bfinal-in-row-3"] == rc.REFUSED     # the unfilter's check; the row rule


def test_coverage_conditions():
    """What the framed files must exercise, asserted from the model's token lists and the tables."""
    starts, row_kinds, per_row = set(), [], []
    for name, data in FRAMED:
        table = rc.expected_table(data)
        starts |= {v % 4 for v in table[:-1]}
        r = rc.model(data)
        if "tokens" in r:
            per_row += rc.tokens_by_row(r)[:r["h"]]
            row_kinds += [set(k) for k in rc.blocks_by_row(r, table)[:r["h"]]]
    assert starts == {0, 1, 2, 3}                                                   # rows beginning at every offset in a word
    assert any(len(row) > 64 for row in per_row)                                    # more tokens than one round takes
    matches = [t for row in per_row for t, _ in row if t[0] == "match"]
    assert any(t[2] < t[1] for t in matches) and any(1 < t[2] < t[1] for t in matches)     # a distance shorter than the length
    assert any(t[1] == 258 for t in matches)
    assert {"stored"} in row_kinds and {"fixed", "stored"} in row_kinds and any("dynamic" in k for k in row_kinds)
    assert any(k == {"fixed", "dynamic", "stored"} for k in row_kinds)              # a row of several blocks
    stored = [t for row in per_row for t, _ in row if t[0] == "stored"]
    assert any(t[1] > 0 for t in stored) and any(t[1] == 0 for t in stored)         # a last stored block that carries bytes
    shapes = {(rc.model(data)["h"], rc.model(data)["w"]) for _, data in FRAMED}
    assert {(h, w) for h in (1, 2, 65) for w in (1, 7, 86, 640)} | {(3, 4096), (2, 8192)} <= shapes
    kinds = {(rc.model(data)["c"], rc.model(data)["depth"]) for _, data in FRAMED}
    assert kinds == {(1, 8), (3, 8), (4, 8), (1, 16)}
    assert max(len(rc.model(data)["inflated"]) // rc.model(data)["h"] for _, data in FRAMED) == 32769


def test_table_checks_of_the_host_half():
    lib = _lib.load()
    name, data = FRAMED[-1]
    d, _, _ = pc.parse_host(data)
    good = rc.row_table_host(data, d)
    descs = (_lib.PngDesc * 2)(d, pc.parse_host(pc.corpus()[0][1])[0])             # a candidate and a file that is none

    def query(table, words=None, ds=descs, n=2):
        t = np.ascontiguousarray(table, dtype=np.uint32)
        return lib.cgan_png_decode_rows_workspace_bytes(C.addressof(ds), t.ctypes.data, len(t) if words is None else words, n)

    assert query(good) > lib.cgan_png_decode_workspace_bytes(C.addressof(descs), 2) > 0
    descending, outside, early = good.copy(), good.copy(), good.copy()
    descending[3] = descending[2]
    outside[-1] = d.stream_bytes + 1
    early[0] = 0
    for what, table in (("descending", descending), ("out of range", outside), ("in front of the header", early)):
        assert query(table) == 0 and b"file 0" in lib.cgan_last_error(), what
    assert query(good[:-1]) == 0 and query(np.append(good, good[-1] + 1)) == 0     # fewer and more words than rows + 1
    assert query(good, ds=(_lib.PngDesc * 2)(descs[1], descs[1])) == 0             # a table and no candidate
    wrong = (_lib.PngDesc * 2)(d, descs[1])
    wrong[0].rows = d.height - 1                                                    # rows is the height or 0
    assert query(good[:-1], ds=wrong) == 0
    assert lib.cgan_png_decode_rows_workspace_bytes(C.addressof(descs), None, 0, 2) == 0
    none = (_lib.PngDesc * 1)(descs[1])
    assert lib.cgan_png_decode_rows_workspace_bytes(C.addressof(none), None, 0, 1) > 0
    # the table entry wants the file's own descriptor, and a candidate's
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    out = np.zeros(d.rows + 1, dtype=np.uint32)
    assert lib.cgan_png_row_table_host(buf.ctypes.data, len(data), C.addressof(descs[1]), out.ctypes.data) != 0
    other = type(d).from_buffer_copy(d)
    other.stream_bytes += 1
    assert lib.cgan_png_row_table_host(buf.ctypes.data, len(data), C.addressof(other), out.ctypes.data) != 0
    # and the twin refuses a table that is not the descriptor's
    stream = np.frombuffer(pc.stream_host(data, d), dtype=np.uint8).copy()
    scratch, status, path = np.zeros(d.height * (1 + d.width), dtype=np.uint8), C.c_int32(0), C.c_int32(0)
    assert lib.cgan_png_decode_rows_host(stream.ctypes.data, C.addressof(d), outside.ctypes.data, scratch.ctypes.data,
                                         scratch.ctypes.data, C.addressof(status), C.addressof(path)) != 0


def test_probe_exposes_rows():
    from climategan_amd import png

    d, why = png.probe(FRAMED[-1][1])
    assert why is None and d.rows == d.height == 6
    assert png.probe(pc.corpus()[0][1])[0].rows == 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no compiler")
def test_row_path_under_sanitizers(tmp_path):
    """tools/png_rows_asan.cpp (its own ``main``, the core header and nothing of the GPU) built with
    -fsanitize=address,undefined and run over the framed, refused and broken files and every eighth corpus file."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "png_rows_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "climategan_amd" / "csrc"),
                    str(ROOT / "tools" / "png_rows_asan.cpp"), "-o", str(exe)], check=True, timeout=120)
    plain = [(name, data) for name, data in pc.corpus()[::8] if pc.parse_host(data)[0].rows == 0]
    files = list(FRAMED) + list(REFUSED) + list(BROKEN) + plain + list(pc.unsupported_files())
    for k, (_, data) in enumerate(files):
        (tmp_path / ("f%03d.png" % k)).write_bytes(data)
    out = subprocess.run([str(exe)] + sorted(str(p) for p in tmp_path.glob("f*.png")), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    paths = [rc.decode_rows_host(data)[2] for _, data in BROKEN]                   # a changed byte may or may not break the row rule
    assert ("%d files: %d by rows, %d serial, %d serial after a refusal, %d of them with a status from the decode, %d refused" % (
        len(files), len(FRAMED) + paths.count(rc.ROWS), len(plain), len(REFUSED) + paths.count(rc.REFUSED), len(BROKEN),
        len(pc.unsupported_files()))) in out.stdout
