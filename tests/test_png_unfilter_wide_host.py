"""The wide unfilter's schedule on the host, no GPU: ``cgan_png_unfilter_wide_host`` runs the multi-wave
kernel's schedule -- csrc/png_decode_core.h's ``unf_*`` functions, chunk by chunk, wave by wave, lane by lane -- with every
ring and ``above`` slot stamped by the chunk that wrote it, over the shape list of ``png_unfilter_wide_cases``: 1, 2, 4 and 16
waves, a lag of one and of two prefetches.  Its pixels must be the source array's and the serial twin's, its status the serial
twin's, and no read may cross a barrier the wrong way (CGAN_ERR_INTERNAL).  Every stage is integer: the tolerance is 0."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import png_decode_corpus as pc
import png_unfilter_wide_cases as wc
from climategan_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
COMBOS = [(nw, k) for nw in wc.WAVES for k in wc.LAGS_IN_PREFETCHES]
IDS = ["waves%d-lag%dp" % c for c in COMBOS]


def test_compiled_parameters_are_ones_the_schedule_takes():
    nw, lag, prefetch = wc.compiled()
    assert nw in (4, 8, 16) and prefetch >= 2 and lag >= prefetch and lag % prefetch == 0


@pytest.mark.parametrize("nw,k", COMBOS, ids=IDS)
def test_wide_twin_equals_the_source_and_the_serial_twin(nw, k):
    lag = k * wc.prefetch()
    cases = wc.files(nw, lag)
    assert {(img.shape[0], img.shape[1]) for _, img, _ in cases} >= {(h, w) for h in wc.heights(nw) for w in wc.widths(lag)}
    assert {(img.shape[2], img.dtype.itemsize) for _, img, _ in cases} == {(1, 1), (3, 1), (4, 1), (1, 2)}
    for name, img, data in cases:
        px, status, code, serial_px, serial_status = wc.wide_host(data, nw, lag)
        assert code == 0, (name, _lib.load().cgan_last_error())                    # no schedule violation
        assert status == serial_status == pc.OK, name
        assert px.dtype == img.dtype and np.array_equal(px, img) and np.array_equal(px, serial_px), name


@pytest.mark.parametrize("nw,k", COMBOS, ids=IDS)
def test_broken_files_get_the_serial_twins_status(nw, k):
    lag = k * wc.prefetch()
    for name, data in wc.broken(nw, lag):
        _, status, code, _, serial_status = wc.wide_host(data, nw, lag)
        assert code == 0 and status == serial_status == pc.CORRUPT, name


def test_the_chunk_count_is_the_same_for_every_wave():
    """The twin walks ``chunks`` chunks in every pass for every wave (the loop bound is one number per file); what has to hold
    is that this number is enough for the last wave and lane: the last step of the last wave's last lane is inside it."""
    prefetch = wc.prefetch()
    for nw in wc.WAVES:
        for lag in wc.lags():
            for w in wc.widths(lag) + (8192,):
                steps = w + 63 + (nw - 1) * (64 + lag)
                chunks = -(-steps // prefetch)
                last = (nw - 1) * (64 + lag) + 63 + (w - 1)                        # wave nw - 1, lane 63, pixel w - 1
                assert last < chunks * prefetch and last >= (chunks - 1) * prefetch
                # a read crosses a wave boundary lag + 1 steps behind its write: at least one chunk boundary between them
                assert all((s + lag + 1) // prefetch > s // prefetch for s in range(4 * prefetch))


def test_refused_arguments():
    lib = _lib.load()
    _, img, data = wc.tiny()
    d, _, _ = pc.parse_host(data)
    buf, status = np.zeros(16, dtype=np.uint8), C.c_int32(0)
    prefetch = wc.prefetch()
    for nw, lag in ((0, prefetch), (17, prefetch), (4, 0), (4, prefetch + 1), (4, prefetch // 2)):
        assert lib.cgan_png_unfilter_wide_host(C.addressof(d), buf.ctypes.data, 0, nw, lag, buf.ctypes.data, C.addressof(status)) == -1, (nw, lag)
    assert lib.cgan_png_unfilter_wide_host(None, buf.ctypes.data, 0, 4, prefetch, buf.ctypes.data, C.addressof(status)) == -1


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no compiler")
def test_wide_schedule_under_sanitizers(tmp_path):
    """tools/png_unfilter_wide_asan.cpp (its own ``main``, the core header and nothing of the GPU) built with
    -fsanitize=address,undefined and run over the same shape list, once per (waves, lag)."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "png_unfilter_wide_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "climategan_amd" / "csrc"),
                    str(ROOT / "tools" / "png_unfilter_wide_asan.cpp"), "-o", str(exe)], check=True, timeout=120)
    written = {}
    for nw, k in COMBOS:
        lag = k * wc.prefetch()
        cases = [(name, data) for name, _, data in wc.files(nw, lag)] + list(wc.broken(nw, lag))
        paths = []
        for name, data in cases:
            if data not in written:
                written[data] = tmp_path / ("f%04d.png" % len(written))
                written[data].write_bytes(data)
            paths.append(str(written[data]))
        out = subprocess.run([str(exe), str(nw), str(lag)] + paths, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert ("waves %d, lag %d: %d files: %d equal to the serial twin, %d corrupt in both, 0 not inflated" % (
            nw, lag, len(cases), len(cases) - 3, 3)) in out.stdout
