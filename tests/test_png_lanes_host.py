"""The lane-parallel inflate's host side, no GPU: the window rule in Python (``tests/png_lanes_model.py``) against
the serial model's token list, ``cgan_png_inflate_lanes_host`` (csrc/png_decode_core.h's ``decode_subseq`` lane by lane and
pass by pass) against ``zlib.decompress`` and the model's statistics at subsequences of 32 bits / 4 tokens, 64 / 8 and the
compiled defaults, its status on every broken file against ``cgan_png_decode_host``'s, the conditions that make the hand-built
files of ``tests/png_lanes_cases.py`` what their names say, and the refusals.  Everything is integer: the tolerance is 0."""
import ctypes as C
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import png_decode_corpus as pc
import png_lanes_cases as lc
import png_lanes_model as lm
from climategan_amd import _lib, png

ROOT = Path(__file__).resolve().parent.parent
CASES = lc.cases()
BROKEN = lc.broken()
SETTINGS = lc.all_settings()
IDS = ["%d-%d" % s for s in SETTINGS]


def stream_of(data):
    d, why = png.probe(data)
    assert d is not None, why
    return png.stream_of(data, d), d


@pytest.mark.parametrize("S,cap", SETTINGS, ids=IDS)
def test_model_commits_the_serial_tokens(S, cap):
    n = 0
    for name, data in CASES:
        if lc.small(data):
            raw, tokens, stats, windows, _ = lc.model(data, S, cap)
            assert raw == pc.model(data)["inflated"] and tokens == pc.model(data)["tokens"], name
            assert 1 <= stats["max_passes"] <= lm.LANES or not windows, name
            n += 1
    assert n >= len(CASES) - 12                                                   # all but the few long files


@pytest.mark.parametrize("S,cap", SETTINGS, ids=IDS)
def test_twin_equals_zlib_and_the_models_statistics(S, cap):
    for name, data in CASES:
        stream, d = stream_of(data)
        inflated, trailer, stats, status, rc = lc.inflate_lanes_host(stream, d, S, cap)
        assert (rc, status) == (0, pc.OK), name
        raw = zlib.decompress(stream)
        assert inflated == raw and trailer == zlib.adler32(raw), name
        assert inflated == pc.decode_host(stream, d)[0], name
        if lc.small(data):
            assert stats == lc.model(data, S, cap)[2], name


def test_serial_form_of_the_twin():
    for name, data in CASES[::7]:
        stream, d = stream_of(data)
        inflated, trailer, stats, status, rc = lc.inflate_lanes_host(stream, d, 0, 1)
        assert (rc, status) == (0, pc.OK) and inflated == zlib.decompress(stream) and not any(stats.values()), name


@pytest.mark.parametrize("S,cap", SETTINGS, ids=IDS)
def test_broken_files_get_the_serial_twins_status(S, cap):
    assert len(BROKEN) == 23 + 25
    for name, data in BROKEN:
        stream, d = stream_of(data)
        _, _, _, status, rc = lc.inflate_lanes_host(stream, d, S, cap)
        assert rc == 0 and status == pc.decode_host(stream, d)[2] == pc.CORRUPT, name
        with pytest.raises(Exception):                                            # and the model refuses it
            r = lm.inflate_lanes(stream, S, cap, d.height * (1 + d.width * d.channels * d.bit_depth // 8))
            pc.pm.unfilter(r[0], d.height, d.width * d.channels * d.bit_depth // 8, d.channels * d.bit_depth // 8)


def test_coverage_conditions():
    """What the hand-built files must exercise, asserted from the model's windows."""
    files = dict(lc.hand_built())

    def windows(name, S, cap):
        return lc.model(files[name], S, cap)

    # a 48-bit token at S = 32: the token exists, and a committed lane had nothing to begin
    tokens = pc.model(files["lanes-48-bit-token"])["tokens"]
    assert ("match", 227, 24577) in tokens
    lit = pc.model(files["lanes-48-bit-token"])["blocks"][0]
    assert lit["longest"] == 15
    assert any(w["empty"] for w in windows("lanes-48-bit-token", 32, 4)[3])
    # an end-of-block symbol in mid-window, then a dynamic, a fixed and a stored block
    _, _, _, wins, blocks = windows("lanes-block-kinds", 32, 4)
    mid = [blocks[w["block"] + 1] for w in wins if w["flag"] == lm.EOB and 1 < w["lanes"] < lm.LANES and w["block"] + 1 < len(blocks)]
    assert {"dynamic", "fixed", "stored"} <= set(mid)
    # the final block ends in lane 0, in lane 63, and exactly where a lane's bits end
    last = {name: windows(name, 32, 4)[3][-1] for name in files if name.startswith("lanes-final")}
    assert all(w["flag"] == lm.EOB for w in last.values())
    assert last["lanes-final-in-lane0"]["lanes"] == 1 and last["lanes-final-in-lane63"]["lanes"] == 64
    w = last["lanes-final-on-boundary"]
    assert w["exit"] == w["start"] + 32 * w["lanes"]
    # a lane that hits its cap, at every setting: 128 tokens in 128 bits
    for S, cap in SETTINGS:
        _, _, stats, wins, _ = windows("lanes-cap", S, cap)
        assert stats["full_windows"] > 0 and any(max(w["counts"]) == cap for w in wins), (S, cap)
    # the bound of 64 passes: a window that needed as many passes as the lanes it committed, all 64
    for S, cap in SETTINGS:
        assert any(w["passes"] == w["lanes"] == lm.LANES for w in windows("lanes-wrong-phase", S, cap)[3]), (S, cap)
    assert all(t == ("lit", 0) or t == ("match", 3, 1) or t == ("lit", 37) for t in pc.model(files["lanes-wrong-phase"])["tokens"])
    # a window that crosses the stream's end, and one that does not
    crossing = [w["crosses_end"] for name, data in CASES if lc.small(data) for w in lc.model(data, 32, 4)[3]]
    assert any(crossing) and not all(crossing)
    # the broken files the commit finds and the ones a committed lane reports
    names = {name for name, _ in BROKEN}
    assert {"distance-too-far", "too-much-output", "too-much-output-match", "literal-286", "distance-30", "cut@9"} <= names


def test_no_window_ends_full_on_pil_files_at_the_defaults():
    S, cap = lc.defaults()
    n = 0
    for name, data in CASES:
        if name.startswith("pil-"):
            stream, d = stream_of(data)
            _, _, stats, status, rc = lc.inflate_lanes_host(stream, d, S, cap)
            assert (rc, status) == (0, pc.OK), name
            assert stats["full_windows"] == 0, (name, stats)
            n += 1
    assert n >= 20


def test_refusals():
    lib = _lib.load()
    _, good = pc.corrupt_streams()
    d = pc.stream_desc(good, 4, 7)
    S, cap = lc.defaults()
    assert (S, cap) == tuple(png.inflate_params()[k] for k in ("subseq_bits", "lane_tokens")) and S % 32 == 0 and S > 0 and cap >= 1
    assert lc.inflate_lanes_host(good, d, S, cap)[3:] == (pc.OK, 0)
    for bits, tokens in ((-32, 4), (16, 4), (33, 4), (288, 4), (32, 0), (32, -1), (32, 49), (0, 0)):
        assert lc.inflate_lanes_host(good, d, bits, tokens)[4] != 0, (bits, tokens)
        assert "subseq_bits" in lib.cgan_last_error().decode()
    assert lc.inflate_lanes_host(good, d, 256, 48)[3:] == (pc.OK, 0)              # the largest values taken
    for field, value in (("width", 8193), ("height", 0), ("channels", 2), ("bit_depth", 4), ("stream_bytes", 1)):
        bad = type(d).from_buffer_copy(d)
        setattr(bad, field, value)
        src, buf, out = np.frombuffer(good, dtype=np.uint8).copy(), np.zeros(64, dtype=np.uint8), (C.c_uint32 * 8)()
        assert lib.cgan_png_inflate_lanes_host(src.ctypes.data, C.addressof(bad), 32, 4, buf.ctypes.data, out, out, out) != 0, field
    assert lib.cgan_png_inflate_lanes_host(None, C.addressof(d), 32, 4, None, None, None, None) != 0
    # the device call refuses the same values before it looks at anything else
    zero = C.c_void_p(0)
    for bits, tokens in ((16, 4), (288, 4), (32, 0), (32, 49)):
        assert lib.cgan_png_decode_lanes(zero, 0, zero, zero, 0, zero, 0, zero, zero, 0, zero, bits, tokens) != 0
        assert "subseq_bits" in lib.cgan_last_error().decode()


@pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="no compiler")
def test_twin_under_sanitizers(tmp_path):
    """tools/png_lanes_asan.cpp (its own ``main``, the core header and nothing of the GPU) built with
    -fsanitize=address,undefined and run as a child process over every fourth case and all broken files."""
    cxx = shutil.which("clang++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "png_lanes_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "climategan_amd" / "csrc"),
                    str(ROOT / "tools" / "png_lanes_asan.cpp"), "-o", str(exe)], check=True, timeout=120)
    files = list(CASES[::4]) + list(lc.hand_built()) + list(BROKEN)
    for k, (_, data) in enumerate(files):
        (tmp_path / ("f%03d.png" % k)).write_bytes(data)
    out = subprocess.run([str(exe)] + sorted(str(p) for p in tmp_path.glob("f*.png")), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "%d files: %d decoded, %d with a status from the decode, 0 refused" % (
        len(files), len(files) - len(BROKEN), len(BROKEN)) in out.stdout
