"""The device PNG encoder's bytes, pinned.  The other PNG tests decode the files, so a changed filter choice, block choice or
token coding that still decodes passes them; the encoder is integer arithmetic only, so its files are a fixed function of
the pixels, and tests/golden/png_bytes.json holds, per (shape, level), the files' lengths, one SHA-256 over the concatenated
files and a SHA-256 of the input array.  The fixture was recorded with the build of the commit before csrc/row_files.h
(``python tests/test_gpu_png_bytes.py`` in that checkout rewrites it): it pins the encoder as it was, not as it is.

Shapes: ``test_gpu_png.test_container``'s (every token kind, both 258-byte edge widths) and the two images of
``test_round_trip_at_the_limits`` at (300, 7, 3) -- two tiles of the row-offset scan -- and (2, 4096, 3) -- the widest row."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

if __name__ == "__main__":                                # record mode runs without the suite's conftest
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from test_gpu_png import contents  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "png_bytes.json"
CONTAINER = [(1, 1, 1), (3, 87, 3), (17, 89, 3), (17, 640, 1), (2, 86, 3)]
LIMITS = [(300, 7, 3), (2, 4096, 3)]


def images(h, w, c):
    if (h, w, c) in CONTAINER:
        return contents(h, w, c, seed=7)
    rng = np.random.default_rng(w + c)                    # test_round_trip_at_the_limits' two images
    return np.stack([rng.integers(0, 256, (h, w, c)), np.full((h, w, c), 31)]).astype(np.uint8)


def digests(h, w, c, level):
    from climategan_amd import png

    imgs = np.ascontiguousarray(images(h, w, c))
    files = png.encode(torch.from_numpy(imgs).cuda(), level=level)
    return {"input_sha256": hashlib.sha256(imgs.tobytes()).hexdigest(), "lengths": [len(b) for b in files],
            "files_sha256": hashlib.sha256(b"".join(files)).hexdigest()}


@pytest.fixture(scope="module")
def pinned():
    return json.loads(FIXTURE.read_text())


@pytest.mark.parametrize("level", (1, 2))
@pytest.mark.parametrize("h,w,c", CONTAINER + LIMITS)
def test_bytes_are_the_recorded_ones(pinned, h, w, c, level):
    want = pinned["%d,%d,%d,%d" % (h, w, c, level)]
    got = digests(h, w, c, level)
    assert got["input_sha256"] == want["input_sha256"], "the test images changed, not the encoder"
    assert got["lengths"] == want["lengths"]
    assert got["files_sha256"] == want["files_sha256"]


def test_one_pinned_buffer_serves_both_encoders():
    """png.encode, jpeg.encode and png.encode again fetch through the same pinned buffer: the PNG files come out the same, and
    the ``bytes`` handed out earlier are copies that the later calls leave alone."""
    from climategan_amd import jpeg, png

    x = torch.from_numpy(contents(17, 89, 3, seed=7)).cuda()
    first = png.encode(x)
    kept = [bytes(bytearray(b)) for b in first]           # copies of the values in memory of their own
    jpegs = jpeg.encode(x)
    jpegs_kept = [bytes(bytearray(b)) for b in jpegs]
    assert png.encode(x) == first
    assert first == kept and jpegs == jpegs_kept
    assert all(b[:8] == b"\x89PNG\r\n\x1a\n" for b in first) and all(b[:2] == b"\xff\xd8" for b in jpegs)


if __name__ == "__main__":                                # record mode: the fixture from whatever build this checkout has
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else FIXTURE
    rec = {"%d,%d,%d,%d" % (h, w, c, level): digests(h, w, c, level) for h, w, c in CONTAINER + LIMITS for level in (1, 2)}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print("recorded %d cases to %s" % (len(rec), out))
