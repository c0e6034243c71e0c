"""``python -m climategan_amd.repack_png`` on a small tree: the RGB and the grey file come out row-framed with PIL's
pixels unchanged, everything else byte for byte, the summary counts, and the refusal of an existing output folder."""
import io
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import jpeg_model as jm
import png_decode_corpus as pc
from climategan_amd import png

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run(*args):
    return subprocess.run([sys.executable, "-m", "climategan_amd.repack_png", *args], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_repack_a_tree(tmp_path):
    src, dst = tmp_path / "src", tmp_path / "dst"
    (src / "sub").mkdir(parents=True)
    rgb, grey = jm.make_image("sinusoid", 40, 56, 3), jm.make_image("noise", 40, 56, 1)
    files = {"a.png": pc.pil_file(rgb), "sub/m.png": pc.pil_file(grey),
             "sub/rgba.png": pc.pil_file(pc.as_mode(rgb, "RGBA")), "deep.png": pc.pil_file(pc.as_mode(grey, "I;16")),
             "sub/labels.json": b'{"a": 1}\n'}
    for name, data in files.items():
        (src / name).write_bytes(data)
    out = run("-i", str(src), "-o", str(dst))
    assert out.returncode == 0, out.stdout + out.stderr
    assert sorted(str(p.relative_to(dst)) for p in dst.rglob("*") if p.is_file()) == sorted(files)
    for name, want in (("a.png", rgb), ("sub/m.png", grey)):
        new = (dst / name).read_bytes()
        assert new != files[name]
        d, why = png.probe(new)
        assert why is None and d.rows == d.height == 40
        got = np.asarray(Image.open(io.BytesIO(new)))
        assert np.array_equal(got.reshape(want.shape), want) and np.array_equal(got, np.asarray(Image.open(io.BytesIO(files[name]))))
    for name in ("sub/rgba.png", "deep.png", "sub/labels.json"):
        assert (dst / name).read_bytes() == files[name], name
    before, after = (sum(len(d[n]) for n in ("a.png", "sub/m.png")) for d in (files, {n: (dst / n).read_bytes() for n in files}))
    text = out.stdout
    assert "2 repacked at level 2 (%d -> %d bytes), 3 copied" % (before, after) in text
    assert "1 16-bit" in text and "1 4 channels" in text and "1 not a .png" in text
    # an output folder that exists is refused, and so is one inside the input
    # (the same entry in this process: one start of the interpreter is what the test above is about)
    from climategan_amd import repack_png

    with pytest.raises(SystemExit, match="exists"):
        repack_png.main(["-i", str(src), "-o", str(dst)])
    with pytest.raises(SystemExit, match="inside"):
        repack_png.main(["-i", str(src), "-o", str(src / "out")])
    with pytest.raises(SystemExit, match="inside"):
        repack_png.main(["-i", str(src), "-o", str(src)])
    assert not (src / "out").exists()
    assert repack_png.main(["-i", str(src), "-o", str(dst), "--overwrite", "--level", "1", "-b", "1"]) == 0
    assert png.probe((dst / "a.png").read_bytes())[0].rows == 40
    assert (dst / "deep.png").read_bytes() == files["deep.png"]
