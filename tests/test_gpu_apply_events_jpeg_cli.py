"""``python -m climategan_amd.apply_events --format jpg`` end to end on a small saved run: events and input come out as the
device encoder's JPEG files (``jpeg.encode`` of what ``Trainer.infer_all`` returns in this process, byte for byte), the
masks stay PNG and decode exactly, and a run without the new options names its files and lists its arguments as before."""
import io
import json
import subprocess
import sys
from pathlib import Path
from unittest import mock

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent
SIZE = 256                      # the wildfire's 281-tap reflect-border blur needs more than 140 pixels: 128 is too small
# what "Using args" listed before --format and the --jpeg_* options existed
ARGS_BEFORE = ["batch_size", "images_paths", "output_path", "save_input", "resume_path", "no_time", "flood_mask_binarization",
               "target_size", "half", "n_images", "no_conf", "overwrite", "no_cloudy", "keep_ratio_128", "fuse", "save_masks",
               "max_im_width", "zip_outdir", "dtype"]


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory (opts.yaml + checkpoints/) of the small fixture's options with every inference task."""
    import yaml

    from climategan_amd.config import Opts
    from climategan_amd.trainer import Trainer

    o = Opts(yaml.safe_load((ROOT / "golden" / "ckpt_small" / "opts.yaml").read_text()))
    o.tasks = ["d", "s", "m", "p"]
    run = tmp_path_factory.mktemp("apply_jpeg") / "run"
    o.output_path = str(run)
    T = Trainer(o, device="cuda").setup(inference=True)
    (run / "checkpoints").mkdir(parents=True)
    torch.save({"G": T.G.state_dict()}, run / "checkpoints" / "latest_ckpt.pth")
    (run / "opts.yaml").write_text(yaml.safe_dump(json.loads(json.dumps(o))))
    return run


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    rng = np.random.default_rng(23)
    d = tmp_path_factory.mktemp("photos")
    for i, (h, w) in enumerate(((300, 400), (256, 520))):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (h + w)], axis=-1)
        Image.fromarray(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)).save(d / ("im%d.png" % i))
    return d


def run_cli(*args):
    cmd = [sys.executable, "-m", "climategan_amd.apply_events"] + [str(a) for a in args]
    return subprocess.run(cmd, cwd=str(ROOT.parent), capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)


def test_format_jpg(run_dir, photos, tmp_path):
    from climategan_amd import jpeg
    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.eval_masker import find_images
    from climategan_amd.trainer import Trainer

    out_dir = tmp_path / "out"
    out = run_cli("-i", photos, "-r", run_dir, "-b", 2, "-t", SIZE, "--save_masks", "-s", "-o", out_dir, "--no_cloudy",
                  "--no_time", "--format", "jpg", "--jpeg_quality", 75, "--jpeg_subsampling", 420)
    assert out.returncode == 0, out.stderr[-3000:]
    paths = find_images(photos)
    lossy = ("flood", "wildfire", "smog", "input")
    expected = {"%s_%s_%d_no_cloudy.jpg" % (p.stem, e, SIZE) for p in paths for e in lossy}
    expected |= {"%s_mask_%d_no_cloudy.png" % (p.stem, SIZE) for p in paths}
    assert {p.name for p in out_dir.iterdir()} == expected | {"command.txt", "hash.txt"}
    listing = out.stdout.split("Using args")[1]
    assert "format" in listing and "jpeg_quality" in listing and "jpeg_subsampling" in listing

    R = Trainer.resume_from_path(run_dir, inference=True, new_exp=None, device="cuda")
    x = prepare_batch([np.asarray(Image.open(p)) for p in paths], to=SIZE)
    want = R.infer_all(x, numpy=True, bin_value=0.5, cloudy=False, return_masks=True)
    want["input"] = ((x.cpu().numpy() + 1) / 2 * 255).astype(np.uint8).transpose(0, 2, 3, 1)

    def encoded(array):
        return jpeg.encode(torch.from_numpy(np.ascontiguousarray(array)).cuda(), quality=75, subsampling="420")

    written = {e: [(out_dir / ("%s_%s_%d_no_cloudy.jpg" % (p.stem, e, SIZE))).read_bytes() for p in paths] for e in lossy}
    for e in lossy:
        for data in written[e]:
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.format == "JPEG" and im.size == (SIZE, SIZE) and im.mode == "RGB"
        if e != "wildfire":
            assert written[e] == encoded(want[e]), e
    # the wildfire filter's green level is one ``random.randint(100, 150)`` per batch (compute_fire, as in the reference), drawn
    # anew in the command's process: its files are those of one of the 51 levels
    levels = []
    for green in range(100, 151):
        with mock.patch("random.randint", return_value=green):
            fire = R.infer_all(x, numpy=True, bin_value=0.5, cloudy=False, ignore_event={"flood", "smog"})["wildfire"]
        if encoded(fire) == written["wildfire"]:
            levels.append(green)
    assert levels, "the wildfire files are not those of any green level"
    for i, p in enumerate(paths):
        got = np.asarray(Image.open(out_dir / ("%s_mask_%d_no_cloudy.png" % (p.stem, SIZE))))
        assert np.array_equal(got, want["mask"][i, 0]), p.name


def test_default_run_is_unchanged(run_dir, photos, tmp_path):
    from climategan_amd.eval_masker import find_images

    first = find_images(photos)[0].stem                                # -n 1: the first in the command's own order
    out_dir = tmp_path / "out"
    out = run_cli("-i", photos, "-r", run_dir, "-b", 2, "-t", SIZE, "-n", 1, "-o", out_dir, "--no_cloudy", "--no_time",
                  "--no_conf")
    assert out.returncode == 0, out.stderr[-3000:]
    assert {p.name for p in out_dir.iterdir()} == {"%s_%s_%d_no_cloudy.png" % (first, e, SIZE) for e in ("flood", "wildfire", "smog")}
    listing = out.stdout.split("Using args\n\n")[1].split("\n\n")[0]
    assert [line.split(":")[0].strip() for line in listing.splitlines()] == ARGS_BEFORE
    for p in out_dir.iterdir():
        assert Image.open(p).format == "PNG"


def test_jpeg_options_need_format_jpg(photos):
    out = run_cli("-i", photos, "--jpeg_quality", 80)      # the other combinations: test_jpeg_host.py, on the parser alone
    assert out.returncode == 2 and "need --format jpg" in out.stderr, out.stderr[-500:]
