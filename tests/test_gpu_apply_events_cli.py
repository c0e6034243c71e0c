"""``python -m climategan_amd.apply_events`` end to end on a small saved run: the files it writes (device-encoded PNGs)
decode to exactly what ``Trainer.infer_all(numpy=True)`` returns in this process for the same batch."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent
SIZE = 256                      # the wildfire's 281-tap reflect-border blur needs more than 140 pixels: 128 is too small


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    """A run directory (opts.yaml + checkpoints/) of the small fixture's options with every inference task."""
    import yaml

    from climategan_amd.config import Opts
    from climategan_amd.trainer import Trainer

    o = Opts(yaml.safe_load((ROOT / "golden" / "ckpt_small" / "opts.yaml").read_text()))
    o.tasks = ["d", "s", "m", "p"]
    run = tmp_path_factory.mktemp("apply") / "run"
    o.output_path = str(run)
    T = Trainer(o, device="cuda").setup(inference=True)
    (run / "checkpoints").mkdir(parents=True)
    torch.save({"G": T.G.state_dict()}, run / "checkpoints" / "latest_ckpt.pth")
    (run / "opts.yaml").write_text(yaml.safe_dump(json.loads(json.dumps(o))))
    return run


def photo(rng, h, w):
    """Smooth colour gradients plus noise: something for every event to work on."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (h + w)], axis=-1)
    return np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)


def run_cli(*args):
    cmd = [sys.executable, "-m", "climategan_amd.apply_events"] + [str(a) for a in args]
    out = subprocess.run(cmd, cwd=str(ROOT.parent), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def test_cli_end_to_end(run_dir, tmp_path):
    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.eval_masker import find_images
    from climategan_amd.trainer import Trainer

    rng = np.random.default_rng(21)
    (tmp_path / "imgs").mkdir()
    for i, (h, w) in enumerate(((300, 400), (520, 410), (256, 700))):
        Image.fromarray(photo(rng, h, w)).save(tmp_path / "imgs" / ("im%d.png" % i))
    out_dir = tmp_path / "out"
    out = run_cli("-i", tmp_path / "imgs", "-r", run_dir, "-b", 3, "-t", SIZE, "--save_masks", "-s", "-o", out_dir,
                  "--overwrite", "--no_cloudy")
    assert "Unit: s/batch" in out.stdout                               # the timing table
    paths = find_images(tmp_path / "imgs")                             # the order the command processes them in
    events = ("flood", "wildfire", "smog", "mask", "input")
    expected = {"%s_%s_%d_no_cloudy.png" % (p.stem, e, SIZE) for p in paths for e in events}
    assert {p.name for p in out_dir.iterdir()} == expected | {"command.txt", "hash.txt"}
    assert "apply_events" in (out_dir / "command.txt").read_text()

    R = Trainer.resume_from_path(run_dir, inference=True, new_exp=None, device="cuda")
    x = prepare_batch([np.asarray(Image.open(p)) for p in paths], to=SIZE)
    want = R.infer_all(x, numpy=True, bin_value=0.5, cloudy=False, return_masks=True)
    want["mask"] = want["mask"][:, 0]
    want["input"] = ((x.cpu().numpy() + 1) / 2 * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    for i, p in enumerate(paths):
        for e in events:
            got = np.asarray(Image.open(out_dir / ("%s_%s_%d_no_cloudy.png" % (p.stem, e, SIZE))))
            assert got.shape == want[e][i].shape, (p.name, e, got.shape)
            assert np.array_equal(got, want[e][i]), (p.name, e)
    # an existing directory is refused without --overwrite, and nothing prompts
    cmd = [sys.executable, "-m", "climategan_amd.apply_events", "-i", str(tmp_path / "imgs"), "-r", str(run_dir), "-o",
           str(out_dir)]
    again = subprocess.run(cmd, cwd=str(ROOT.parent), capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert again.returncode != 0 and "already exists" in again.stderr


def test_cli_keep_ratio(run_dir, tmp_path):
    from climategan_amd.apply_events import to_128

    (tmp_path / "imgs").mkdir()
    img = photo(np.random.default_rng(22), 620, 300)
    Image.fromarray(img).save(tmp_path / "imgs" / "tall.png")
    out_dir = tmp_path / "out"
    run_cli("-i", tmp_path / "imgs", "-r", run_dir, "--keep_ratio_128", "-m", 256, "-o", out_dir, "--no_cloudy", "--no_time",
            "--no_conf")
    nh, nw = to_128(img, 256)
    assert (nh, nw) == (512, 256)
    assert {p.name for p in out_dir.iterdir()} == {"tall_%s_256_AR_no_cloudy.png" % e for e in ("flood", "wildfire", "smog")}
    for p in out_dir.iterdir():
        assert np.asarray(Image.open(p)).shape == (nh, nw, 3)
