"""``python -m climategan_amd.apply_events --decode device`` end to end on a small saved run, one folder with a 4:2:0 and a
4:4:4 baseline JPEG, a progressive JPEG and a PNG: the baseline files' outputs are those of the pipeline run in this process on
``jpeg.decode``'s tensors, the other two files' outputs are byte for byte those of a run without the option, and that run lists
its arguments as before.  (The wildfire's green level is drawn anew per process: its files are left out of the comparisons.)"""
import numpy as np
import pytest
from PIL import Image

from test_gpu_apply_events_jpeg_cli import ARGS_BEFORE, SIZE, run_cli, run_dir  # noqa: F401  (run_dir: the fixture)

pytestmark = pytest.mark.gpu
EVENTS = ("flood", "smog", "input", "mask")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    rng = np.random.default_rng(29)
    d = tmp_path_factory.mktemp("mixed")
    for name, (h, w), kw in (("a_420.jpg", (300, 400), dict(quality=90, subsampling=2)),
                             ("b_444.jpg", (256, 520), dict(quality=95, subsampling=0, optimize=True)),
                             ("c_progressive.jpg", (280, 300), dict(quality=90, progressive=True)),
                             ("d.png", (270, 310), {})):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (h + w)], axis=-1)
        Image.fromarray(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)).save(d / name, **kw)
    return d


def test_decode_device(run_dir, folder, tmp_path):  # noqa: F811
    from climategan_amd import jpeg
    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.eval_masker import find_images
    from climategan_amd.trainer import Trainer

    common = ["-i", folder, "-r", run_dir, "-b", 4, "-t", SIZE, "--save_masks", "-s", "--no_cloudy", "--no_time", "--no_conf"]
    dev = run_cli(*common, "-o", tmp_path / "device", "--decode", "device")
    assert dev.returncode == 0, dev.stderr[-3000:]
    host = run_cli(*common, "-o", tmp_path / "host")
    assert host.returncode == 0, host.stderr[-3000:]
    listing = host.stdout.split("Using args\n\n")[1].split("\n\n")[0]
    assert [line.split(":")[0].strip() for line in listing.splitlines()] == ARGS_BEFORE
    assert "decode" in dev.stdout.split("Using args\n\n")[1].split("\n\n")[0]
    names = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "device").iterdir()) and len(names) == 4 * 5

    def written(run, stem, event):
        return (tmp_path / run / ("%s_%s_%d_no_cloudy.png" % (stem, event, SIZE))).read_bytes()

    for stem in ("c_progressive", "d"):
        for event in EVENTS:
            assert written("device", stem, event) == written("host", stem, event), (stem, event)

    paths = find_images(folder)                                        # the command's own order
    baseline = [i for i, p in enumerate(paths) if jpeg.probe(p.read_bytes())[0] is not None]
    assert sorted(paths[i].name for i in baseline) == ["a_420.jpg", "b_444.jpg"] and len(paths) == 4
    images = [np.asarray(Image.open(p)) for p in paths]
    for i, im in zip(baseline, jpeg.decode([paths[i] for i in baseline])):
        images[i] = im
    R = Trainer.resume_from_path(run_dir, inference=True, new_exp=None, device="cuda")
    x = prepare_batch(images, to=SIZE)
    want = R.infer_all(x, numpy=True, bin_value=0.5, cloudy=False, return_masks=True, ignore_event={"wildfire"})
    want["input"] = ((x.cpu().numpy() + 1) / 2 * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    for i in baseline:
        p = paths[i]
        for event in EVENTS:
            got = np.asarray(Image.open(tmp_path / "device" / ("%s_%s_%d_no_cloudy.png" % (p.stem, event, SIZE))))
            ref = want[event][i, 0] if event == "mask" else want[event][i]
            assert np.array_equal(got, ref), (p.name, event)
