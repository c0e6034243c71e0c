"""``python -m climategan_amd.apply_events --decode device`` end to end on a small saved run, one folder with an RGB PNG, an
RGBA PNG, an interlaced PNG and a baseline JPEG: the run with the option writes byte for byte what the run without it writes
(PNG pixels are PIL's on either path, and the JPEG decoder's are PIL's too on this file), and ``read_images`` hands the RGB PNG
to the device and leaves the other two PNG files to the host.  (The wildfire's green level is drawn anew per process: its files
are left out of the comparison.)"""
import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_model as pm
from test_gpu_apply_events_jpeg_cli import SIZE, run_cli, run_dir  # noqa: F401  (run_dir: the fixture)

pytestmark = pytest.mark.gpu
EVENTS = ("flood", "smog", "input", "mask")


def photo(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (h + w)], axis=-1)
    return np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    rng = np.random.default_rng(31)
    d = tmp_path_factory.mktemp("pngs")
    Image.fromarray(photo(rng, 270, 310)).save(d / "a_rgb.png")
    rgba = np.concatenate([photo(rng, 256, 300), rng.integers(0, 256, (256, 300, 1)).astype(np.uint8)], axis=-1)
    Image.fromarray(rgba).save(d / "b_rgba.png")
    (d / "c_interlaced.png").write_bytes(pm.write_interlaced(photo(rng, 260, 280)))
    Image.fromarray(photo(rng, 300, 400)).save(d / "d_444.jpg", quality=95, subsampling=0)
    return d


def test_read_images(folder):
    from climategan_amd.apply_events import read_image, read_images
    from climategan_amd.eval_masker import find_images

    paths = sorted(find_images(folder), key=lambda p: p.name)
    assert [p.name for p in paths] == ["a_rgb.png", "b_rgba.png", "c_interlaced.png", "d_444.jpg"]
    images = read_images(paths, decode="device")
    assert [isinstance(im, torch.Tensor) for im in images] == [True, False, False, True]
    assert images[0].is_cuda and images[0].dtype == torch.uint8
    for p, im in zip(paths[:3], images[:3]):
        assert np.array_equal(im.cpu().numpy() if isinstance(im, torch.Tensor) else im, read_image(p)), p.name
    assert all(isinstance(im, np.ndarray) for im in read_images(paths))                 # the default reads on the host


def test_decode_device_writes_the_host_runs_files(run_dir, folder, tmp_path):  # noqa: F811
    common = ["-i", folder, "-r", run_dir, "-b", 4, "-t", SIZE, "--save_masks", "-s", "--no_cloudy", "--no_time", "--no_conf"]
    dev = run_cli(*common, "-o", tmp_path / "device", "--decode", "device")
    assert dev.returncode == 0, dev.stderr[-3000:]
    host = run_cli(*common, "-o", tmp_path / "host")
    assert host.returncode == 0, host.stderr[-3000:]
    names = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "device").iterdir()) and len(names) == 4 * 5
    for stem in ("a_rgb", "b_rgba", "c_interlaced", "d_444"):
        for event in EVENTS:
            name = "%s_%s_%d_no_cloudy.png" % (stem, event, SIZE)
            assert (tmp_path / "device" / name).read_bytes() == (tmp_path / "host" / name).read_bytes(), name
