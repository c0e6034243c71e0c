"""The host logic of ``python -m climategan_amd.apply_events`` (no GPU): arguments, size rules, names, the RGBA blend.
The expected strings are written out by hand from the reference's apply_events.py:308-327, 407-429, 479-485, 590-616."""
import numpy as np
import pytest

from climategan_amd import apply_events as ae


def test_parse_args_defaults():
    a = ae.parse_args(["-i", "photos"])
    assert vars(a) == dict(batch_size=4, images_paths="photos", output_path=None, save_input=False, resume_path=None,
                           no_time=False, flood_mask_binarization=0.5, target_size=640, half=False, n_images=-1,
                           no_conf=False, overwrite=False, no_cloudy=False, keep_ratio_128=False, fuse=False,
                           save_masks=False, max_im_width=-1, zip_outdir=False, dtype=None)


def test_parse_args_short_forms():
    a = ae.parse_args("-b 16 -i in -o out -s -r run -f 0.3 -t 512 -n 7 -m 900 -z --half --no_time --no_conf --overwrite "
                      "--no_cloudy --keep_ratio_128 --fuse --save_masks --dtype bf16".split())
    assert (a.batch_size, a.images_paths, a.output_path, a.save_input, a.resume_path) == (16, "in", "out", True, "run")
    assert (a.flood_mask_binarization, a.target_size, a.n_images, a.max_im_width, a.zip_outdir) == (0.3, 512, 7, 900, True)
    assert a.half and a.no_time and a.no_conf and a.overwrite and a.no_cloudy and a.keep_ratio_128 and a.fuse and a.save_masks
    assert a.dtype == "bf16"
    with pytest.raises(SystemExit):
        ae.parse_args([])                                  # -i is required
    with pytest.raises(SystemExit):
        ae.parse_args(["-i", "in", "--dtype", "fp32"])
    with pytest.raises(SystemExit):
        ae.parse_args(["-i", "in", "-z"])                  # nothing to zip without an output directory


def test_upload_is_refused():
    with pytest.raises(SystemExit, match="--upload is not supported"):
        ae.parse_args(["-i", "in", "--upload"])


@pytest.mark.parametrize("args,name", [
    ((False, False, -1, 640, 0.5, True), "S-640"),
    ((True, False, -1, 640, 0.5, True), "half-S-640"),
    ((False, True, -1, 640, 0.5, True), "AR--1"),
    ((False, True, 1024, 640, 0.5, True), "AR-1024"),
    ((True, True, 0, 640, 0.4, False), "half-AR-bin0.4-no_cloudy"),
    ((False, False, 512, 256, -1.0, False), "S-256-bin-1.0-no_cloudy"),
])
def test_get_outdir_name(args, name):
    assert ae.get_outdir_name(*args) == name


def test_make_outdir(tmp_path):
    out = ae.make_outdir(tmp_path / "_auto_", False, True, False, -1, 640, 0.5, False)
    assert out == tmp_path / "half-S-640-no_cloudy" and out.is_dir()
    with pytest.raises(SystemExit, match="already exists"):
        ae.make_outdir(tmp_path / "_auto_", False, True, False, -1, 640, 0.5, False)
    assert ae.make_outdir(out, True, False, False, -1, 640, 0.5, True) == out
    deep = ae.make_outdir(tmp_path / "a" / "b", False, False, False, -1, 640, 0.5, True)
    assert deep.is_dir()


def test_select_paths():
    p = ["a", "b", "c"]
    assert ae.select_paths(p, -1) == p
    assert ae.select_paths(p, 0) == p
    assert ae.select_paths(p, 2) == ["a", "b"]
    assert ae.select_paths(p, 3) == p
    assert ae.select_paths(p, 7) == ["a", "b", "c", "a", "b", "c", "a"]
    assert ae.select_paths(p, 6) == ["a", "b", "c", "a", "b", "c"]


def test_size_validation(capsys):
    assert ae.validate_sizes(4, 640, False, -1) == (4, 640, -1)
    assert ae.validate_sizes(4, 700, False, -1) == (4, 640, -1)
    assert ae.validate_sizes(4, 255, False, 300) == (4, 128, 300)        # max_im_width matters with keep_ratio only
    assert ae.validate_sizes(8, 640, True, -1) == (1, 640, -1)
    assert ae.validate_sizes(8, 700, True, 1000) == (1, 700, 896)        # target_size is ignored, not rounded
    assert ae.validate_sizes(1, 640, True, 1024) == (1, 640, 1024)
    assert "overwritten to 896" in capsys.readouterr().out


def test_event_file_name():
    assert ae.event_file_name("photo", "flood", 640, False, False) == "photo_flood_640.png"
    assert ae.event_file_name("photo", "smog", 512, True, False) == "photo_smog_512_AR.png"
    assert ae.event_file_name("photo", "mask", 640, False, True) == "photo_mask_640_no_cloudy.png"
    assert ae.event_file_name("a.b", "input", 256, True, True) == "a.b_input_256_AR_no_cloudy.png"


def test_time_stores():
    s = ae.get_time_stores(1.5)
    assert list(s) == ["imports", "setup", "data pre-processing", "encode", "mask", "flood", "depth", "segmentation", "smog",
                       "wildfire", "all events", "numpy", "inference on all images", "write"]
    assert s["imports"] == [1.5] and all(v == [] for k, v in s.items() if k != "imports")


def test_rgba_over_white():
    """uint8(((1 - a) + a * rgb) * 255) on [0, 1] values, truncated."""
    im = np.array([[[255, 0, 0, 255], [255, 0, 0, 0]],
                   [[10, 100, 200, 128], [11, 22, 33, 51]]], dtype=np.uint8)
    # a = 128 / 255: 127 + 128 * (10, 100, 200) / 255 = 132.02, 177.20, 227.39;  a = 51 / 255 = 0.2: 204 + 0.2 * (11, 22, 33)
    want = np.array([[[255, 0, 0], [255, 255, 255]],
                     [[132, 177, 227], [206, 208, 210]]], dtype=np.uint8)
    got = ae.rgba_to_rgb(im)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


def test_read_image(tmp_path):
    from PIL import Image

    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    assert np.array_equal(ae.read_image(tmp_path / "rgb.png"), rgb)
    rgba = np.dstack([rgb, np.full((2, 3), 255, dtype=np.uint8)])
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    assert np.array_equal(ae.read_image(tmp_path / "rgba.png"), rgb)
    Image.fromarray(rgb[..., 0]).save(tmp_path / "grey.png")
    with pytest.raises(ValueError, match="not an 8-bit RGB"):
        ae.read_image(tmp_path / "grey.png")
