"""The host side of ``data.loaders.decode``, no GPU: which files a reader thread leaves to the device decoders
(``data.read_file`` / ``data.device_takes``), on the dataset tests/loader_fixture.py writes and on files written here, and how
``get_loader`` and ``OmniLoader`` read the option."""
import numpy as np
import pytest
import torch
from PIL import Image

import loader_fixture as lf
from climategan_amd import data, png


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    root = tmp_path_factory.mktemp("loaders_decode")
    return root, lf.write(root)


def dataset(root, mode, domain, tasks=("d", "s", "m")):
    return data.OmniListDataset(mode, domain, lf.fixture_opts(root, tasks), device="cpu")


# task, domain -> (channels, bit depth) of the fixture's .png files: what DESIGN 4.23's table takes on the device
EXPECTED = {("x", None): {(3, 8), (4, 8)}, ("m", None): {(1, 8)}, ("s", "r"): {(4, 8)}, ("s", "s"): {(4, 8)},
            ("s", "kitti"): {(3, 8)}, ("d", "s"): {(3, 8), (4, 8)}, ("d", "kitti"): {(1, 16)}}


def test_every_png_of_the_fixture_is_taken_on_the_device(fixture):
    """The condition that lets the GPU test demand zero fall-backs: PIL's default writer makes files the device decoder takes,
    with the channels and the bit depth the task's raw kind accepts."""
    root, listed = fixture
    seen, pngs = set(), 0
    for mode in ("train", "val"):
        for domain in lf.DOMAINS:
            ds = dataset(root, mode, domain, tasks=("d", "s", "m") if domain != "rf" else ("p",))
            for i in range(len(ds)):
                records = ds.read_file(i)
                assert list(records) == list(ds.samples_paths[i])
                for task, rec in records.items():
                    path = data.env_to_path(ds.samples_paths[i][task])
                    if not str(path).endswith(".png"):
                        assert not isinstance(rec, data.FileRecord)
                        continue
                    pngs += 1
                    assert isinstance(rec, data.FileRecord) and rec.codec == "png", (mode, domain, task, path)
                    d = rec.desc
                    assert (d.channels, d.bit_depth) in EXPECTED[(task, None if task in "xm" else domain)], (domain, task)
                    assert len(rec.stream) == d.stream_bytes and rec.table is None and d.rows == 0     # PIL frames no rows
                    assert str(rec.path) == str(path)
                    seen.add((task, domain, d.channels, d.bit_depth))
    assert pngs > 50 and {(t, c, b) for t, _, c, b in seen} >= {("x", 3, 8), ("x", 4, 8), ("m", 1, 8), ("s", 4, 8), ("s", 3, 8),
                                                                ("d", 3, 8), ("d", 1, 16)}


def test_the_table_of_files_taken():
    takes = data.device_takes
    assert takes("x", "r", 3, 8) and takes("x", "kitti", 4, 8) and not takes("x", "r", 1, 8) and not takes("x", "r", 1, 16)
    assert all(takes("m", "rf", c, 8) for c in (1, 3, 4)) and not takes("m", "rf", 1, 16)
    assert takes("s", "r", 4, 8) and takes("s", "s", 4, 8) and not takes("s", "s", 3, 8)
    assert takes("s", "kitti", 3, 8) and not takes("s", "kitti", 4, 8)
    assert takes("d", "s", 3, 8) and takes("d", "s", 4, 8) and not takes("d", "s", 1, 16)
    assert takes("d", "kitti", 1, 16) and not takes("d", "kitti", 1, 8) and not takes("d", "kitti", 3, 8)
    assert not any(takes("d", "r", c, b) for c in (1, 3, 4) for b in (8, 16))       # the host converts the real depth to fp32
    assert not takes("p", "rf", 3, 8)


def test_host_records_for_what_the_device_does_not_take(fixture, tmp_path):
    root, listed = fixture
    npy = next(s["d"] for s in listed["train"]["r"] if s["d"].endswith(".npy"))
    rec = data.read_file(npy, "d", "r")
    want = data.read_host(npy, "d", "r")
    assert not isinstance(rec, data.FileRecord) and np.array_equal(rec[0], want[0]) and rec[1] == want[1]
    pt = tmp_path / "s0.pt"
    torch.save(torch.zeros(1, 1, 4, 4), pt)
    rec = data.read_file(pt, "s", "r")
    assert torch.is_tensor(rec[0]) and rec[1] == {}
    rgb = (np.arange(24 * 40 * 3) % 251).astype(np.uint8).reshape(24, 40, 3)
    palette = tmp_path / "x_palette.png"
    Image.fromarray(rgb).convert("P").save(palette)
    assert png.probe(palette.read_bytes())[0] is None
    rec = data.read_file(palette, "x", "r")
    want = data.read_host(palette, "x", "r")
    assert not isinstance(rec, data.FileRecord) and np.array_equal(rec[0], want[0]) and rec[1] == want[1]
    grey = tmp_path / "x_grey.png"                                                  # a kind the decoder takes and the task refuses
    Image.fromarray(rgb[..., 0]).save(grey)
    assert png.probe(grey.read_bytes())[0] is not None and not isinstance(data.read_file(grey, "x", "r"), data.FileRecord)
    framed = tmp_path / "m_rgb.png"
    Image.fromarray(rgb).save(framed)
    assert isinstance(data.read_file(framed, "m", "rf"), data.FileRecord)
    with pytest.raises(ValueError, match="Unknown data type"):                      # the same error from the same place
        data.read_file(tmp_path / "x.xyz", "x", "r")


def test_the_option(fixture, monkeypatch):
    root, _ = fixture
    monkeypatch.setattr(data, "_device", lambda device=None: torch.device("cpu"))
    opts = lf.fixture_opts(root)
    assert "decode" not in opts.data.loaders
    ld = data.get_loader("train", "r", opts, device="cpu")
    assert ld.decode == "host" and sorted(ld.times) == ["batches", "read", "stage", "transform"]
    assert ld.decode_counts == {"png": 0, "jpeg": 0, "host": 0}
    opts.data.loaders["decode"] = "host"
    assert data.get_loader("train", "r", opts, device="cpu").decode == "host"
    opts.data.loaders["decode"] = "gpu"
    with pytest.raises(ValueError, match="decode"):
        data.get_loader("train", "r", opts, device="cpu")
    with pytest.raises(ValueError, match="decode"):
        data.OmniLoader(ld.dataset, 2, device="cpu", transform=lambda s: s, decode="gpu")
    opts.data.loaders["decode"] = "device"
    with pytest.raises(ValueError, match="cuda"):                                   # no decoder on any other device
        data.get_loader("train", "r", opts, device="cpu")
