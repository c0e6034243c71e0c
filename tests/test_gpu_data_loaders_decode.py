"""``data.loaders.decode: device`` on the dataset tests/loader_fixture.py writes: the reader threads leave the
PNG and JPEG files to the device decoders, one blob and one decoder call per codec and batch.

Bounds.  Every stage between the file and the gather is integer (the decoders' pixels are PIL's, exactly: test_gpu_png_decode.py,
test_gpu_jpeg_decode.py against their own references), and the min / max the device finds are the values the host finds, so a
batch of a device-mode loader is ``torch.equal`` to the host-mode loader's under the same seed and draws; the losses of a train
step equal bit for bit."""
import io
import random
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import loader_fixture as lf
import png_decode_model as pm
from test_gpu_train_loop import build_masker_trainer, close, loop_opts, seed_all

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MASKER, PAINTER = ("d", "s", "m"), ("p",)
CASES = [(mode, domain, PAINTER if domain == "rf" else MASKER) for mode in ("train", "val") for domain in lf.DOMAINS]


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    root = tmp_path_factory.mktemp("loaders_decode")
    return root, lf.write(root)


def seed_draws(n):
    np.random.seed(n)
    random.seed(n)


def make_loader(root, mode, domain, tasks, prefetch, decode, seed=4, remap=None):
    from climategan_amd.data import get_loader
    opts = lf.fixture_opts(root, tasks)
    if decode is not None:
        opts.data.loaders["decode"] = decode
    ld = get_loader(mode, domain, opts, prefetch=prefetch, device=DEV).seed(seed)
    if remap is not None:
        ld.dataset.samples_paths = [{task: remap(task, path) for task, path in s.items()} for s in ld.dataset.samples_paths]
    return ld


def epochs_of(ld, n_epochs=2, draws=9):
    seed_draws(draws)
    out = [[{"data": {k: v.clone() for k, v in b["data"].items()}, "paths": b["paths"]} for b in ld] for _ in range(n_epochs)]
    torch.cuda.synchronize()
    ld.close()
    return out


def assert_equal_epochs(got, want, what=""):
    assert len(got) == len(want)
    for e, (ga, wa) in enumerate(zip(got, want)):
        assert len(ga) == len(wa) == 2
        for a, b in zip(ga, wa):
            assert set(a["data"]) == set(b["data"])
            for task in a["data"]:
                assert a["data"][task].dtype == b["data"][task].dtype
                assert torch.equal(a["data"][task], b["data"][task]), (what, e, task)


def files_read(epochs, suffixes):
    return sum(str(p).lower().endswith(suffixes) for ep in epochs for b in ep for paths in b["paths"].values() for p in paths)


@pytest.fixture(scope="module")
def host_epochs(fixture):
    """The host-mode loader's two epochs per case, computed once (prefetch=0; test_gpu_data_loaders.py holds prefetch=1 to it)."""
    root, _ = fixture
    return {(mode, domain): epochs_of(make_loader(root, mode, domain, tasks, 0, None)) for mode, domain, tasks in CASES}


@pytest.mark.parametrize("prefetch", (0, 1))
@pytest.mark.parametrize("mode,domain,tasks", CASES)
def test_device_mode_equals_host_mode(fixture, host_epochs, mode, domain, tasks, prefetch):
    root, _ = fixture
    ld = make_loader(root, mode, domain, tasks, prefetch, "device")
    got = epochs_of(ld)
    want = host_epochs[(mode, domain)]
    assert [b["paths"] for ep in got for b in ep] == [b["paths"] for ep in want for b in ep]
    assert_equal_epochs(got, want, (mode, domain, prefetch))
    # every .png went to the device decoder, everything else (.npy) to the host
    pngs, others = files_read(got, (".png",)), files_read(got, (".npy", ".pt"))
    assert pngs > 0 and ld.decode_counts == {"png": pngs, "jpeg": 0, "host": others}
    assert (others > 0) == (domain in ("r", "s", "kitti"))
    assert sorted(ld.times) == ["batches", "decode", "read", "stage", "transform"] and ld.times["decode"] > 0


def test_host_mode_counts_nothing_and_times_as_before(fixture):
    root, _ = fixture
    ld = make_loader(root, "val", "rf", PAINTER, 0, "host")
    epochs_of(ld, 1)
    assert ld.decode_counts == {"png": 0, "jpeg": 0, "host": 0} and sorted(ld.times) == ["batches", "read", "stage", "transform"]


@pytest.mark.parametrize("subsampling", (0, 2), ids=("444", "420"))
def test_jpeg_x_files(fixture, tmp_path, subsampling):
    """``x`` rewritten as quality-90 JPEG: the batch is ``compile_transforms`` on ``RawSource(jpeg.decode(file))`` -- the loader
    adds nothing to what ``jpeg.decode`` returns (val mode: the transforms draw nothing)."""
    from climategan_amd import data, jpeg
    from climategan_amd.transforms import RawSource
    root, _ = fixture

    def as_jpeg(task, path):
        if task != "x":
            return path
        target = tmp_path / (str(abs(hash(path))) + ".jpg")
        Image.fromarray(np.array(Image.open(data.env_to_path(path)))[..., :3]).save(target, "JPEG", quality=90, subsampling=subsampling)
        return str(target)

    ld = make_loader(root, "val", "rf", PAINTER, 1, "device", remap=as_jpeg)
    got = epochs_of(ld, 1)
    assert ld.decode_counts == {"png": 4, "jpeg": 4, "host": 0}
    for b in got[0]:
        samples = [{"x": RawSource(jpeg.decode([x])[0], "x"), "m": data.raw_source(m, "m", "rf", ld.dataset.opts, device=DEV)}
                   for x, m in zip(b["paths"]["x"], b["paths"]["m"])]
        want = ld.transform(samples)
        assert torch.equal(b["data"]["x"], want["x"]) and torch.equal(b["data"]["m"], want["m"])


def test_row_framed_files(fixture, host_epochs, tmp_path):
    """The fixture's train/s folder through ``repack_png``: the RGB and grey files come back row-framed and go through the row
    path of the one ``png_decode_rows`` call beside the RGBA files; the batches are the unrepacked ones."""
    from climategan_amd import png, repack_png
    root, _ = fixture
    src, dst = root / "train" / "s", tmp_path / "repacked"
    repack_png.main(["-i", str(src), "-o", str(dst)])
    framed = [png.probe(p.read_bytes())[0].rows != 0 for p in sorted(dst.glob("*.png"))]
    assert any(framed) and not all(framed)
    ld = make_loader(root, "train", "s", MASKER, 1, "device", remap=lambda task, path: path.replace(str(src), str(dst)))
    got = epochs_of(ld)
    assert all(str(dst) in p for b in got[0] for paths in b["paths"].values() for p in paths)
    assert_equal_epochs(got, host_epochs[("train", "s")], "repacked")
    assert ld.decode_counts["png"] == files_read(got, (".png",)) and ld.decode_counts["jpeg"] == 0


def corrupted(data):
    """One byte of the IDAT payload changed, the chunk's CRC made valid again."""
    out = pm.SIGNATURE
    for kind, payload, _ in pm.chunks(data):
        if kind == b"IDAT":
            payload = bytearray(payload)
            payload[len(payload) // 2] ^= 0x55
            payload = bytes(payload)
        out += pm.chunk(kind, payload)
    return out


def test_a_corrupt_file_falls_back_to_the_host(fixture, tmp_path):
    from climategan_amd import data
    root, listed = fixture
    bad = tmp_path / "x_corrupt.png"
    victim = listed["val"]["rf"][0]["x"]
    bad.write_bytes(corrupted(open(victim, "rb").read()))

    def remap(task, path):
        return str(bad) if path == victim else path

    host = make_loader(root, "val", "rf", PAINTER, 0, "host", remap=remap)
    seed = next(s for s in range(20) if 0 in [i for b in host.seed(s).batches() for i in b])      # an epoch that reads sample 0
    try:
        want, error = epochs_of(host.seed(seed), 1), None
    except Exception as e:                                                          # PIL refuses the file
        want, error = None, e
        host.close()
    for prefetch in (0, 1):
        ld = make_loader(root, "val", "rf", PAINTER, prefetch, "device", seed=seed, remap=remap)
        if error is not None:
            with pytest.raises(type(error)):
                epochs_of(ld, 1)
            ld.close()
            # the intact files still decode: the epoch of another seed's loader without the file
            continue
        got = epochs_of(ld, 1)
        assert_equal_epochs(got, want, "corrupt")                                   # PIL's pixels for the file, the rest exact
        assert ld.decode_counts == {"png": 7, "jpeg": 0, "host": 1}
    if error is not None:
        # what host mode raises is raised; the rest of such a batch is covered by the status test below
        rec = data.read_file(bad, "x", "rf")
        assert isinstance(rec, data.FileRecord)


def test_the_status_word_decides_file_by_file(fixture, tmp_path):
    """The staging itself, on records: a batch with one corrupt stream; the corrupt file's ``read_host`` is replaced by one
    that returns a marker array, so the test does not depend on whether PIL reads the file."""
    from climategan_amd import data
    root, listed = fixture
    ld = make_loader(root, "val", "rf", PAINTER, 0, "device")
    samples = [ld.dataset.read_file(i) for i in (0, 1)]
    good = samples[0]["x"]
    stream = bytearray(good.stream)
    stream[len(stream) // 2] ^= 0x55
    samples[0]["x"] = good._replace(stream=bytes(stream))
    marker = np.full((good.desc.height, good.desc.width, 3), 7, dtype=np.uint8)
    original, data.read_host = data.read_host, lambda path, task, domain: (marker, {"minmax": (7, 7)})
    try:
        staged = ld._stage(samples, ld._slots[0], torch.cuda.current_stream())
    finally:
        data.read_host = original
    assert ld.decode_counts == {"png": 3, "jpeg": 0, "host": 1}
    assert torch.equal(staged[0]["x"][0].cpu(), torch.from_numpy(marker)) and staged[0]["x"][1] == {"minmax": (7, 7)}
    for k, task in ((0, "m"), (1, "x"), (1, "m")):
        want = np.array(Image.open(data.env_to_path(ld.dataset.samples_paths[k][task])))
        got, known = staged[k][task]
        assert known == {} and got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (k, task)


def test_an_abandoned_epoch_leaves_the_loader_usable(fixture):
    root, _ = fixture
    seed_draws(1)
    ld = make_loader(root, "train", "r", MASKER, 1, "device")
    it = iter(ld)
    first = next(it)
    del it
    assert len(list(ld)) == 2 and first["data"]["x"].shape == (2, 3, 16, 16)
    ld.close()


def test_a_train_epoch_from_device_decoded_batches(fixture, tmp_path):
    """Two identically seeded trainers, one per decode mode: the losses of the epoch's last step are equal bit for bit."""
    from climategan_amd import ops
    root, _ = fixture
    last = {}
    for decode in ("host", "device"):
        opts = loop_opts(root, tmp_path / decode)
        opts.data.loaders["decode"] = decode
        T = build_masker_trainer(opts)
        assert all(ld.decode == decode for ld in T.loaders["train"].values())
        ops.touch(*T.G.parameters(), *T.G.buffers(), *T.D.parameters(), *T.D.buffers())
        for ld in T.loaders["train"].values():
            ld.seed(11)
        seed_all(7)
        out = T.run_epoch()
        torch.cuda.synchronize()
        last[decode] = (float(out[0]), float(out[1]), T.global_step)
        if decode == "device":
            assert all(ld.decode_counts["png"] > 0 for ld in T.loaders["train"].values())
        close(T)
    assert last["host"] == last["device"] and np.isfinite(last["host"][0])
