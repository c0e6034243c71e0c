"""The device PNG decoder (csrc/png_decode.hip) against the model of ``tests/png_decode_model.py``: the pixels of
``cgan_png_decode`` equal the model's (which equal PIL's, test_png_decode_host.py) exactly on the whole corpus -- PIL's and the
model's files, the hand-built streams, H, W in {1, 2, 7, 64, 65, 129}^2, the long shapes and the 600 x 900 noise file -- in one
batch and file by file; the round trip with the project's encoder, broken files against the host twin, refusals and the count
of calls."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as jm
import png_decode_corpus as pc
import png_decode_model as pm
from climategan_amd import _lib, ops, png

pytestmark = pytest.mark.gpu
CORPUS = pc.corpus()


def device_decode(datas):
    """The files in ONE call -> (per file: the pixels as numpy, shaped and typed as the model's; the status words)."""
    descs = []
    for data in datas:
        d, why = png.probe(data)
        assert d is not None, why
        descs.append(d)
    blob, descs, descs_dev = png.upload(list(zip(descs, datas)), "cuda")
    out, status = ops.png_decode(blob, descs, descs_dev)
    out, results = out.cpu().numpy(), []
    for d in descs:
        px = out[d.out_offset:d.out_offset + d.width * d.height * d.channels * (d.bit_depth // 8)]
        results.append(px.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else px.reshape(d.height, d.width, d.channels))
    return results, status.cpu().tolist()


@pytest.fixture(scope="module")
def together():
    return device_decode([data for _, data in CORPUS])


def test_corpus_in_one_batch(together):
    pixels, status = together
    assert status == [0] * len(CORPUS)
    for (name, data), got in zip(CORPUS, pixels):
        want = pc.model(data)["pixels"]
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    assert any(p.dtype == np.uint16 for p in pixels)                      # the 16-bit path


def test_file_by_file(together):
    """Batch independence: every file alone gives what it gave among the others."""
    for (name, data), want in zip(CORPUS, together[0]):
        alone, status = device_decode([data])
        assert status == [0] and np.array_equal(alone[0], want), name


def test_decode_returns_typed_views():
    files = [data for name, data in CORPUS if name.startswith("model-filters-cycling")]
    images = png.decode(files)
    assert [tuple(im.shape)[2] for im in images] == [3, 1, 4, 1]
    assert [im.dtype for im in images] == [torch.uint8] * 3 + [torch.uint16]
    assert all(im.data_ptr() % 16 == 0 and im.is_cuda for im in images)
    for data, im in zip(files, images):
        want = pc.model(data)["pixels"]
        assert np.array_equal(im.cpu().numpy().view(want.dtype), want)


@pytest.mark.parametrize("level", (1, 2))
def test_round_trip_with_the_encoder(level):
    for c in (3, 1):
        imgs = np.stack([jm.make_image(kind, 72, 100, c) for kind in jm.CONTENTS])
        files = png.encode(torch.from_numpy(imgs).cuda(), level=level)
        for i, im in enumerate(png.decode(files)):
            assert np.array_equal(im.cpu().numpy(), imgs[i]), (level, c, jm.CONTENTS[i])


def test_cut_and_changed_files():
    """The files the sanitizer program has passed on the CPU: the device's status is the host twin's, and the intact files of
    the same batch stay exact."""
    intact = list(CORPUS[::30])
    broken = list(pc.broken_files())
    grey = np.zeros((4, 7, 1), dtype=np.uint8)
    broken += [(name, pm.frame(grey, stream)) for name, stream in pc.corrupt_streams()[0]]
    assert len(broken) == 25 + 23
    files = intact[:2] + broken + intact[2:]
    pixels, status = device_decode([data for _, data in files])
    for (name, data), got, s in zip(files, pixels, status):
        d = pc.parse_host(data)[0]
        _, want, host_status, _ = pc.decode_host(pc.stream_host(data, d), d)
        assert s == host_status, name
        if (name, data) in intact:
            assert s == 0 and np.array_equal(got, pc.model(data)["pixels"]), name
        else:
            assert s == pc.CORRUPT, name


def logged(fn):
    """The C-ABI calls ``fn`` makes, by name, and the exception it ends with (or None)."""
    _lib.CALL_LOG = []
    try:
        try:
            fn()
            err = None
        except RuntimeError as e:
            err = e
        return [what for what, _ in _lib.CALL_LOG], err
    finally:
        _lib.CALL_LOG = None


def test_call_counts_and_refusals():
    good = CORPUS[0][1]
    # per file one parse and one copy of its stream; per batch ONE device call (a memset and three launches)
    calls, err = logged(lambda: png.decode([good, CORPUS[1][1]]))
    assert err is None and sorted(calls) == ["cgan_png_decode"] + ["cgan_png_parse_host"] * 2 + ["cgan_png_stream_host"] * 2
    # a file the parser refuses is named, and alone it leads to no device call at all
    for name, data in pc.unsupported_files():
        calls, err = logged(lambda: png.decode([data]))
        assert calls == ["cgan_png_parse_host"] and "file 0" in str(err), name
        calls, err = logged(lambda: png.decode([good, data]))
        assert "file 1" in str(err), name
    # descriptors and ranges the call refuses: the size query or the call's own checks say so, before any launch
    d, _ = png.probe(good)
    blob, descs, descs_dev = png.upload([(d, good)], "cuda")
    calls, err = logged(lambda: ops.png_decode(blob[:-40], descs, descs_dev))
    assert calls == ["cgan_png_decode"] and "blob's end" in str(err)
    descs[0].blob_offset = 2
    calls, err = logged(lambda: ops.png_decode(blob, descs, descs_dev))
    assert calls == ["cgan_png_decode_workspace_bytes"] and "aligned" in str(err)
    descs[0].blob_offset = 0
    for field, value in (("channels", 2), ("width", 8193), ("bit_depth", 16), ("stream_bytes", 0)):
        bad = (_lib.PngDesc * 1)(type(d).from_buffer_copy(descs[0]))
        setattr(bad[0], field, value)
        calls, err = logged(lambda: ops.png_decode(blob, bad, descs_dev))
        assert calls == ["cgan_png_decode_workspace_bytes"] and "descriptor 0" in str(err), field
    with pytest.raises(RuntimeError):
        png.decode([good], device="cpu")
    with pytest.raises(RuntimeError):
        ops.png_decode(torch.zeros(64, dtype=torch.uint8), descs, descs_dev)      # a CPU tensor
    out, status = ops.png_decode(blob, descs, descs_dev)                          # and the good descriptor still decodes
    assert status.tolist() == [0]


def test_fallback_for_an_interlaced_file():
    good, laced = CORPUS[0][1], pc.interlaced_file()
    images = png.decode([good, laced], fallback=True)
    assert np.array_equal(images[0].cpu().numpy(), pc.model(good)["pixels"])
    assert images[1].is_cuda and np.array_equal(images[1].cpu().numpy(), np.asarray(Image.open(io.BytesIO(laced))))
