"""The device PNG decoder's row path (csrc/png_decode.hip) against the model of ``tests/png_decode_model.py`` and the
host twin: the pixels of ``cgan_png_decode_rows`` equal the model's on the row-framed files of ``tests/png_rows_cases.py``, on
the candidates the row path refuses and on ordinary files, in one mixed batch and file by file; ``path`` is the twin's; the
project's encoder round-trips by rows at both levels; broken candidates get the twin's status; the count of calls."""
import numpy as np
import pytest
import torch

import jpeg_model as jm
import png_decode_corpus as pc
import png_rows_cases as rc
from climategan_amd import _lib, ops, png

pytestmark = pytest.mark.gpu
CORPUS = pc.corpus()
PLAIN = [(name, data) for name, data in CORPUS[::12] if png.probe(data)[0].rows == 0]
PLAIN += [next((name, data) for name, data in CORPUS if name.startswith("pil-") and "I;16" in name)]        # the uint16 path
MIXED = list(rc.framed_files()[:20]) + PLAIN[:4] + list(rc.refused_files()) + list(rc.framed_files()[20:]) + PLAIN[4:]


def device_decode(datas):
    """The files in ONE ``cgan_png_decode_rows`` -> (per file the pixels as numpy, shaped and typed as the model's; the status
    words; the paths)."""
    descs = []
    for data in datas:
        d, why = png.probe(data)
        assert d is not None, why
        descs.append(d)
    blob, descs, descs_dev = png.upload(list(zip(descs, datas)), "cuda")
    tables, tables_dev = png.row_tables(descs, datas, "cuda")
    out, status, path = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
    out, results = out.cpu().numpy(), []
    for d in descs:
        px = out[d.out_offset:d.out_offset + d.width * d.height * d.channels * (d.bit_depth // 8)]
        results.append(px.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else px.reshape(d.height, d.width, d.channels))
    return results, status.cpu().tolist(), path.cpu().tolist()


@pytest.fixture(scope="module")
def together():
    return device_decode([data for _, data in MIXED])


def test_mixed_batch(together):
    pixels, status, path = together
    assert status == [0] * len(MIXED)
    for (name, data), got, p in zip(MIXED, pixels, path):
        want = rc.model(data)["pixels"]
        assert got.dtype == want.dtype and np.array_equal(got, want), name
        assert p == rc.decode_rows_host(data)[2], name                             # the path is the twin's
    assert any(p.dtype == np.uint16 for p in pixels)
    names = [name for name, _ in MIXED]
    framed, refused, plain = (set(n for n, _ in part) for part in (rc.framed_files(), rc.refused_files(), PLAIN))
    assert all(p == (rc.ROWS if n in framed else rc.REFUSED if n in refused else rc.SERIAL) for n, p in zip(names, path))
    assert plain and {rc.SERIAL, rc.ROWS, rc.REFUSED} == set(path)


def test_file_by_file(together):
    """Batch independence: every file alone gives what it gave among the others."""
    for (name, data), want, p in zip(MIXED, together[0], together[2]):
        alone, status, path = device_decode([data])
        assert status == [0] and path == [p] and np.array_equal(alone[0], want), name


@pytest.mark.parametrize("level", (1, 2))
def test_encoder_files_go_by_rows(level):
    for c, h, w in ((3, 72, 100), (1, 72, 100), (3, 3, 4096), (1, 65, 7)):
        imgs = np.stack([jm.make_image(kind, h, w, c) for kind in jm.CONTENTS])
        files = png.encode(torch.from_numpy(imgs).cuda(), level=level)
        assert all(png.probe(f)[0].rows == h for f in files)
        pixels, status, path = device_decode(files)
        assert status == [0] * len(files) and path == [rc.ROWS] * len(files), (level, c, h, w)
        for i, (f, got) in enumerate(zip(files, pixels)):
            assert np.array_equal(got, imgs[i]), (level, c, h, w, jm.CONTENTS[i])
            assert rc.decode_rows_host(f)[2] == rc.ROWS
        for i, im in enumerate(png.decode(files)):                                 # and through the public call
            assert np.array_equal(im.cpu().numpy(), imgs[i])


def test_broken_candidates():
    """The device's status is the twin's, and the intact files of the same batch stay exact."""
    intact = [rc.framed_files()[5], ("base", rc.broken_base()), PLAIN[0]]
    files = intact[:2] + list(rc.broken_files()) + intact[2:]
    pixels, status, path = device_decode([data for _, data in files])
    for (name, data), got, s, p in zip(files, pixels, status, path):
        _, host_status, host_path, _, _ = rc.decode_rows_host(data)
        assert (s, p) == (host_status, host_path), name
        if (name, data) in intact:
            assert s == 0 and np.array_equal(got, rc.model(data)["pixels"]), name
        else:
            assert s == pc.CORRUPT, name
    images, reasons = png.try_decode([data for _, data in files])
    assert sorted(reasons) == [2, 3, 4] and all(images[i] is not None for i in (0, 1, 5))


def logged(fn):
    """The C-ABI calls ``fn`` makes, by name."""
    _lib.CALL_LOG = []
    try:
        fn()
        return sorted(what for what, _ in _lib.CALL_LOG)
    finally:
        _lib.CALL_LOG = None


def test_call_counts():
    framed, plain = rc.framed_files()[-1][1], CORPUS[0][1]
    # a batch with a candidate: the table of that file, ONE cgan_png_decode_rows and no cgan_png_decode
    calls = logged(lambda: png.decode([plain, framed, CORPUS[1][1]]))
    assert calls == (["cgan_png_decode_rows"] + ["cgan_png_parse_host"] * 3 + ["cgan_png_row_table_host"] + ["cgan_png_stream_host"] * 3)
    # a batch without one: the calls of before
    calls = logged(lambda: png.decode([plain, CORPUS[1][1]]))
    assert calls == ["cgan_png_decode"] + ["cgan_png_parse_host"] * 2 + ["cgan_png_stream_host"] * 2


def test_refusals_before_any_launch():
    framed = rc.framed_files()[-1][1]
    d, _ = png.probe(framed)
    blob, descs, descs_dev = png.upload([(d, framed)], "cuda")
    tables, tables_dev = png.row_tables(descs, [framed], "cuda")
    tables[3] = tables[2]
    with pytest.raises(RuntimeError, match="file 0"):
        ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
    with pytest.raises(RuntimeError):
        ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev[:-1])
    with pytest.raises(RuntimeError):
        ops.png_decode_rows(blob, descs, descs_dev, None, None)
    tables, tables_dev = png.row_tables(descs, [framed], "cuda")
    out, status, path = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)      # and the good table still decodes
    assert status.tolist() == [0] and path.tolist() == [rc.ROWS]
