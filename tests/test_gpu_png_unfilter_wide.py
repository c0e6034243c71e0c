"""The multi-wave unfilter kernel (csrc/png_decode.hip) on the shape list of ``png_unfilter_wide_cases`` at the
waves and the lag the library was compiled with: heights around one wave's and one pass's rows, widths around a chunk of the
prefetch and the distance between two waves, the four pixel kinds, all five filters, row-framed and ordinary files -- through
``png.decode`` in one mixed batch and file by file, and through both device calls.  The pixels are the source arrays', exactly;
broken files get the host twin's status with the intact files of the batch exact."""
import numpy as np
import pytest
import torch

import png_decode_corpus as pc
import png_unfilter_wide_cases as wc
from climategan_amd import ops, png

pytestmark = pytest.mark.gpu
NW, LAG, _ = wc.compiled()
CASES = wc.files(NW, LAG)


def as_numpy(image, like):
    return image.cpu().numpy().view(like.dtype).reshape(like.shape)


@pytest.fixture(scope="module")
def together():
    return png.decode([data for _, _, data in CASES])


def test_mixed_batch_is_exact(together):
    assert any(png.probe(data)[0].rows for _, _, data in CASES) and not all(png.probe(data)[0].rows for _, _, data in CASES)
    assert {img.dtype.itemsize for _, img, _ in CASES} == {1, 2}
    for (name, img, _), got in zip(CASES, together):
        assert tuple(got.shape) == img.shape and np.array_equal(as_numpy(got, img), img), name


def test_file_by_file(together):
    """Batch independence: every file alone gives what it gave among the others."""
    for (name, img, data), want in zip(CASES, together):
        alone = png.decode([data])[0]
        assert torch.equal(alone, want), name


def test_ordinary_files_through_the_call_without_rows():
    plain = [(name, img, data) for name, img, data in CASES if png.probe(data)[0].rows == 0]
    taken = [png.probe(data)[0] for _, _, data in plain]
    blob, descs, descs_dev = png.upload(list(zip(taken, [data for _, _, data in plain])), "cuda")
    out, status = ops.png_decode(blob, descs, descs_dev)
    assert status.tolist() == [0] * len(plain)
    out = out.cpu().numpy()
    for (name, img, _), d in zip(plain, descs):
        assert np.array_equal(out[d.out_offset:d.out_offset + img.nbytes].view(img.dtype).reshape(img.shape), img), name


def test_framed_and_ordinary_files_in_one_rows_call():
    picked = [c for c in CASES if c[1].shape[0] >= 64 * NW][:12] + list(wc.extremes())
    datas = [data for _, _, data in picked]
    taken = [png.probe(data)[0] for data in datas]
    assert any(d.rows for d in taken) and any(d.rows == 0 for d in taken)
    blob, descs, descs_dev = png.upload(list(zip(taken, datas)), "cuda")
    tables, tables_dev = png.row_tables(descs, datas, "cuda")
    out, status, path = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
    assert status.tolist() == [0] * len(picked) and path.tolist() == [1 if d.rows else 0 for d in descs]
    out = out.cpu().numpy()
    for (name, img, _), d in zip(picked, descs):
        assert np.array_equal(out[d.out_offset:d.out_offset + img.nbytes].view(img.dtype).reshape(img.shape), img), name


def test_idle_waves_and_many_passes_in_one_launch():
    """A 1 x 1 file (one lane of one wave has a pixel) beside the 8192 x 3 file (the most passes a file can take)."""
    cases = [wc.tiny(), wc.extremes()[0], wc.tiny()]
    for (name, img, _), got in zip(cases, png.decode([data for _, _, data in cases])):
        assert np.array_equal(as_numpy(got, img), img), name


def test_broken_files_get_the_twins_status():
    broken = wc.broken(NW, LAG)
    intact = [c for c in CASES if c[1].shape[0] > 64][:3]
    datas = [intact[0][2], broken[0][1], intact[1][2], broken[1][1], broken[2][1], intact[2][2]]
    images, reasons = png.try_decode(datas)
    assert sorted(reasons) == [1, 3, 4]
    for name, data in broken:
        assert wc.wide_host(data, NW, LAG)[1:3] == (pc.CORRUPT, 0), name
    for i, (name, img, _) in zip((0, 2, 5), intact):
        assert np.array_equal(as_numpy(images[i], img), img), name
