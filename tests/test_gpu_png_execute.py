"""The execute step the three inflate kernels share (csrc/png_decode.hip's ``execute_tokens``) on the hand-built files of
``tests/png_execute_cases.py``: the framed files through ``ops.png_decode_rows`` (the row window), the ordinary ones through
``ops.png_decode`` as the serial kernel, at subsequences of 32 bits / 4 tokens and at the compiled defaults (the ring) --
pixels equal to the Python model's byte for byte, status 0 everywhere; a candidate with a match that reaches in front of its
row is refused by the row path and decoded by the fallback, as the host twin says.  What the files' names claim is asserted
from the model and the twin without a GPU."""
import numpy as np
import pytest

import png_decode_corpus as pc
import png_execute_cases as ec
import png_rows_cases as rc
from climategan_amd import ops, png

FORMS = (("serial", {"subseq_bits": 0}), ("32-4", {"subseq_bits": 32, "lane_tokens": 4}), ("defaults", {}))


def test_the_cases_are_what_they_claim():
    """No GPU: the twin takes every framed file by rows and the reaching one by the fallback; the rows hold the tokens."""
    for name, framed, ordinary in ec.intact():
        want = rc.model(framed)["pixels"]
        px, status, path, d, _ = rc.decode_rows_host(framed)
        assert (status, path, d.rows) == (pc.OK, rc.ROWS, ec.H) and np.array_equal(px, want), name
        assert png.probe(ordinary)[0].rows == 0 and np.array_equal(rc.model(ordinary)["pixels"], want), name
    rows = [[(t, at) for t, at in row if t[0] == "lit" or t[1]]                                  # an empty stored block is no token
            for row in rc.tokens_by_row(rc.model(ec.intact()[0][1]))]
    assert len(rows[0]) == 128 and [tuple(t) for t, _ in rows[0][126:]] == [("match", 258, 1), ("match", 217, 300)]
    assert rows[1][63][0][0] == "match" and rows[1][63][0][2] < rows[1][63][0][1]               # token 64 of the round, a repeat
    assert rows[1][64 + 62][0][0] == "match" and rows[1][64 + 62][0][2] <= 62                   # token 63 reads its round's literals
    assert all(t[0] == "match" for t, _ in rows[2][3:]) and len(rows[2]) - 3 > 64
    name, data = ec.reaching_back()
    px, status, path, _, _ = rc.decode_rows_host(data)
    assert (status, path) == (pc.OK, rc.REFUSED) and np.array_equal(px, rc.model(data)["pixels"]), name


def pixels_of(out, d):
    return out[d.out_offset:d.out_offset + d.width * d.height].reshape(d.height, d.width, 1)


@pytest.mark.gpu
def test_framed_files_by_rows():
    files = [(name, framed) for name, framed, _ in ec.intact()] + [ec.reaching_back()]
    datas = [data for _, data in files]
    probed = [png.probe(data)[0] for data in datas]
    blob, descs, descs_dev = png.upload(list(zip(probed, datas)), "cuda")
    tables, tables_dev = png.row_tables(descs, datas, "cuda")
    out, status, path = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
    out = out.cpu().numpy()
    assert status.cpu().tolist() == [pc.OK] * len(files)
    assert path.cpu().tolist() == [rc.ROWS] * len(ec.intact()) + [rc.REFUSED]
    for (name, data), d in zip(files, descs):
        assert np.array_equal(pixels_of(out, d), rc.model(data)["pixels"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("form", [name for name, _ in FORMS])
def test_ordinary_files_whole_stream(form):
    files = [(name, ordinary) for name, _, ordinary in ec.intact()]
    datas = [data for _, data in files]
    probed = [png.probe(data)[0] for data in datas]
    blob, descs, descs_dev = png.upload(list(zip(probed, datas)), "cuda")
    out, status = ops.png_decode(blob, descs, descs_dev, **dict(FORMS)[form])
    out = out.cpu().numpy()
    assert status.cpu().tolist() == [pc.OK] * len(files)
    for (name, data), d in zip(files, descs):
        assert np.array_equal(pixels_of(out, d), rc.model(data)["pixels"]), (form, name)
