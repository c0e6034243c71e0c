"""The lane-parallel inflate on the device (csrc/png_decode.hip's ``inflate_lanes_kernel``) against the model: every
file of ``tests/png_lanes_cases.py``, intact and broken, in ONE ``png.decode`` batch and in one ``ops.png_decode`` batch at
subsequences of 32 bits / 4 tokens, of 64 / 8 and through the serial kernel (``subseq_bits=0``) -- pixels and status words
identical across the four and equal to the model's; a ``png_decode_rows`` batch with a refused candidate, whose whole-stream
fallback is the same kernel; which C-ABI call each form makes.  Everything is integer: the tolerance is 0."""
import numpy as np
import pytest
import torch

import png_decode_corpus as pc
import png_lanes_cases as lc
import png_rows_cases as rc
from climategan_amd import _lib, ops, png

pytestmark = pytest.mark.gpu
INTACT = list(lc.cases())
BROKEN = list(lc.broken())
FILES = INTACT[:40] + BROKEN[:24] + INTACT[40:] + BROKEN[24:]                  # the broken ones among the others
FORMS = (("defaults", {}), ("32-4", {"subseq_bits": 32, "lane_tokens": 4}), ("64-8", {"subseq_bits": 64, "lane_tokens": 8}),
         ("serial", {"subseq_bits": 0}))


def batch_decode(datas, **kw):
    """The files in ONE ``ops.png_decode`` -> (the output blob as numpy, the descriptors, the status words)."""
    probed = [png.probe(data)[0] for data in datas]
    assert all(d is not None for d in probed)
    blob, descs, descs_dev = png.upload(list(zip(probed, datas)), "cuda")
    out, status = ops.png_decode(blob, descs, descs_dev, **kw)
    return out.cpu().numpy(), descs, status.cpu().tolist()


def pixels_of(out, d):
    px = out[d.out_offset:d.out_offset + d.width * d.height * d.channels * (d.bit_depth // 8)]
    return px.view(np.uint16).reshape(d.height, d.width, 1) if d.bit_depth == 16 else px.reshape(d.height, d.width, d.channels)


@pytest.fixture(scope="module")
def decoded():
    return {form: batch_decode([data for _, data in FILES], **kw) for form, kw in FORMS}


def test_every_form_equals_the_model(decoded):
    broken = {name for name, _ in BROKEN}
    for form, (out, descs, status) in decoded.items():
        for (name, data), d, s in zip(FILES, descs, status):
            if name in broken:
                assert s == pc.CORRUPT, (form, name)                              # never OK on a broken file
            else:
                want = pc.model(data)["pixels"]
                got = pixels_of(out, d)
                assert s == pc.OK and got.dtype == want.dtype and np.array_equal(got, want), (form, name)


def test_forms_agree_word_for_word(decoded):
    _, descs, status = decoded["defaults"]
    for form, (out, _, other) in decoded.items():
        assert other == status, form
        for (name, _), d, s in zip(FILES, descs, status):
            if s == pc.OK:
                assert np.array_equal(pixels_of(out, d), pixels_of(decoded["defaults"][0], d)), (form, name)
    assert status.count(pc.CORRUPT) == len(BROKEN) and status.count(pc.OK) == len(INTACT)


def test_public_decode_in_one_batch():
    """``png.decode`` (the compiled defaults) on all intact files at once, and ``try_decode`` with the broken ones between them."""
    images = png.decode([data for _, data in INTACT])
    for (name, data), im in zip(INTACT, images):
        want = pc.model(data)["pixels"]
        assert np.array_equal(im.cpu().numpy(), want), name
    images, reasons = png.try_decode([data for _, data in FILES])
    broken = {name for name, _ in BROKEN}
    assert sorted(reasons) == [i for i, (name, _) in enumerate(FILES) if name in broken]
    assert all((im is None) == (name in broken) for (name, _), im in zip(FILES, images))


def test_rows_batch_with_a_refused_candidate():
    """``cgan_png_decode_rows``: its whole-stream path (no candidate, or refused by the row path) runs the lanes kernel."""
    files = list(rc.framed_files()[:3]) + list(rc.refused_files()) + list(lc.hand_built()) + [INTACT[0], BROKEN[16], BROKEN[30]]
    datas = [data for _, data in files]
    probed = [png.probe(data)[0] for data in datas]
    blob, descs, descs_dev = png.upload(list(zip(probed, datas)), "cuda")
    tables, tables_dev = png.row_tables(descs, datas, "cuda")
    out, status, path = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
    out, status, path = out.cpu().numpy(), status.cpu().tolist(), path.cpu().tolist()
    assert rc.REFUSED in path and rc.ROWS in path and rc.SERIAL in path
    for (name, data), d, s, p in zip(files[:-2], descs, status, path):
        assert s == pc.OK and np.array_equal(pixels_of(out, d), rc.model(data)["pixels"]), name
        assert p == rc.decode_rows_host(data)[2], name
    assert status[-2:] == [pc.CORRUPT, pc.CORRUPT]


def logged(fn):
    """The C-ABI calls ``fn`` makes, by name."""
    _lib.CALL_LOG = []
    try:
        fn()
        return sorted(what for what, _ in _lib.CALL_LOG)
    finally:
        _lib.CALL_LOG = None


def test_call_names():
    datas = [INTACT[0][1], INTACT[1][1]]
    probed = [png.probe(data)[0] for data in datas]
    blob, descs, descs_dev = png.upload(list(zip(probed, datas)), "cuda")
    assert logged(lambda: ops.png_decode(blob, descs, descs_dev)) == ["cgan_png_decode"]
    assert logged(lambda: ops.png_decode(blob, descs, descs_dev, subseq_bits=64)) == ["cgan_png_decode_lanes"]
    assert logged(lambda: ops.png_decode(blob, descs, descs_dev, lane_tokens=8)) == ["cgan_png_decode_lanes"]
    assert logged(lambda: ops.png_decode(blob, descs, descs_dev, subseq_bits=0)) == ["cgan_png_decode_lanes"]
    assert logged(lambda: png.decode(datas)) == ["cgan_png_decode"] + ["cgan_png_parse_host"] * 2 + ["cgan_png_stream_host"] * 2


def test_refusals_before_any_launch():
    datas = [INTACT[0][1]]
    blob, descs, descs_dev = png.upload([(png.probe(datas[0])[0], datas[0])], "cuda")
    for kw in ({"subseq_bits": 16}, {"subseq_bits": 288}, {"subseq_bits": -32}, {"lane_tokens": 0}, {"lane_tokens": 49}):
        with pytest.raises(RuntimeError, match="subseq_bits"):
            ops.png_decode(blob, descs, descs_dev, **kw)
    out, status = ops.png_decode(blob, descs, descs_dev, subseq_bits=256, lane_tokens=48)      # the largest values decode
    assert status.tolist() == [pc.OK] and torch.equal(png.image_view(out, descs[0]).cpu(), torch.from_numpy(pc.model(datas[0])["pixels"]))
