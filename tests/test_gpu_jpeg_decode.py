"""The device JPEG decoder (csrc/jpeg_decode.hip) against the model of ``tests/jpeg_decode_model.py``: the
coefficients of ``cgan_jpeg_decode_coefficients`` equal the model reader's and the pixels of ``cgan_jpeg_decode_u8`` equal the
integer reconstruction's, exactly, on the host corpus of ``test_jpeg_decode_host.py``, on H, W in {1, 7, 8, 9, 16, 17, 33}^2
and three long shapes, and on a 600 x 900 file whose scan spans 15 workgroups' worth of subsequences; forced subsequence
sizes, the round trip with the project's encoder, batch independence, broken files against the host twin, refusals."""
import numpy as np
import pytest
import torch

import jpeg_decode_corpus as jc
import jpeg_decode_model as dm
import jpeg_model as jm
from climategan_amd import jpeg, ops

pytestmark = pytest.mark.gpu


def device_decode(datas, subseq=0, coefficients=False):
    """The files in ONE call -> (per file: int16 coefficients or uint8 [h, w, c] pixels, as numpy; the status words)."""
    descs = []
    for data in datas:
        d, why = jpeg.probe(data)
        assert d is not None, why
        descs.append(d)
    blob, descs, descs_dev = jpeg.upload(list(zip(descs, datas)), "cuda")
    out, status = ops.jpeg_decode(blob, descs, descs_dev, subseq, coefficients=coefficients)
    out, results, at = out.cpu().numpy(), [], 0
    for d in descs:
        if coefficients:
            n = 64 * ops.jpeg_blocks(d)
            results.append(out[at:at + n])
            at += n
        else:
            results.append(out[d.out_offset:d.out_offset + d.width * d.height * d.ncomp].reshape(d.height, d.width, d.ncomp))
    return results, status.cpu().tolist()


def model_pixels(data):
    r = jc.model(data)
    return dm.reconstruct(r["coef"], r["h"], r["w"], r["c"], r["hs"], r["vs"], r["qtables"])


def check(files, subseq=0):
    datas = [data for _, data in files]
    coefs, status = device_decode(datas, subseq, coefficients=True)
    assert status == [0] * len(files)
    for (name, data), got in zip(files, coefs):
        assert np.array_equal(got, jc.model(data)["coef"]), name
    pixels, status = device_decode(datas, subseq)
    assert status == [0] * len(files)
    for (name, data), got in zip(files, pixels):
        assert np.array_equal(got, model_pixels(data)), name


def test_host_corpus():
    check(jc.host_corpus())


def test_sizes():
    check(jc.gpu_sizes_corpus())


def test_scan_over_many_workgroups():
    data = jc.big_file()
    d, _ = jpeg.probe(data)
    assert d.scan_bytes > 8 * 256 * 128                # more tiles than sync launches can hand states across one by one
    check((("noise-600x900", data),))


@pytest.mark.parametrize("subseq", (4, 16))
def test_forced_subsequence_sizes(subseq):
    files = [f for f in jc.gpu_sizes_corpus() if jc.model(f[1])["h"] <= 33 and jc.model(f[1])["w"] <= 33]
    assert len(files) == 49
    datas = [data for _, data in files]
    for coefficients in (True, False):
        want, s0 = device_decode(datas, 0, coefficients)
        got, s1 = device_decode(datas, subseq, coefficients)
        assert s0 == s1 == [0] * len(files)
        for (name, _), a, b in zip(files, want, got):
            assert np.array_equal(a, b), name


@pytest.mark.parametrize("sub", ("444", "420"))
def test_round_trip_with_the_encoder(sub):
    imgs = np.stack([jm.make_image(kind, 72, 100, 3) for kind in jm.CONTENTS])
    x = torch.from_numpy(imgs).cuda()
    files = jpeg.encode(x, quality=90, subsampling=sub)
    want = ops.jpeg_coefficients(x, 90, sub).cpu().numpy()
    got, status = device_decode(files, coefficients=True)
    assert status == [0] * len(files)
    for i in range(len(files)):
        assert np.array_equal(got[i], want[i]), jm.CONTENTS[i]


def test_batch_independence():
    files = list(jc.gpu_sizes_corpus()[5::7]) + list(jc.host_corpus()[3::29])
    together, status = device_decode([data for _, data in files])
    assert status == [0] * len(files) and len({jc.model(d)["interval"] for _, d in files}) > 2
    for (name, data), want in zip(files, together):
        alone, status = device_decode([data])
        assert status == [0] and np.array_equal(alone[0], want), name


def test_cut_and_changed_files():
    """The files the sanitizer program has passed on the CPU: the device's status is the host twin's, equal coefficients where
    both decode, and the intact files of the same batch stay exact."""
    intact = list(jc.host_corpus()[::40])
    broken = [(name, data) for name, data in jc.broken_files() if jc.parse_host(data)[1] == jc.OK]
    assert len(broken) >= 20
    files = intact[:2] + broken + intact[2:]
    coefs, status = device_decode([data for _, data in files], coefficients=True)
    for (name, data), got, s in zip(files, coefs, status):
        want, host_status, _ = jc.decode_host(data, jc.parse_host(data)[0])
        assert s == host_status, name
        if s == 0:
            assert np.array_equal(got, want), name
    for (name, data), got, s in zip(files, coefs, status):
        if (name, data) in intact:
            assert s == 0 and np.array_equal(got, jc.model(data)["coef"]), name


def test_refusals():
    good = jc.host_corpus()[0][1]
    for name, data in jc.unsupported_files():
        d, why = jpeg.probe(data)
        assert d is None and why, name
        with pytest.raises(RuntimeError, match="file 1"):
            jpeg.decode([good, data])
    images = jpeg.decode([good, jc.unsupported_files()[0][1]], fallback=True)
    assert np.array_equal(images[0].cpu().numpy(), model_pixels(good)) and tuple(images[1].shape) == (33, 41, 3)
    with pytest.raises(RuntimeError):
        jpeg.decode([good], device="cpu")
    d, _ = jpeg.probe(good)
    blob, descs, descs_dev = jpeg.upload([(d, good)], "cuda")
    with pytest.raises(RuntimeError):
        ops.jpeg_decode(blob[:-40], descs, descs_dev)                   # the scan reaches behind the blob's end
    with pytest.raises(RuntimeError):
        ops.jpeg_decode(blob, descs, descs_dev, subseq_bytes=3)
    descs[0].hs = 3
    with pytest.raises(RuntimeError):
        ops.jpeg_decode(blob, descs, descs_dev)
