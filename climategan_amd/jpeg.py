"""JPEG files from uint8 device images: ``ops.jpeg_encode`` (csrc/jpeg.hip) builds the files on the device,
``_files`` brings their bytes to the host (two waits, only the compressed bytes cross PCIe) and writes them.  There is no
host encoder behind it: a CPU tensor is refused.

The other way: ``probe`` reads a baseline file's headers on the host, ``decode`` uploads a batch of files'
bytes (about a tenth of their pixels) and decodes them on the device (``ops.jpeg_decode``).
"""
import ctypes as C
from pathlib import Path

import torch

from . import _files, _lib, ops

STATUS_TEXT = {ops.JPEG_UNSUPPORTED: "unsupported", ops.JPEG_CORRUPT: "corrupt data",
               ops.JPEG_NOT_CONVERGED: "the entropy decode did not converge within its launches"}


def encode(img_u8, quality=90, subsampling="444"):
    """uint8 [N, H, W, C] device tensor (C = 1 or 3) -> list of N ``bytes``, each a complete baseline JPEG file.  ``quality``,
    ``subsampling``: see ``ops.jpeg_encode``."""
    return _files.to_bytes(*_files.fetch(*ops.jpeg_encode(img_u8, quality, subsampling)))


def write(img_u8, paths, quality=90, subsampling="444"):
    """Encode a batch on the device (see ``ops.jpeg_encode``) and write image i to ``paths[i]``."""
    _files.write_files("jpeg.write", *_files.fetch(*ops.jpeg_encode(img_u8, quality, subsampling)), paths)


def probe(data):
    """The bytes of one file -> (descriptor, None) if the device decoder takes it (a ``_lib.JpegDesc``: width, height, ncomp,
    luma sampling hs x vs, restart interval, scan offset and length, tables), else (None, reason): not a JPEG file, a kind of
    JPEG outside DESIGN 4.20's list (progressive, 12 bits, CMYK, ...), or broken headers.  Host only."""
    data = bytes(data)
    lib = _lib.load()
    d, status = _lib.JpegDesc(), C.c_int32(0)
    _lib.check(lib.cgan_jpeg_parse_host(data, len(data), C.addressof(d), C.addressof(status)), "cgan_jpeg_parse_host")
    if status.value != ops.JPEG_OK:
        return None, lib.cgan_last_error().decode()
    return d, None


def upload(descs_and_data, device):
    """[(descriptor, bytes)] -> (blob, descs, descs_dev) as ``ops.jpeg_decode`` takes them: the files 16-byte aligned in one
    blob, the pixels 16-byte aligned in one output, one upload each for the bytes and for the descriptors."""
    descs = (_lib.JpegDesc * len(descs_and_data))()
    blob, out_at = bytearray(), 0
    for k, (d, data) in enumerate(descs_and_data):
        d.blob_offset, d.out_offset = len(blob), out_at
        blob += data
        blob += bytes(-len(blob) % 16)
        out_at += -(-d.width * d.height * d.ncomp // 16) * 16
        descs[k] = d
    return (torch.frombuffer(blob, dtype=torch.uint8).to(device), descs,
            torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(device))


def image_view(out, d):
    """File ``d``'s uint8 [H, W, C] pixels in the output of ``ops.jpeg_decode``"""
    return out[d.out_offset:d.out_offset + d.width * d.height * d.ncomp].view(d.height, d.width, d.ncomp)


def try_decode(files, device="cuda", subseq_bytes=0):
    """``decode`` without raising for a file's sake -> (images, reasons): ``images[i]`` is None for a file that was not
    decoded and ``reasons[i]`` says why."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("jpeg.decode needs a device (got %s); there is no CPU path" % device)
    datas = [bytes(f) if isinstance(f, (bytes, bytearray, memoryview)) else Path(f).read_bytes() for f in files]
    images, reasons, taken = [None] * len(datas), {}, []
    for i, data in enumerate(datas):
        d, why = probe(data)
        if d is None:
            reasons[i] = why
        else:
            taken.append((i, d))
    if taken:
        blob, descs, descs_dev = upload([(d, datas[i]) for i, d in taken], device)
        out, status = ops.jpeg_decode(blob, descs, descs_dev, subseq_bytes)
        for (i, _), d, s in zip(taken, descs, status.tolist()):               # the one wait
            if s != ops.JPEG_OK:
                reasons[i] = STATUS_TEXT[ops.JPEG_NOT_CONVERGED if s & ops.JPEG_NOT_CONVERGED else ops.JPEG_CORRUPT]
            else:
                images[i] = image_view(out, d)
    return images, reasons


def decode(files, fallback=False, device="cuda", subseq_bytes=0):
    """``files``: a list of ``bytes`` or paths of baseline JPEG files -> a list of uint8 [H, W, C] device tensors (C = 1 or 3),
    views into one allocation.  One upload of the bytes, one of the descriptors, one wait (for the status words).  A file the
    decoder does not take (``probe``) or reports as corrupt or not converged raises ``RuntimeError`` with its index and the
    reason -- unless ``fallback``: that file is then decoded by PIL on the host and uploaded."""
    images, reasons = try_decode(files, device, subseq_bytes)
    if reasons and not fallback:
        i = min(reasons)
        raise RuntimeError("jpeg.decode: file %d: %s" % (i, reasons[i]))
    for i in reasons:
        import io

        import numpy as np
        from PIL import Image

        f = files[i]
        a = np.asarray(Image.open(io.BytesIO(bytes(f)) if isinstance(f, (bytes, bytearray, memoryview)) else f))
        images[i] = torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to(device)
    return images
