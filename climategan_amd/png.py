"""PNG files from uint8 device images: ``ops.png_encode`` (csrc/png.hip) builds the files on the device,
``_files`` brings their bytes to the host (two waits, only the compressed bytes cross PCIe) and writes them.  There is no
host encoder behind it: a CPU tensor is refused.

The other way: ``probe`` reads a file's chunks on the host, ``decode`` uploads a batch of files' zlib streams
and inflates and unfilters them on the device (``ops.png_decode``), one wave per file with the stream's tokens decoded
across its 64 lanes (``inflate_params``).  Row-framed files (one
IDAT chunk per row, as ``encode`` writes them; ``probe`` reports them as ``rows == height``) are inflated one wave per row
(``ops.png_decode_rows``); ``python -m climategan_amd.repack_png`` turns a folder's PNG files into such files.
"""
import ctypes as C
from pathlib import Path

import torch

from . import _files, _lib, ops

STATUS_TEXT = {ops.PNG_UNSUPPORTED: "unsupported", ops.PNG_CORRUPT: "corrupt data"}


def encode(img_u8, level=1):
    """uint8 [N, H, W, C] device tensor (C = 1 or 3) -> list of N ``bytes``, each a complete PNG file.  ``level``: see
    ``ops.png_encode``."""
    return _files.to_bytes(*_files.fetch(*ops.png_encode(img_u8, level)))


def write(img_u8, paths, level=1):
    """Encode a batch on the device (at ``level``, see ``ops.png_encode``) and write image i to ``paths[i]``."""
    _files.write_files("png.write", *_files.fetch(*ops.png_encode(img_u8, level)), paths)


def probe(data):
    """The bytes of one file -> (descriptor, None) if the device decoder takes it (a ``_lib.PngDesc``: width, height,
    channels, bit depth, the length of its zlib stream, and ``rows``: the height if the IDAT chunks make the file a row-framed
    candidate, DESIGN 4.22, else 0), else (None, reason): not a PNG file, a kind of PNG outside DESIGN
    4.21's list (interlaced, palette, grey + alpha, fewer than 8 bits, 16-bit colour, animated), or broken chunks.  Host
    only."""
    data = bytes(data)
    lib = _lib.load()
    d, status = _lib.PngDesc(), C.c_int32(0)
    _lib.check(lib.cgan_png_parse_host(data, len(data), C.addressof(d), C.addressof(status)), "cgan_png_parse_host")
    if status.value != ops.PNG_OK:
        return None, lib.cgan_last_error().decode()
    return d, None


def stream_of(data, d):
    """The zlib stream of a probed file: its IDAT payloads one behind the other, as ``bytes``.  Host only."""
    data = bytes(data)
    buf = C.create_string_buffer(max(d.stream_bytes, 1))
    _lib.check(_lib.load().cgan_png_stream_host(data, len(data), C.addressof(d), buf, d.stream_bytes), "cgan_png_stream_host")
    return buf.raw[:d.stream_bytes]


def inflate_params():
    """How the device spreads a whole zlib stream over a wave's 64 lanes -> {"subseq_bits": the bits of a lane's
    subsequence, "lane_tokens": the most tokens a lane decodes in a window}: the compiled values ``decode`` runs with.
    ``ops.png_decode`` takes other values for a measurement.  Host only."""
    bits, tokens = ops.png_inflate_params()
    return {"subseq_bits": bits, "lane_tokens": tokens}


def _pixel_bytes(d):
    return d.width * d.height * d.channels * (d.bit_depth // 8)


def upload(descs_and_data, device):
    """[(descriptor, the file's bytes)] -> (blob, descs, descs_dev) as ``ops.png_decode`` takes them: the files' zlib streams
    16-byte aligned in one blob, the pixels 16-byte aligned in one output, one upload each for the bytes and for the
    descriptors."""
    descs = (_lib.PngDesc * len(descs_and_data))()
    blob, out_at = bytearray(), 0
    for k, (d, data) in enumerate(descs_and_data):
        d.blob_offset, d.out_offset = len(blob), out_at
        blob += stream_of(data, d)
        blob += bytes(-len(blob) % 16)
        out_at += -(-_pixel_bytes(d) // 16) * 16
        descs[k] = d
    return (torch.frombuffer(blob, dtype=torch.uint8).to(device), descs,
            torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(device))


def row_table(data, d):
    """The row offsets of one probed candidate (``d.rows != 0``) -> a ``c_uint32`` array of rows + 1 words: what a caller
    that assembles its own batch (the loaders) puts one file behind the other.  Host only."""
    data = bytes(data)
    table = (C.c_uint32 * (d.rows + 1))()
    _lib.check(_lib.load().cgan_png_row_table_host(data, len(data), C.addressof(d), table), "cgan_png_row_table_host")
    return table


def image_view(out, d):
    """File ``d``'s pixels in the output of ``ops.png_decode`` / ``ops.png_decode_rows``: uint8 [H, W, C], ``torch.uint16``
    [H, W, 1] for 16-bit grey"""
    px = out[d.out_offset:d.out_offset + _pixel_bytes(d)]
    if d.bit_depth == 16:
        px = px.view(torch.uint16)
    return px.view(d.height, d.width, d.channels)


def row_tables(descs, datas, device):
    """The row offsets of a batch's candidates (``descs[k].rows != 0``; ``datas[k]``: that file's bytes) as
    ``ops.png_decode_rows`` takes them -> (tables, tables_dev): one ``c_uint32`` array, every candidate's rows + 1 words one
    file behind the other, and the same words uploaded; (None, None) without a candidate."""
    words = sum(d.rows + 1 for d in descs if d.rows)
    if not words:
        return None, None
    tables, at, lib = (C.c_uint32 * words)(), 0, _lib.load()
    for d, data in zip(descs, datas):
        if d.rows:
            _lib.check(lib.cgan_png_row_table_host(data, len(data), C.addressof(d), C.byref(tables, 4 * at)), "cgan_png_row_table_host")
            at += d.rows + 1
    return tables, torch.frombuffer(bytearray(tables), dtype=torch.int32).to(device)


def try_decode(files, device="cuda"):
    """``decode`` without raising for a file's sake -> (images, reasons): ``images[i]`` is None for a file that was not
    decoded and ``reasons[i]`` says why."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("png.decode needs a device (got %s); there is no CPU path" % device)
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
        if any(d.rows for d in descs):                                        # row-framed files: one wave per row
            tables, tables_dev = row_tables(descs, [datas[i] for i, _ in taken], device)
            out, status, _ = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
        else:
            out, status = ops.png_decode(blob, descs, descs_dev)
        for (i, _), d, s in zip(taken, descs, status.tolist()):               # the one wait
            if s != ops.PNG_OK:
                reasons[i] = STATUS_TEXT[ops.PNG_CORRUPT]
            else:
                images[i] = image_view(out, d)
    return images, reasons


def decode(files, fallback=False, device="cuda"):
    """``files``: a list of ``bytes`` or paths of PNG files -> a list of device tensors, views into one allocation: uint8
    [H, W, C] with C = 1, 3 or 4, and ``torch.uint16`` [H, W, 1] for 16-bit grey.  One upload of the bytes, one of the
    descriptors, one wait (for the status words); a batch that holds a row-framed file uploads its row offsets
    too and goes through ``ops.png_decode_rows``.  A file the decoder does not take (``probe``) or reports as corrupt raises
    ``RuntimeError`` with its index and the reason -- unless ``fallback``: that file is then decoded by PIL on the host and
    uploaded."""
    images, reasons = try_decode(files, device)
    if reasons and not fallback:
        i = min(reasons)
        raise RuntimeError("png.decode: file %d: %s" % (i, reasons[i]))
    for i in reasons:
        import io

        import numpy as np
        from PIL import Image

        f = files[i]
        a = np.asarray(Image.open(io.BytesIO(bytes(f)) if isinstance(f, (bytes, bytearray, memoryview)) else f))
        images[i] = torch.from_numpy(a.reshape(a.shape[0], a.shape[1], -1).copy()).to(device)
    return images
