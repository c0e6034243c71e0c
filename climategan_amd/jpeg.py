"""JPEG files from uint8 device images: ``ops.jpeg_encode`` (csrc/jpeg.hip) builds the files on the device,
``_files`` brings their bytes to the host (two waits, only the compressed bytes cross PCIe) and writes them.  There is no
host encoder behind it: a CPU tensor is refused.
"""
from . import _files, ops


def encode(img_u8, quality=90, subsampling="444"):
    """uint8 [N, H, W, C] device tensor (C = 1 or 3) -> list of N ``bytes``, each a complete baseline JPEG file.  ``quality``,
    ``subsampling``: see ``ops.jpeg_encode``."""
    return _files.to_bytes(*_files.fetch(*ops.jpeg_encode(img_u8, quality, subsampling)))


def write(img_u8, paths, quality=90, subsampling="444"):
    """Encode a batch on the device (see ``ops.jpeg_encode``) and write image i to ``paths[i]``."""
    _files.write_files("jpeg.write", *_files.fetch(*ops.jpeg_encode(img_u8, quality, subsampling)), paths)
