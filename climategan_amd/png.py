"""PNG files from uint8 device images: ``ops.png_encode`` (csrc/png.hip) builds the files on the device,
``_files`` brings their bytes to the host (two waits, only the compressed bytes cross PCIe) and writes them.  There is no
host encoder behind it: a CPU tensor is refused.
"""
from . import _files, ops


def encode(img_u8, level=1):
    """uint8 [N, H, W, C] device tensor (C = 1 or 3) -> list of N ``bytes``, each a complete PNG file.  ``level``: see
    ``ops.png_encode``."""
    return _files.to_bytes(*_files.fetch(*ops.png_encode(img_u8, level)))


def write(img_u8, paths, level=1):
    """Encode a batch on the device (at ``level``, see ``ops.png_encode``) and write image i to ``paths[i]``."""
    _files.write_files("png.write", *_files.fetch(*ops.png_encode(img_u8, level)), paths)
