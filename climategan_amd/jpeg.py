"""JPEG files from uint8 device images: ``ops.jpeg_encode`` (csrc/jpeg.hip) builds the files on the device,
this module brings their bytes to the host and writes them.  There is no host encoder behind it: a CPU tensor is refused.

As in ``png.py`` only the compressed bytes cross PCIe, in two waits: one for the N file lengths, one for a single copy of the
first ``max(lengths)`` bytes of every row of the output buffer into pinned memory.  (The fetch is restated here rather than
shared: ``png.py`` stays as it is.)
"""
import torch

from . import ops

_PINNED = None


def _pinned(nbytes):
    """A pinned staging buffer, kept and grown between calls (pinning memory costs far more than the copy it serves)."""
    global _PINNED
    if _PINNED is None or _PINNED.numel() < nbytes:
        _PINNED = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
    return _PINNED[:nbytes]


def _fetch(img_u8, quality, subsampling):
    """-> (host uint8 array [N, max length] in the pinned buffer, list of N lengths); valid until the next call."""
    buf, sizes = ops.jpeg_encode(img_u8, quality, subsampling)
    lengths = sizes.cpu().tolist()
    n, longest = buf.shape[0], max(lengths)
    host = _pinned(n * longest).view(n, longest)
    host.copy_(buf[:, :longest], non_blocking=True)
    torch.cuda.current_stream(img_u8.device).synchronize()
    return host.numpy(), lengths


def encode(img_u8, quality=90, subsampling="444"):
    """uint8 [N, H, W, C] device tensor (C = 1 or 3) -> list of N ``bytes``, each a complete baseline JPEG file.  ``quality``,
    ``subsampling``: see ``ops.jpeg_encode``."""
    host, lengths = _fetch(img_u8, quality, subsampling)
    return [host[i, :k].tobytes() for i, k in enumerate(lengths)]


def write(img_u8, paths, quality=90, subsampling="444"):
    """Encode a batch on the device (see ``ops.jpeg_encode``) and write image i to ``paths[i]``."""
    paths = list(paths)
    if len(paths) != img_u8.shape[0]:
        raise ValueError("jpeg.write: %d images but %d paths" % (img_u8.shape[0], len(paths)))
    host, lengths = _fetch(img_u8, quality, subsampling)
    for i, (path, k) in enumerate(zip(paths, lengths)):
        with open(path, "wb") as f:
            f.write(memoryview(host[i, :k]))
