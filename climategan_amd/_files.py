"""Files the device encoders built (``ops.png_encode``, ``ops.jpeg_encode``: ``buf`` uint8 [N, bound], ``sizes`` int64 [N])
brought to the host and written.

Only the compressed bytes cross PCIe.  How many they are is known on the device alone, so a batch costs two waits: one for
the N file lengths (8 N bytes; this is where the host waits for the encoder), one for a single copy of the first
``max(lengths)`` bytes of every row of the output buffer into pinned memory.
"""
import torch

_PINNED = None


def _pinned(nbytes):
    """The pinned staging buffer, kept and grown between calls (pinning memory costs far more than the copy it serves)."""
    global _PINNED
    if _PINNED is None or _PINNED.numel() < nbytes:
        _PINNED = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
    return _PINNED[:nbytes]


def fetch(buf, sizes):
    """-> (host uint8 array [N, max length] in the pinned buffer, list of N lengths); valid until the next call."""
    lengths = sizes.cpu().tolist()
    n, longest = buf.shape[0], max(lengths)
    host = _pinned(n * longest).view(n, longest)
    host.copy_(buf[:, :longest], non_blocking=True)
    torch.cuda.current_stream(buf.device).synchronize()
    return host.numpy(), lengths


def to_bytes(host, lengths):
    """-> list of N ``bytes``, copies that outlive the pinned buffer's next use."""
    return [host[i, :k].tobytes() for i, k in enumerate(lengths)]


def write_files(what, host, lengths, paths):
    """File i to ``paths[i]``.  ``what``: the caller's name, for the refusal."""
    paths = list(paths)
    if len(paths) != len(lengths):
        raise ValueError("%s: %d images but %d paths" % (what, len(lengths), len(paths)))
    for i, (path, k) in enumerate(zip(paths, lengths)):
        with open(path, "wb") as f:
            f.write(memoryview(host[i, :k]))
