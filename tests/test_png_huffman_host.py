"""The code construction of the PNG encoder's level 2 on the host (``cgan_png_huffman_lengths``, csrc/png_huffman.h: the
same functions one lane of ``png_rows_kernel`` runs), against a ``heapq`` Huffman tree and the Kraft sum, and the
``--png_level`` option of apply_events.  No GPU."""
import heapq
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from climategan_amd import _lib
from climategan_amd.apply_events import parse_args


def lengths(counts, limit):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    out = np.full(len(counts), 99, dtype=np.uint8)
    _lib.check(_lib.load().cgan_png_huffman_lengths(counts.ctypes.data, len(counts), limit, out.ctypes.data),
               "cgan_png_huffman_lengths")
    return out.astype(np.int64)


def huffman(counts):
    """(cost, depth) of a heapq Huffman tree over the used symbols."""
    tick = itertools.count()
    heap = [(int(c), next(tick), 0) for c in counts if c]         # weight, tie-break, height
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], next(tick), max(a[2], b[2]) + 1))
    return cost, heap[0][2]


def fibonacci(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def histograms():
    rng = np.random.default_rng(0)
    out = []
    for k, n in enumerate((286, 286, 286, 19, 30, 2, 286)):                                     # random ones
        c = rng.integers(0, (3, 50, 4000, 40, 9, 5, 2)[k], n)
        c[rng.integers(0, n)] += 1                                                                  # never empty ...
        c[(np.flatnonzero(c)[0] + 1) % n] += 1                                                      # ... nor one symbol
        out.append(("random%d" % k, c, 15 if n > 19 else 7))
    out.append(("geometric", np.maximum(1, (6000 * 0.8 ** np.arange(286)).astype(np.int64)), 15))
    out.append(("two", [0, 7, 0, 0, 1], 15))
    out.append(("two_equal", [4, 4], 7))
    dominant = np.ones(286, dtype=np.int64)
    dominant[100] = 12000
    out.append(("dominant", dominant, 15))
    out.append(("dominant_sparse", [1, 0, 0, 100000, 0, 2, 1], 15))
    out.append(("fibonacci19", fibonacci(19), 15))
    out.append(("fibonacci10_limit7", fibonacci(10), 7))
    out.append(("full", np.ones(128, dtype=np.int64), 7))                                        # exactly 2^limit symbols
    return out


def test_fibonacci_premises():
    assert sum(fibonacci(19)) == 10945 and huffman(fibonacci(19))[1] == 18
    assert huffman(fibonacci(10))[1] == 9


@pytest.mark.parametrize("name,counts,limit", histograms(), ids=[h[0] for h in histograms()])
def test_huffman_lengths(name, counts, limit):
    counts = np.asarray(counts, dtype=np.int64)
    got = lengths(counts, limit)
    used = counts > 0
    assert used.sum() >= 2
    assert np.all(got[~used] == 0)
    assert np.all((got[used] >= 1) & (got[used] <= limit))
    assert sum(Fraction(1, 2 ** int(l)) for l in got[used]) == 1                                  # complete, exactly
    cost = int((counts * got).sum())
    best, depth = huffman(counts)
    print("%s: %d used, cost %d, Huffman %d (depth %d), limit %d" % (name, used.sum(), cost, best, depth, limit))
    if depth <= limit:
        assert cost == best
    else:
        assert best <= cost <= int(counts.sum()) * math.ceil(math.log2(len(counts)))
    assert np.array_equal(lengths(counts, limit), got)                                            # the same twice
    order = np.lexsort((np.arange(len(counts)), counts))                                          # by (count, symbol)
    order = order[used[order]]
    assert np.all(np.diff(got[order]) <= 0)            # rarer never shorter, and among equal counts the lower symbol


def test_one_symbol_and_refusals():
    assert lengths([0, 0, 9, 0], 15).tolist() == [0, 0, 1, 0]
    assert lengths([0, 0, 0], 15).tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match="limit"):
        lengths([1, 2, 3], 16)
    with pytest.raises(RuntimeError, match="limit"):
        lengths([1, 2, 3], 0)
    with pytest.raises(RuntimeError, match="do not fit"):
        lengths([1, 1, 1, 1, 1], 2)
    with pytest.raises(RuntimeError, match="sum"):
        lengths([2 ** 31, 2 ** 31, 1], 15)


def test_png_level_option():
    base = ["-i", "photos", "-r", "run"]
    assert parse_args(base).png_level == 1
    assert parse_args(base + ["--png_level", "2"]).png_level == 2
    assert parse_args(base + ["--png_level", "1"]).png_level == 1
    for bad in ("3", "0"):
        with pytest.raises(SystemExit):
            parse_args(base + ["--png_level", bad])
