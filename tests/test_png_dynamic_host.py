"""Host side of the device PNG encoder's level 1: png_code_lengths is the host instantiation of the length-limited code
construction the band kernel runs (pure arithmetic, no device), and png_bound knows the level."""
import heapq

import numpy as np
import pytest


def huffman_cost(counts):
    """Sum of count * depth over an (unconstrained) Huffman tree, and the tree's depth."""
    heap = [(int(c), 0) for c in counts if c]                      # (weight, depth of the subtree)
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def check_lengths(counts, limit):
    import pseg_amd
    counts = np.asarray(counts, np.uint32)
    lens = pseg_amd.png_code_lengths(counts, limit)
    assert lens.dtype == np.uint8 and lens.shape == counts.shape
    assert np.array_equal(lens == 0, counts == 0)
    used = int((counts != 0).sum())
    if used == 0:
        return lens
    assert int(lens.max()) <= limit
    kraft = sum(2 ** (limit - int(l)) for l in lens if l)          # in units of 2^-limit: exact
    if used >= 2:
        assert kraft == 2 ** limit, (kraft, limit, counts, lens)
    else:
        assert kraft <= 2 ** limit
    cost = int((counts.astype(np.int64) * lens).sum())
    tree_cost, depth = huffman_cost(counts)
    if depth <= limit:
        assert cost == tree_cost, (cost, tree_cost, counts, lens)
    else:
        assert cost >= tree_cost
    return lens


@pytest.mark.parametrize("limit,nmax", [(15, 286), (7, 19)])
def test_code_lengths_random_histograms(limit, nmax):
    rng = np.random.default_rng(limit)
    for trial in range(300):
        n = int(rng.integers(1, nmax + 1))
        kind = trial % 4
        if kind == 0:
            c = rng.integers(0, 1000, n)
        elif kind == 1:
            c = rng.integers(0, 4, n)                                # many ties and zeros
        elif kind == 2:
            c = (rng.pareto(0.7, n) * 3).astype(np.int64)            # a few huge counts, a long tail: deep trees
        else:
            c = rng.integers(1, 1 << 20, n) * (rng.random(n) < 0.3)
        check_lengths(np.minimum(c, 1 << 22), limit)


@pytest.mark.parametrize("limit,nmax", [(15, 286), (7, 19)])
def test_code_lengths_single_symbol(limit, nmax):
    for n in (1, 2, nmax):
        for at in sorted({0, n // 2, n - 1}):
            c = np.zeros(n, np.uint32)
            c[at] = 77
            lens = check_lengths(c, limit)
            assert lens[at] == 1
    assert not check_lengths(np.zeros(nmax, np.uint32), limit).any()


@pytest.mark.parametrize("limit,n", [(15, 24), (7, 12)])
def test_code_lengths_fibonacci_forces_the_limiter(limit, n):
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    assert huffman_cost(fib)[1] > limit                             # the plain tree is n - 1 deep
    lens = check_lengths(fib, limit)
    assert int(lens.max()) == limit
    check_lengths(fib[::-1], limit)
    rng = np.random.default_rng(n)
    check_lengths(rng.permutation(fib), limit)
    c = np.zeros(19 if limit == 7 else 286, np.uint32)           # ... scattered among unused symbols
    c[rng.choice(c.size, n, replace=False)] = fib
    check_lengths(c, limit)


def test_code_lengths_rejects_bad_arguments():
    import pseg_amd
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.ones(287, np.uint32), 15)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.ones(10, np.uint32), 16)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.ones(10, np.uint32), 0)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.ones(9, np.uint32), 3)          # nine symbols have no code of three bits
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.zeros(0, np.uint32), 15)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_code_lengths(np.full(4, 2 ** 31, np.uint32), 15)


def _formula(H, W, ch, rows):
    """include/pseg.h: 80 + sum over the bands of (12 + n + n / 8 + 8)."""
    L = ch * W + 1
    total = 80
    for r0 in range(0, H, rows):
        n = min(rows, H - r0) * L
        total += 12 + n + n // 8 + 8
    return total


def test_bound_level1():
    import pseg_amd
    for H, W, ch in ((1, 1, 1), (10, 100, 3), (64, 64, 1), (300, 333, 3), (2048, 1536, 3), (40, 30000, 3), (5, 70000, 1)):
        L = ch * W + 1
        rows1 = min(H, max(1, 65536 // L))
        assert pseg_amd.png_bound(H, W, ch, 0, level=1) == _formula(H, W, ch, rows1), (H, W, ch)
        assert pseg_amd.png_bound(H, W, ch, 0, level=0) == pseg_amd.png_bound(H, W, ch, 0) == _formula(H, W, ch, min(H, max(1, 16384 // L)))
        for band_rows in (1, 2, 7, 16, 1000):
            assert pseg_amd.png_bound(H, W, ch, band_rows, level=1) == pseg_amd.png_bound(H, W, ch, band_rows) \
                == _formula(H, W, ch, min(H, band_rows)), (H, W, ch, band_rows)
    for level in (2, -1):
        assert pseg_amd.lib().pseg_png_bound_lv(10, 10, 3, 0, level) == 0
        with pytest.raises(pseg_amd.PsegError):
            pseg_amd.png_bound(10, 10, 3, 0, level=level)


def test_python_surface_level1():
    import inspect
    import pseg_amd
    from ocr4all_pixel_classifier.lib import output, predictor
    assert output.DEVICE_PNG_LEVEL == 0
    assert inspect.signature(predictor.Predictor.write_masks).parameters["level"].default is None
    assert inspect.signature(pseg_amd.png_encode).parameters["level"].default == 0
    assert inspect.signature(pseg_amd.masks_png).parameters["level"].default == 0
    assert inspect.signature(pseg_amd.png_bound).parameters["level"].default == 0
    assert inspect.signature(pseg_amd.Engine.predict_chain).parameters["png_level"].default == 0
    for sym in ("pseg_png_bound_lv", "pseg_png_encode_lv", "pseg_png_encode_device_lv", "pseg_masks_png_lv", "pseg_masks_png_device_u8_lv",
                "pseg_predict_chain_png_lv", "pseg_png_code_lengths"):
        assert sym in pseg_amd.EXPORTED_SYMBOLS and hasattr(pseg_amd.lib(), sym)
