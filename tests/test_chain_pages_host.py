"""How pseg_predict_chain_pages_png cuts a page list into units (pseg_chain_units): host logic, no GPU."""
import ctypes

import numpy as np
import pytest


def _random_shapes(rng, n):
    """Runs of equal shapes of random lengths, a few distinct shapes."""
    pool = [(96, 64), (70, 50), (160, 224), (33, 97)]
    out = []
    while len(out) < n:
        out += [pool[int(rng.integers(0, len(pool)))]] * int(rng.integers(1, 12))
    return out[:n]


def test_without_out_shapes_the_units_are_batch_units():
    from pseg_amd import engine as E
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 3, 7, 31, 64):
        for cap in (1, 2, 3, 8):
            shapes = _random_shapes(rng, n)
            assert E.chain_units(shapes, cap=cap) == E.batch_units(shapes, cap=cap), (n, cap)
            assert E.chain_units(shapes, out_shapes=[None] * n, cap=cap) == E.batch_units(shapes, cap=cap), (n, cap)
    assert E.chain_units([]) == [] and E.chain_units([(5, 7)]) == [(0, 1)]


def test_an_out_shape_alone_splits_a_unit():
    from pseg_amd import engine as E
    shapes = [(96, 64)] * 12
    same = [(167, 105)] * 12
    assert E.chain_units(shapes, same, cap=4) == E.batch_units(shapes, cap=4)
    split = list(same)
    split[5] = (167, 106)
    units = E.chain_units(shapes, split, cap=4)
    assert units != E.batch_units(shapes, cap=4)
    for first, count in units:                                      # page 5 shares a unit with nobody
        assert (first, count) == (5, 1) or not (first <= 5 < first + count)
    assert (5, 1) in units
    none_vs_zero = [None] * 6 + [(0, 0)] * 6                        # None and 0 both mean "no rescale": one key
    assert E.chain_units(shapes, none_vs_zero, cap=4) == E.batch_units(shapes, cap=4)


@pytest.mark.parametrize("cap", [1, 2, 5, 8])
def test_cap_is_respected_and_the_units_tile_the_list_in_order(cap):
    from pseg_amd import engine as E
    rng = np.random.default_rng(cap)
    for n in (1, 9, 40):
        shapes = _random_shapes(rng, n)
        outs = [(s[0] + int(rng.integers(0, 2)), s[1]) for s in shapes]
        units = E.chain_units(shapes, outs, cap=cap)
        pos = 0
        for first, count in units:
            assert first == pos and 1 <= count <= cap
            assert len({(shapes[k], outs[k]) for k in range(first, first + count)}) == 1
            pos += count
        assert pos == n


def test_c_abi_errors_and_room():
    from pseg_amd import engine as E
    L = E.lib()
    I = ctypes.c_int * 4
    H, W = I(8, 8, 8, 9), I(8, 8, 8, 8)
    first, count = I(), I()
    assert L.pseg_chain_units(4, H, W, None, None, 0, first, count, 4) == -1          # cap < 1
    assert L.pseg_chain_units(4, None, W, None, None, 2, first, count, 4) == -1
    assert L.pseg_chain_units(-1, H, W, None, None, 2, first, count, 4) == -1
    nu = L.pseg_chain_units(4, H, W, None, None, 8, None, None, 0)                    # counting needs no room
    assert nu == len(E.batch_units([(8, 8)] * 3 + [(9, 8)], cap=8))
    assert L.pseg_chain_units(4, H, W, None, None, 8, first, count, nu - 1) == -1 and b"room" in L.pseg_last_error()
    assert "pseg_predict_chain_pages_png" in E.EXPORTED_SYMBOLS and "pseg_chain_units" in E.EXPORTED_SYMBOLS
