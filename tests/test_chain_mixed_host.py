"""How pseg_predict_chain_pages_mixed_png cuts a list of pages of different shapes (pseg_chain_units_mixed): host logic, no GPU."""
import ctypes

import numpy as np


def _canvas(s):
    return (-(-s[0] // 32) * 32, -(-s[1] // 32) * 32)


def _lists():
    rng = np.random.default_rng(7)
    out = [[(96, 64), (160, 224), (70, 50), (33, 1), (65, 47), (129, 193), (90, 33), (150, 200), (1, 37)], [(5, 7)], []]
    for n in (2, 9, 23, 40):
        # shapes around three canvases, interleaved at random
        out.append([(int(rng.integers(60, 130)), int(rng.integers(30, 100))) for _ in range(n)])
    return out


def test_order_and_units():
    from pseg_amd import engine as E
    for shapes in _lists():
        n = len(shapes)
        for cap in (1, 2, 4, 8):
            order, units = E.chain_units_mixed(shapes, cap=cap)
            assert sorted(order) == list(range(n)), (shapes, cap)
            # stable: canvases by first appearance, list order within a canvas
            first = {}
            for k, s in enumerate(shapes):
                first.setdefault(_canvas(s), len(first))
            assert order == sorted(range(n), key=lambda k: (first[_canvas(shapes[k])], k)), (shapes, cap)
            # the units tile the permuted list, hold at most `cap` pages, and every unit's pages share a canvas
            assert [u[0] for u in units] == [sum(c for _, c in units[:k]) for k in range(len(units))]
            assert sum(c for _, c in units) == n and all(1 <= c <= cap for _, c in units)
            for f, c in units:
                assert len({_canvas(shapes[order[f + k]]) for k in range(c)}) == 1, (shapes, cap, f, c)
            # ... and are chain_units' cut of the permuted canvas list
            assert units == E.chain_units([_canvas(shapes[k]) for k in order], cap=cap), (shapes, cap)


def test_the_issue_list_has_four_interleaved_canvases():
    from pseg_amd import engine as E
    shapes = _lists()[0]
    order, units = E.chain_units_mixed(shapes, cap=4)
    assert order == [0, 2, 4, 6, 1, 5, 7, 3, 8]
    assert [_canvas(shapes[k]) for k in order] == [(96, 64)] * 4 + [(160, 224)] * 3 + [(64, 32), (32, 64)]
    # the ramp of the list's head (1, 2, ...), then whole runs: the middle canvas is one unit of three pages
    assert units == [(0, 1), (1, 2), (3, 1), (4, 3), (7, 1), (8, 1)]


def test_one_shape_is_the_identity():
    from pseg_amd import engine as E
    for n in (1, 5, 32, 33):
        for cap in (1, 2, 4, 8):
            order, units = E.chain_units_mixed([(70, 50)] * n, cap=cap)
            assert order == list(range(n)) and units == E.chain_units([(70, 50)] * n, cap=cap)
    # shapes of one canvas are one run, whatever their own sizes
    order, units = E.chain_units_mixed([(70, 50), (65, 47), (96, 64), (90, 33)], cap=8)
    assert order == [0, 1, 2, 3] and units == E.chain_units([(96, 64)] * 4, cap=8)
    assert E.chain_units_mixed([]) == ([], [])


def test_argument_errors():
    from pseg_amd import engine as E
    import pseg_amd
    L = pseg_amd.lib()
    I = ctypes.c_int * 4
    H, W = I(70, 160, 65, 150), I(50, 224, 47, 200)
    order, first, count = I(), I(), I()
    assert L.pseg_chain_units_mixed(4, H, W, 0, order, first, count, 4) == -1          # cap < 1
    assert L.pseg_chain_units_mixed(4, None, W, 2, order, first, count, 4) == -1
    assert L.pseg_chain_units_mixed(4, H, None, 2, order, first, count, 4) == -1
    assert L.pseg_chain_units_mixed(-1, H, W, 2, order, first, count, 4) == -1
    assert L.pseg_chain_units_mixed(4, I(70, 0, 65, 150), W, 2, order, first, count, 4) == -1 and b"page 1" in L.pseg_last_error()
    nu = L.pseg_chain_units_mixed(4, H, W, 8, None, None, None, 0)                     # counting needs no room
    assert nu == len(E.chain_units_mixed([(70, 50), (160, 224), (65, 47), (150, 200)], cap=8)[1]) == 4   # two canvases, ramps 1 + 1 each
    assert L.pseg_chain_units_mixed(4, H, W, 8, order, first, count, nu - 1) == -1 and b"room" in L.pseg_last_error()
    assert L.pseg_chain_units_mixed(0, None, None, 8, None, None, None, 0) == 0
    assert "pseg_predict_chain_pages_mixed_png" in E.EXPORTED_SYMBOLS and "pseg_chain_units_mixed" in E.EXPORTED_SYMBOLS
