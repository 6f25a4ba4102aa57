"""The despeckling without a GPU: pseg_despeckle_maps_host -- a two-pass union-find over the page, the second implementation beside
the device's tile scheme -- against the scipy.ndimage restatement of tests/despeckle_cases.py, maps and counts, array_equal
throughout; idempotence; every refusal; the max_area rule; the arguments of the Python entries."""
import ctypes

import numpy as np
import pytest

import despeckle_cases as C


def _host(cases, counts=True):
    import pseg_amd
    return pseg_amd.despeckle_maps([c[1] for c in cases], [pseg_amd.Despeckle(c[2], c[3]) for c in cases], host=True, counts=counts)


def _assert_equal(cases, outs, cnt):
    assert len(outs) == len(cases) and cnt.shape == (len(cases), 3) and cnt.dtype == np.int64
    for k, c in enumerate(cases):
        want, wc = C.restated(c[1], c[2], c[3])
        assert outs[k].dtype == np.uint8 and outs[k].shape == c[1].shape, c[0]
        assert np.array_equal(outs[k], want), (c[0], int((outs[k] != want).sum()))
        assert np.array_equal(cnt[k], wc), (c[0], cnt[k], wc)


def test_symbols_and_geometry():
    from pseg_amd import engine as E
    for sym in ("pseg_despeckle_maps", "pseg_despeckle_maps_host", "pseg_despeckle_geometry"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    th, tw, slots, run_cap = E.despeckle_geometry()
    assert th >= 1 and tw >= 1 and slots >= 2 * (th + tw) - 4 and run_cap >= th * ((tw + 1) // 2)
    assert ctypes.sizeof(E.DESPECKLE) == 8


def test_host_entry_equals_the_restatement_over_the_grid():
    cases = C.grid_cases()
    assert len(cases) == len(C.SHAPES) * len(C.CONNECTIVITIES) * len(C.AREAS) * len(C.DENSITIES)
    outs, cnt = _host(cases)
    _assert_equal(cases, outs, cnt)
    # the grid is not a grid of trivial results: many cases erase something and keep something
    assert sum(cnt[k][0] > 0 and cnt[k][2] > 0 for k in range(len(cases))) > len(cases) // 4
    # without the counts, and the entries one by one
    assert all(np.array_equal(a, b) for a, b in zip(_host(cases, counts=False), outs))
    for k in range(150, 160):
        o, c = _host([cases[k]])
        assert np.array_equal(o[0], outs[k]) and np.array_equal(c[0], cnt[k])


def test_hand_placed_cases():
    cases = C.hand_cases()
    outs, cnt = _host(cases)
    _assert_equal(cases, outs, cnt)
    for k, c in enumerate(cases):
        if c[4] is not None:
            assert list(cnt[k]) == c[4], (c[0], cnt[k])
    by = {c[0]: outs[k] for k, c in enumerate(cases)}
    assert not by["checkerboard c=4"].any() and np.array_equal(by["checkerboard c=8"], cases[[c[0] for c in cases].index("checkerboard c=8")][1])
    assert by["all ink c=4"].all() and not by["all ink, erased c=8"].any()
    assert set(np.unique(by["bytes other than 1 c=8"])) <= {0, 1}


def test_idempotent_and_in_place():
    import pseg_amd
    cases = C.grid_cases(seed=5, shapes=[(33, 63), (70, 50)]) + [c[:4] for c in C.hand_cases()]
    outs, cnt = _host(cases)
    again, cnt2 = _host([(c[0], o, c[2], c[3]) for c, o in zip(cases, outs)])
    for k, c in enumerate(cases):
        assert np.array_equal(again[k], outs[k]), c[0]
        assert list(cnt2[k]) == [0, 0, cnt[k][2]], c[0]
    # out may be the input
    L = pseg_amd.lib()
    from pseg_amd import engine as E
    m = cases[7][1].copy()
    p = (ctypes.c_void_p * 1)(m.ctypes.data)
    assert L.pseg_despeckle_maps_host(1, p, (ctypes.c_int * 1)(m.shape[0]), (ctypes.c_int * 1)(m.shape[1]),
                                      (E.DESPECKLE * 1)(E.DESPECKLE(cases[7][2], cases[7][3])), p, None) == 0
    assert np.array_equal(m, outs[7])


def test_counts_against_numpy():
    rng = np.random.default_rng(17)
    m = C.random_map(rng, (120, 150), 0.25)
    for conn in C.CONNECTIVITIES:
        for a in (1, 3, 20):
            (out,), cnt = _host([("", m, a, conn)])
            assert cnt[0][1] == int((m != 0).sum()) - int(out.sum())          # pixels erased
            total = C.ndimage.label(m != 0, C.CROSS if conn == 4 else C.ONES)[1]
            assert cnt[0][0] + cnt[0][2] == total
            assert cnt[0][2] == C.ndimage.label(out, C.CROSS if conn == 4 else C.ONES)[1]


def test_refusals_leave_the_outputs_untouched():
    import pseg_amd
    C.refusals(pseg_amd.lib(), host=True)


def test_wrapper_arguments():
    import pseg_amd
    from pseg_amd import PsegError, Despeckle
    for bad in (0, -1, (1 << 24) + 1, 2.5, True, "3"):
        with pytest.raises((PsegError, ValueError, TypeError)):
            Despeckle(bad)
    for bad in (3, 0, 6, True, None, "8"):
        with pytest.raises(PsegError):
            Despeckle(4, bad)
    assert Despeckle(4.0).max_area == 4 and Despeckle(1 << 24).max_area == 1 << 24
    assert Despeckle() == Despeckle(None, 8) and Despeckle(3, 4) != Despeckle(3, 8) and hash(Despeckle(3)) == hash(Despeckle(3, 8))
    assert repr(Despeckle(3, 4)) == "Despeckle(max_area=3, connectivity=4)"
    assert Despeckle().resolved(40) == Despeckle(25, 8) and Despeckle(7, 4).resolved(40) == Despeckle(7, 4)
    m = np.zeros((4, 5), np.uint8)
    with pytest.raises(PsegError, match="line height"):
        pseg_amd.despeckle_maps([m], Despeckle(), host=True)
    with pytest.raises(PsegError, match="one entry per map"):
        pseg_amd.despeckle_maps([m, m], [Despeckle(2)], host=True)
    with pytest.raises(PsegError, match="map 1"):
        pseg_amd.despeckle_maps([m, m], [Despeckle(2), 5], host=True)
    with pytest.raises(PsegError, match="map 0"):
        pseg_amd.despeckle_maps([np.zeros((2, 3, 4), np.uint8)], Despeckle(2), host=True)
    assert pseg_amd.despeckle_maps([], Despeckle(2), host=True) == []
    outs, cnt = pseg_amd.despeckle_maps([], Despeckle(2), host=True, counts=True)
    assert outs == [] and cnt.shape == (0, 3)
    # None: the map comes back as it is
    b = np.arange(20, dtype=np.uint8).reshape(4, 5)
    outs, cnt = pseg_amd.despeckle_maps([b, b], [None, Despeckle(100)], host=True, counts=True)
    assert np.array_equal(outs[0], b) and not outs[1].any() and list(cnt[0]) == [0, 0, 0] and list(cnt[1]) == [1, 19, 0]
    # a bool map and a non-contiguous one
    v = np.ones((6, 8), bool)[:, ::2]
    assert pseg_amd.despeckle_maps([v], Despeckle(23), host=True)[0].all() and not pseg_amd.despeckle_maps([v], Despeckle(24), host=True)[0].any()


def test_despeckle_area():
    import pseg_amd
    from pseg_amd import PsegError
    for lh, want in ((1, 1), (7.9, 1), (15, 1), (16, 4), (23.4, 4), (23.6, 9), (40, 25), (64, 64), (100, 144)):
        assert pseg_amd.despeckle_area(lh) == want == max(1, int(round(lh)) // 8) ** 2
    for bad in (0, -3, float("nan"), float("inf"), None):
        with pytest.raises(PsegError):
            pseg_amd.despeckle_area(bad)


def test_front_end_arguments():
    """prepare_scans' despeckle= is checked on the host, and the C entry refuses a bad entry before it looks for a device."""
    import pseg_amd
    from pseg_amd import engine as E
    D, Err = pseg_amd.Despeckle, pseg_amd.PsegError
    for sym in ("pseg_prepare_scans_clean", "pseg_predict_chain_scans_clean_png"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    g = np.zeros((6, 5), np.uint8)
    with pytest.raises(Err, match="one entry per scan"):
        E.prepare_scans([g], [1.0], despeckle=[D(3), D(3)])
    with pytest.raises(Err, match="line height"):
        E.prepare_scans([g], [1.0], despeckle=D())
    with pytest.raises(Err, match="scan 0"):
        E.prepare_scans([g], [1.0], despeckle=["despeckle"])
    L = E.lib()
    table, keep, plans = E.scan_table([g], [1.0])
    out = [np.full(plans[0][:2], 0xA5, np.uint8) for _ in range(2)]
    P = ctypes.c_void_p * 1
    for bad, word in ((E.DESPECKLE(-2, 8), b"max_area"), (E.DESPECKLE((1 << 24) + 1, 8), b"max_area"), (E.DESPECKLE(4, 3), b"connectivity")):
        assert L.pseg_prepare_scans_clean(0, 1, table, None, (E.DESPECKLE * 1)(bad), P(out[0].ctypes.data), P(out[1].ctypes.data), None) == -1
        assert b"scan 0" in L.pseg_last_error() and word in L.pseg_last_error() and all((o == 0xA5).all() for o in out)


def test_loader_and_predictor_validate_despeckle():
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    assert DatasetLoader(6, None).despeckle is None
    d = pseg_amd.Despeckle()
    assert DatasetLoader(6, None, despeckle=d).despeckle is d
    for bad in ("despeckle", 15, (15, 8)):
        with pytest.raises(Exception, match="despeckle"):
            DatasetLoader(6, None, despeckle=bad)
        with pytest.raises(Exception, match="despeckle"):
            next(Predictor.write_masks_scans(None, [], None, "nowhere", despeckle=bad))      # refused before anything is touched
