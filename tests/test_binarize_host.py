"""The adaptive binarisation without a GPU: pseg_binarize_scans_host -- the decision function and the integer sums the device kernels
are compiled from -- against the NumPy restatement of tests/binarize_cases.py, ink maps and float64 thresholds bit for bit; every
refusal; the window rule; the arguments of the Python entries."""
import ctypes

import numpy as np
import pytest

import binarize_cases as C


def _host(cases):
    import pseg_amd
    how = [None if c[2] == 0 else pseg_amd.Sauvola(c[2], c[3], c[4]) for c in cases]
    return pseg_amd.binarize_scans([c[1] for c in cases], how, host=True, thresholds=True)


def _assert_equal(cases, got, want):
    assert len(got) == len(want) == len(cases)
    for c, (ink, T), (rink, rT) in zip(cases, got, want):
        assert ink.dtype == np.uint8 and T.dtype == np.float64 and ink.shape == T.shape == c[1].shape, c[0]
        assert np.array_equal(ink, rink), (c[0], int((ink != rink).sum()))
        assert np.array_equal(T, rT), (c[0], int((T != rT).sum()))


def test_symbols_and_geometry():
    from pseg_amd import engine as E
    for sym in ("pseg_binarize_scans", "pseg_binarize_scans_host", "pseg_binarize_geometry", "pseg_prepare_scans_bin", "pseg_predict_chain_scans_bin_png"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    seg, band, tile, vec = E.binarize_geometry()
    assert seg % 2 == 0 and seg - 254 > 0 and band >= 1 and tile >= 1 and vec == 16
    assert ctypes.sizeof(E.BINARIZE) == 24


def test_host_entry_equals_the_restatement_over_the_grid():
    cases = C.grid_cases()
    assert len(cases) == len(C.SHAPES) * len(C.WINDOWS) * len(C.KS) * len(C.DENSITIES)
    want = C.restated(cases)
    _assert_equal(cases, _host(cases), want)
    # the grid is not a grid of trivial maps: most cases hold ink and paper
    assert sum(0 < r[0].mean() < 1 for r in want) > len(cases) // 2
    # a list that mixes fixed and adaptive entries, and the entries one by one
    mixed = [(c[0], c[1], 0 if k % 3 == 0 else c[2], c[3], c[4]) for k, c in enumerate(cases[100:130])]
    got = _host(mixed)
    _assert_equal(mixed, got, C.restated(mixed))
    for c, g in zip(mixed[:6], got):
        _assert_equal([c], _host([c]), [g])


def test_another_R_and_no_thresholds():
    import pseg_amd
    rng = np.random.default_rng(3)
    g = C.random_scan(rng, (45, 61), 0.3)
    for R in (1.0, 64.0, 255.0):
        ink, T = pseg_amd.binarize_scans([g], pseg_amd.Sauvola(15, 0.34, R), host=True, thresholds=True)[0]
        rink, rT = C.sauvola(g, 15, 0.34, R)
        assert np.array_equal(ink, rink) and np.array_equal(T, rT)
        assert np.array_equal(pseg_amd.binarize_scans([g], pseg_amd.Sauvola(15, 0.34, R), host=True)[0], rink)
    assert pseg_amd.binarize_scans([], pseg_amd.Sauvola(15), host=True) == []


def test_special_images():
    cases = C.special_cases()
    want = C.restated(cases)
    got = _host(cases)
    _assert_equal(cases, got, want)
    for c, (ink, _) in zip(cases, got):
        if c[0].startswith("flat 0 "):
            assert ink.all(), c[0]                              # m = 0, T = 0, 0 <= 0
        elif c[0].startswith("flat"):
            assert not ink.any(), c[0]                          # s = 0: T = 0.8 m < m
    # radii larger than the image on both axes are among them
    assert any(c[2] // 2 > max(c[1].shape) for c in cases)


def test_refusals_leave_the_outputs_untouched():
    import pseg_amd
    C.refusals(pseg_amd.lib(), True)


def test_sauvola_window():
    import pseg_amd
    w = pseg_amd.sauvola_window
    assert [w(h) for h in (0.2, 1, 1.4, 7, 16, 16.5, 17.5, 30, 126, 127, 128, 4000)] == [3, 3, 3, 15, 33, 33, 37, 61, 253, 255, 255, 255]
    for bad in (None, 0, -3, float("nan"), float("inf")):
        with pytest.raises(pseg_amd.PsegError):
            w(bad)
    s = pseg_amd.Sauvola()
    assert (s.window, s.k, s.R) == (None, 0.2, 128.0)
    assert s.resolved(16) == pseg_amd.Sauvola(33) and pseg_amd.Sauvola(15, 0.3, 100).resolved(16) == pseg_amd.Sauvola(15, 0.3, 100)


def test_wrapper_argument_errors():
    import pseg_amd
    from pseg_amd import engine as E
    S, Err = pseg_amd.Sauvola, pseg_amd.PsegError
    for kw in (dict(window=14), dict(window=1), dict(window=257), dict(window=15.5), dict(window=True), dict(k=-0.1), dict(k=1.5), dict(R=0.0),
               dict(R=-2.0), dict(R=float("inf"))):
        with pytest.raises(Err):
            S(**kw)
    g = np.zeros((6, 5), np.uint8)
    with pytest.raises(Err, match="line height"):
        pseg_amd.binarize_scans([g], S(), host=True)                       # no window and nobody who knows the line height
    with pytest.raises(Err, match="one entry per scan"):
        pseg_amd.binarize_scans([g, g], [S(3)], host=True)
    with pytest.raises(Err, match="Sauvola"):
        pseg_amd.binarize_scans([g], ["sauvola"], host=True)
    with pytest.raises(Err, match="scan 1"):
        pseg_amd.binarize_scans([g, np.zeros((2, 3, 4), np.uint8)], S(3), host=True)
    with pytest.raises(Err, match="one entry per scan"):
        E.prepare_scans([g], [1.0], binarize=[S(3), S(3)])
    with pytest.raises(Err, match="line height"):
        E.prepare_scans([g], [1.0], binarize=S())
    # the front end refuses a bad entry before it looks for a device
    L = E.lib()
    table, keep, plans = E.scan_table([g], [1.0])
    out = [np.full(plans[0][:2], 0xA5, np.uint8) for _ in range(2)]
    P = ctypes.c_void_p * 1
    how = (E.BINARIZE * 1)(E.BINARIZE(8, 0.2, 128.0))
    assert L.pseg_prepare_scans_bin(0, 1, table, how, P(out[0].ctypes.data), P(out[1].ctypes.data), None) == -1
    assert b"scan 0" in L.pseg_last_error() and b"window" in L.pseg_last_error() and all((o == 0xA5).all() for o in out)


def test_loader_and_predictor_validate_binarize():
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    assert DatasetLoader(6, None).binarize is None
    s = pseg_amd.Sauvola()
    assert DatasetLoader(6, None, binarize=s).binarize is s
    for bad in ("sauvola", 15, (15, 0.2)):
        with pytest.raises(Exception, match="binarize"):
            DatasetLoader(6, None, binarize=bad)
        with pytest.raises(Exception, match="binarize"):
            next(Predictor.write_masks_scans(None, [], None, "nowhere", binarize=bad))      # refused before anything is touched


def test_an_unevenly_lit_page_needs_the_adaptive_threshold():
    """The point of the feature, on the restatement first: under light that falls off across the page the fixed threshold turns the
    dark side into ink, Sauvola at the default window does not.  Then the host entry equals the restatement."""
    import pseg_amd
    gray, glyph, line_height = C.uneven_page()
    assert gray.shape == (384, 512) and 0.05 < glyph.mean() < 0.3
    window = pseg_amd.sauvola_window(line_height)
    ink, T = C.sauvola(gray, window)
    assert (ink != glyph).mean() <= 0.005
    assert ((gray <= 127) != glyph).mean() >= 0.20
    got = pseg_amd.binarize_scans([gray], pseg_amd.Sauvola().resolved(line_height), host=True, thresholds=True)[0]
    assert np.array_equal(got[0], ink) and np.array_equal(got[1], T)
