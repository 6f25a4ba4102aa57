"""The deskewing without a GPU: the host twins (pseg_skew_maps_host, pseg_rotate_maps_host, pseg_deskew_scans_host), which walk the
contract's functions of csrc/pseg_skew.h in plain loops, against the NumPy restatement of tests/skew_cases.py -- indices, whole score
arrays and rotated bytes, array_equal throughout; the hand-made maps; the identity; every refusal; the accuracy on synthetic pages;
the arguments of the Python entries, the loader and the Predictor."""
import ctypes

import numpy as np
import pytest

import skew_cases as C


def _skew(cases, host=True, **kw):
    import pseg_amd
    return pseg_amd.skew_maps([c[1] for c in cases], [_how(c[2], c[3]) for c in cases], scores=True, host=host, **kw)


def _how(A, D):
    """A Skew with exactly these steps and denominator."""
    import pseg_amd
    s = pseg_amd.Skew(denom=D)
    s.steps = A
    return s


def _assert_skew(cases, idx, sc):
    assert idx.dtype == np.int32 and len(idx) == len(sc) == len(cases)
    for k, c in enumerate(cases):
        want_i, want_s = C.restated_skew(c[1], c[2], c[3])
        assert sc[k].dtype == np.uint64 and np.array_equal(sc[k], want_s), c[0]
        assert idx[k] == want_i, (c[0], idx[k], want_i)


def _rotate(cases, host=True):
    import pseg_amd
    outs = [None] * len(cases)
    groups = {}
    for k, c in enumerate(cases):                                      # one call per (denom, order, fill)
        groups.setdefault(c[3:], []).append(k)
    for (D, order, fill), ks in groups.items():
        for k, o in zip(ks, pseg_amd.rotate_maps([cases[k][1] for k in ks], [cases[k][2] for k in ks], denom=D, order=order, fill=fill, host=host)):
            outs[k] = o
    return outs


def test_symbols_geometry_and_structs():
    from pseg_amd import engine as E
    for sym in ("pseg_skew_maps", "pseg_skew_maps_host", "pseg_rotate_maps", "pseg_rotate_maps_host", "pseg_deskew_scans",
                "pseg_deskew_scans_host", "pseg_skew_geometry"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    assert E.skew_geometry() == (C.STRIP, 128, 16384)
    assert E.lib().pseg_skew_geometry(None, None, None) == 0
    assert ctypes.sizeof(E.SKEW) == 8 and ctypes.sizeof(E.ROTATE) == 16
    assert E.lib().pseg_abi_version() == 1


def test_skew_equals_the_restatement_over_the_grid():
    cases = C.skew_grid()
    assert len(cases) == len(C.SHAPES) * len(C.STEPS) * len(C.DENSITIES)
    assert any(((c[1] != 0) & (c[1] != 1)).any() for c in cases)       # bytes other than 1 occur as ink
    idx, sc = _skew(cases)
    _assert_skew(cases, idx, sc)
    assert len(set(int(i) for i in idx)) > 10                          # not a grid of one answer
    assert all(i == 0 for i, c in zip(idx, cases) if not c[1].any())   # a map without ink has index 0
    import pseg_amd
    assert np.array_equal(pseg_amd.skew_maps([c[1] for c in cases], [_how(c[2], c[3]) for c in cases], host=True), idx)   # without the scores
    for k in range(100, 110):                                          # one by one
        i1, s1 = _skew([cases[k]])
        assert i1[0] == idx[k] and np.array_equal(s1[0], sc[k])


def test_rotation_equals_the_restatement_over_the_grid():
    cases = C.rotate_grid()
    assert len(cases) == len(C.SHAPES) * len(C.STEPS) * len(C.ORDERS) * len(C.FILLS) * 5
    outs = _rotate(cases)
    differs = 0
    for c, o in zip(cases, outs):
        want = C.restated_rotate(*c[1:])
        assert o.dtype == np.uint8 and o.shape == c[1].shape and np.array_equal(o, want), (c[0], int((o != want).sum()))
        differs += not np.array_equal(o, c[1])
        if c[2] == 0:
            assert np.array_equal(o, c[1]), c[0]                        # index 0 is the identity, both orders, any fill
    assert differs > len(cases) // 3


def test_hand_made_maps():
    cases = C.hand_cases()
    idx, sc = _skew(cases)
    _assert_skew(cases, idx, sc)
    by = {c[0]: (int(idx[k]), sc[k], c) for k, c in enumerate(cases)}
    # ink in the first or last row only: the apron rows count, so no candidate loses a pixel -- and every profile of a full row
    # holds W pixels in all, whatever the offsets
    for name in ("ink only in the first row A=16", "ink only in the last row A=16"):
        i, s, c = by[name]
        assert i == 0 and s[16] == 100 * 100 and (s[[0, 32]] < s[16]).all() and (s > 0).all()
    i, s, c = by["ink only in the last, ragged strip"]
    assert i == 0 and len(set(s.tolist())) == 1                        # one strip holds all the ink: every candidate only moves it
    i, s, c = by["1 x 16384 of ink"]
    assert i == 0 and int(s[128]) == 1 << 28
    i, s, c = by["16384 x 512 of ink: a score of 2^32"]
    assert i == 0 and int(s[1]) == 1 << 32                             # needs the 64-bit sum
    i, s, c = by["a plateau of equal scores around 0"]
    assert i == 0 and (s[89 - 31:89 + 32] == s[89]).all() and s[89] == s.max() and s[0] < s[89]
    i, s, c = by["one strip: every score equal"]
    assert i == 0 and len(set(s.tolist())) == 1
    i, s, c = by["a tie between +a and -a only"]
    assert i > 0 and np.array_equal(s, s[::-1]) and s[16 + i] == s[16 - i] == s.max() and (s == s.max()).sum() == 2


def test_index_zero_is_the_identity_and_a_round_trip_comes_back():
    import pseg_amd
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (37, 53), (64, 64)):
        m = rng.integers(0, 256, shape).astype(np.uint8)
        for order in (0, 1):
            for fill in (0, 255):
                for D in (64, 1024, 4096):
                    assert np.array_equal(pseg_amd.rotate_maps([m], 0, denom=D, order=order, fill=fill, host=True)[0], m)
    # order 0 by +a then -a: the pixels well inside come back (a label map can be mapped to the scan's frame)
    lab = np.kron(rng.integers(0, 4, (10, 12)), np.ones((10, 10))).astype(np.uint8)
    back = pseg_amd.rotate_maps(pseg_amd.rotate_maps([lab], 40, host=True), -40, host=True)[0]
    inner = (slice(10, -10), slice(10, -10))
    assert (back[inner] == lab[inner]).mean() > 0.95


def test_deskew_is_the_estimate_followed_by_the_rotation():
    import pseg_amd
    rng = np.random.default_rng(8)
    scans = [rng.integers(0, 256, s).astype(np.uint8) for s in ((40, 70), (1, 1), (65, 33))]
    inks = [None, np.ones((1, 1), np.uint8), C.random_ink(rng, (65, 33), 0.1)]
    how = [_how(16, 64), _how(89, 1024), _how(128, 512)]
    for ks in (None, inks):
        outs, idx = pseg_amd.deskew_scans(scans, how, inks=ks, host=True)
        for k, g in enumerate(scans):
            ink = (g <= 127) if ks is None or ks[k] is None else ks[k]
            want_i = C.restated_skew(np.asarray(ink, np.uint8), how[k].steps, how[k].denom)[0]
            assert idx[k] == want_i
            assert np.array_equal(outs[k], C.restated_rotate(g, want_i, how[k].denom, 1, 255))


def test_refusals_leave_the_outputs_untouched():
    import pseg_amd
    C.refusals(pseg_amd.lib(), host=True)


def test_accuracy_on_synthetic_pages():
    """Planted skews on synthetic pages, D = 1024, A = 89 (one step is 0.056 degrees): the winner lies within 3 steps of the
    planted index -- the strip approximation leaves up to +-1.4 rows inside a strip at the largest slope --, and the corrected
    page measures 0.  36 cases; the restatement gave the same before the contract was fixed (worst: -70 -> -67, 88 -> 85)."""
    import pseg_amd
    from pseg_amd import synth
    how = pseg_amd.Skew(5.0, 1024)
    assert (how.steps, how.denom) == (89, 1024)
    planted = (-70, -23, 0, 5, 40, 88)
    scans, want = [], []
    for H, W in ((300, 420), (600, 450)):
        for i in range(3):
            scan = (255 - synth.synth_page(i, H, W)[0]).astype(np.uint8)
            for a0 in planted:
                scans.append(pseg_amd.rotate_maps([scan], -a0, denom=1024, order=1, fill=255, host=True)[0])
                want.append(a0)
    assert len(scans) == 36
    got = pseg_amd.skew_maps([s <= 127 for s in scans], how, host=True)
    print("planted -> found:", list(zip(want, got.tolist())))
    assert all(abs(int(g) - w) <= 3 for g, w in zip(got, want)), list(zip(want, got.tolist()))
    fixed, idx = pseg_amd.deskew_scans(scans, how, host=True)
    assert np.array_equal(idx, got)
    again = pseg_amd.skew_maps([s <= 127 for s in fixed], how, host=True)
    print("after the correction:", again.tolist())
    assert not again.any(), again.tolist()


def test_skew_and_wrapper_arguments():
    import pseg_amd
    from pseg_amd import PsegError, Skew
    assert (Skew().steps, Skew().denom) == (89, 1024)
    assert Skew(5.0, 64).steps == 5 and Skew(0.001, 64).steps == 1                # clamped below
    assert Skew(45, 64).steps == 16 and Skew(45, 4096).steps == 128 and Skew(10, 4096).steps == 128    # clamped above
    assert Skew(1.0, 4096).steps == int(np.floor(np.tan(np.radians(1.0)) * 4096)) == 71
    for bad in (63, 4097, 0, -1024, 1024.0, True, "1024", None):
        with pytest.raises(PsegError, match="denom"):
            Skew(5.0, bad)
    for bad in (0, -1, 90, 120, float("nan"), float("inf"), None, "5", True):
        with pytest.raises(PsegError, match="max_degrees"):
            Skew(bad)
    assert Skew() == Skew(5.0, 1024) and Skew() != Skew(4.0) and hash(Skew()) == hash(Skew(5.0)) and repr(Skew()) == "Skew(max_degrees=5.0, denom=1024)"
    assert pseg_amd.skew_degrees(0, 1024) == 0 and abs(pseg_amd.skew_degrees(1024, 1024) - 45) < 1e-12
    assert abs(pseg_amd.skew_degrees(-1, 1024) + 0.05595) < 1e-4
    m = np.zeros((4, 5), np.uint8)
    with pytest.raises(PsegError, match="one entry per map"):
        pseg_amd.skew_maps([m, m], [Skew()], host=True)
    with pytest.raises(PsegError, match="map 1"):
        pseg_amd.skew_maps([m, m], [Skew(), 5], host=True)
    with pytest.raises(PsegError, match="Skew"):
        pseg_amd.skew_maps([m], None, host=True)
    with pytest.raises(PsegError, match="map 0"):
        pseg_amd.skew_maps([np.zeros((2, 3, 4), np.uint8)], Skew(), host=True)
    with pytest.raises(PsegError, match="one index per map"):
        pseg_amd.rotate_maps([m, m], [1], host=True)
    for kw in ({"order": 2}, {"fill": 256}, {"fill": -1}, {"denom": 63}, {"denom": 4097}):
        with pytest.raises(PsegError, match="map 0"):
            pseg_amd.rotate_maps([m], 1, host=True, **kw)
    with pytest.raises(PsegError, match="map 1"):
        pseg_amd.rotate_maps([m, m], [0, 257], host=True)              # 4 * 257 > 1024
    with pytest.raises(PsegError, match="integer"):
        pseg_amd.rotate_maps([m], [1.5], host=True)
    with pytest.raises(PsegError, match="per scan"):
        pseg_amd.deskew_scans([m, m], Skew(), inks=[m], host=True)
    with pytest.raises(PsegError, match="scan 0"):
        pseg_amd.deskew_scans([m], Skew(), inks=[np.zeros((4, 6), np.uint8)], host=True)
    # empty lists; a bool map and a non-contiguous one
    assert len(pseg_amd.skew_maps([], Skew(), host=True)) == 0 and pseg_amd.rotate_maps([], [], host=True) == []
    outs, idx = pseg_amd.deskew_scans([], Skew(), host=True)
    assert outs == [] and idx.shape == (0,)
    idx, sc = pseg_amd.skew_maps([], Skew(), scores=True, host=True)
    assert sc == [] and idx.dtype == np.int32
    v = np.ones((6, 80), bool)[:, ::2]
    assert pseg_amd.skew_maps([v], Skew(), host=True)[0] == 0
    assert np.array_equal(pseg_amd.rotate_maps([v], 0, host=True)[0], v.astype(np.uint8))


def test_loader_and_predictor_validate_deskew():
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    ld = DatasetLoader(6, None)
    assert ld.deskew is None and ld.on_skew is None
    s = pseg_amd.Skew()
    cb = lambda *a: None
    ld = DatasetLoader(6, None, deskew=s, on_skew=cb)
    assert ld.deskew is s and ld.on_skew is cb
    for bad in ("deskew", 5.0, (89, 1024), True):
        with pytest.raises(Exception, match="deskew"):
            DatasetLoader(6, None, deskew=bad)
        with pytest.raises(Exception, match="deskew"):
            next(Predictor.write_masks_scans(None, [], None, "nowhere", deskew=bad))      # refused before anything is touched
    with pytest.raises(Exception, match="on_skew"):
        DatasetLoader(6, None, on_skew=cb)                                                 # goes with a deskew
    with pytest.raises(Exception, match="on_skew"):
        DatasetLoader(6, None, deskew=s, on_skew=3)
    with pytest.raises(Exception, match="on_skew"):
        next(Predictor.write_masks_scans(None, [], None, "nowhere", on_skew=cb))
