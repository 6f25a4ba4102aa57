"""The polygons of the text regions without a GPU: pseg_text_regions_poly_host -- the host entry, then the walk over bit planes that the
device tracer shares (csrc/pseg_regions.h: rg_hrun takes a horizontal stretch a word at a time) -- against pseg_text_regions_host +
pseg_trace_regions_host, the independent walk that goes pixel by pixel over a byte mask.  Everything is integer: array_equal
throughout.  The grid and the hand-made maps of tests/regions_cases.py, the word-run maps of tests/regions_poly_util.py, the capacity
protocol, max_regions below a map's count, every refusal, and regions_of_record from a record without a mask."""
import numpy as np
import pytest

import regions_cases as C
import regions_poly_util as U


def _hand():
    return [c[:4] for c in C.hand_cases()]


def _twin(cases, **kw):
    import pseg_amd
    return pseg_amd.text_regions([c[1] for c in cases], U.how_of(cases), host=True, polygons=True, **kw)


def test_symbols():
    from pseg_amd import engine as E
    for sym in ("pseg_text_regions_poly", "pseg_text_regions_poly_host"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)


def test_grid_equals_the_pixel_walk():
    cases = C.grid_cases()
    U.assert_records_equal(cases, _twin(cases), U.yardstick(cases, "grid"))


def test_hand_and_word_cases_equal_the_pixel_walk():
    cases = _hand() + U.word_cases()
    want = U.yardstick(cases, "hand+word")
    U.assert_records_equal(cases, _twin(cases), want)
    U.assert_records_equal(cases, _twin(cases, masks=False), want, masks=False)
    for c, w, n in zip(cases, want, [h[4] for h in C.hand_cases()]):
        if n is not None:
            assert len(w["polygons"]) == n, c[0]


def test_the_comparison_is_not_empty():
    """What the cases must contain for the equality above to say something about a word-run walk."""
    cases = C.grid_cases() + _hand()
    recs = _twin(cases)                            # the word-run walk's own polygons: what the tests above compare
    wide = tall = island = single = 0
    edges = [0, 0, 0, 0]
    for c, rec in zip(cases, recs):
        H, W = c[1].shape
        for b, a, p in zip(rec["boxes"], rec["areas"], rec["polygons"]):
            wide += b[2] - b[0] > 64
            tall += b[3] - b[1] > 32
            single += a == 1
            island += C.shoelace(p) > a            # the outer boundary encloses more than the region: background inside it
            for e, hit in enumerate((b[0] == 0, b[1] == 0, b[2] == W, b[3] == H)):
                edges[e] += bool(hit)
            assert len(p) >= 4 and len(p) % 2 == 0
    assert wide > 0 and tall > 0 and island > 0 and single > 0 and all(e > 0 for e in edges), (wide, tall, island, single, edges)


def _small_list():
    cases = [c for c in _hand() if c[0] in ("diagonal neighbours", "label id 255", "ring over a tile corner", "none")] + \
            [c for c in U.word_cases() if c[0] in ("comb", "staircase left")]
    return cases, U.yardstick(_hand() + U.word_cases(), "hand+word")


def _want_of(cases):
    allc = _hand() + U.word_cases()
    recs = U.yardstick(allc, "hand+word")
    names = [c[0] for c in allc]
    return [recs[names.index(c[0])] for c in cases]


def check_capacity_protocol(device):
    """cap = 0, needed - 1 and needed, on the host twin (device None) or the device entry."""
    cases, _ = _small_list()
    want = _want_of(cases)
    maps, hows, n, R = [c[1] for c in cases], U.how_of(cases), len(cases), 8
    need = sum(len(p) for w in want for p in w["polygons"])
    assert need > 40
    for cap in (0, need - 1):
        out = U.raw(maps, hows, R, cap, device=device)
        assert out["rc"] == 0, out["msg"]
        assert out["first"][n - 1, R] == need
        assert (out["first"].ravel()[:-1] == U.SENTINEL).all() and (out["xy"] == U.SENTINEL).all()   # no vertex, no other offset
        assert (out["status"] == 0).all()
        for k, w in enumerate(want):               # tables and counts stay valid
            r = len(w["boxes"])
            assert out["cnt"][k] == r and np.array_equal(out["rows"][k, :r, 0:4], w["boxes"]) and np.array_equal(out["rows"][k, :r, 5:7], w["seeds"])
    out = U.raw(maps, hows, R, need, device=device)
    assert out["rc"] == 0 and out["first"][n - 1, R] == need and out["first"][0, 0] == 0 and (out["status"] == 0).all()
    assert (out["xy"] != U.SENTINEL).all()
    for k, w in enumerate(want):
        r = len(w["boxes"])
        assert k == 0 or out["first"][k, 0] == out["first"][k - 1, R]
        assert (out["first"][k, r:] == out["first"][k, r]).all()
        for j, p in enumerate(w["polygons"]):
            assert np.array_equal(out["xy"][out["first"][k, j]:out["first"][k, j + 1]], p), (cases[k][0], j)


def check_max_regions_overflow(device):
    """max_regions below one map's count: that map's status says so and it has no polygons; the other maps are complete."""
    from pseg_amd import engine as E
    cases, _ = _small_list()
    want = _want_of(cases)
    maps, hows, n, R = [c[1] for c in cases], U.how_of(cases), len(cases), 1
    assert sorted(len(w["boxes"]) for w in want) == [0, 1, 1, 1, 2, 2]
    out = U.raw(maps, hows, R, 4096, device=device)
    assert out["rc"] == 0, out["msg"]
    run = 0
    for k, w in enumerate(want):
        r = len(w["boxes"])
        assert out["cnt"][k] == r
        assert out["first"][k, 0] == run
        if r > R:
            assert out["status"][k] == E.PSEG_EUNSUPPORTED and (out["first"][k] == run).all() and (out["rows"][k] == U.SENTINEL).all()
            continue
        assert out["status"][k] == 0
        for j, p in enumerate(w["polygons"]):
            assert np.array_equal(out["xy"][out["first"][k, j]:out["first"][k, j + 1]], p), (cases[k][0], j)
        run = out["first"][k, R]
    assert (out["xy"][run:] == U.SENTINEL).all()
    # no table at all: a map with a region is over, a map without one is complete
    out = U.raw(maps, hows, 0, 16, device=device)
    assert out["rc"] == 0 and (out["first"] == 0).all() and (out["xy"] == U.SENTINEL).all()
    assert [int(s) for s in out["status"]] == [0 if len(w["boxes"]) == 0 else E.PSEG_EUNSUPPORTED for w in want]


def check_refusals(device):
    cases, _ = _small_list()
    maps, hows = [c[1] for c in cases], U.how_of(cases)
    import pseg_amd
    bad = []
    for kw in (dict(drop=("first",)), dict(drop=("status",)), dict(drop=("xy",))):
        bad.append(U.raw(maps, hows, 8, 64, device=device, masks=True, **kw))
    bad.append(U.raw(maps, hows, 8, -1, device=device, masks=True))
    bad.append(U.raw(maps, hows, -1, 64, device=device, masks=True))
    bad.append(U.raw(maps, hows[:-1] + [pseg_amd.TextRegions(1, kernels=(1, 1, 1))], 8, 64, device=device, masks=True))   # (a sound list: the control)
    for out in bad[:-1]:
        assert out["rc"] == -1 and out["msg"] and U.untouched(out), (out["rc"], out["msg"])
    assert bad[-1]["rc"] == 0 and not U.untouched(bad[-1])
    # pseg_text_regions' own refusals, through this entry: a side of 0, a NULL map is covered by its own tests; here a side and a shape
    from pseg_amd import engine as E
    how_bad = list(hows)
    how_bad[2] = type("H", (), {"label": 1, "kernels": (3, 0, 2)})()
    out = U.raw(maps, how_bad, 8, 64, device=device, masks=True)
    assert out["rc"] == -1 and out["msg"].startswith("map 2:") and U.untouched(out)
    out = U.raw(maps[:2] + [np.zeros((1 << 16, 0), np.uint8)], hows[:3], 8, 64, device=device)
    assert out["rc"] == -1 and out["msg"].startswith("map 2:") and U.untouched(out)
    assert E.lib().pseg_text_regions_poly_host(0, None, None, None, None, None, 0, None, None, None, 0, None, None) == 0   # nothing to do


def test_capacity_protocol():
    check_capacity_protocol(None)


def test_max_regions_below_the_count():
    check_max_regions_overflow(None)


def test_refusals_leave_the_outputs_untouched():
    check_refusals(None)


def test_wrapper_reruns_a_map_with_more_regions_and_grows_the_capacity():
    import pseg_amd
    dots = [c for c in _hand() if c[0] == "dots"]
    rec = pseg_amd.text_regions([dots[0][1]], U.how_of(dots), host=True, polygons=True, masks=False, max_regions=4)[0]
    assert rec["mask"] is None and len(rec["polygons"]) == 33 * 65
    for (y, x), p in zip(rec["seeds"], rec["polygons"]):
        assert np.array_equal(p, [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1]])


def test_regions_of_record_without_a_mask():
    import pseg_amd
    from ocr4all_pixel_classifier.lib.pc_segmentation import regions_of_record
    cases = [c for c in _hand() if c[0] in ("two lines", "label id 255")]
    with_mask = pseg_amd.text_regions([c[1] for c in cases], U.how_of(cases), host=True)
    no_mask = pseg_amd.text_regions([c[1] for c in cases], U.how_of(cases), host=True, polygons=True, masks=False)
    for a, b in zip(with_mask, no_mask):
        ra, rb = regions_of_record(a), regions_of_record(b)
        assert b["mask"] is None and len(ra) == len(rb) > 0
        for p, q in zip(ra, rb):
            assert np.array_equal(p.polygon, q.polygon) and p.box == q.box and p.area == q.area and p.seed == q.seed
