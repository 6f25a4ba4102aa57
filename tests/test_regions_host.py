"""The text regions without a GPU: pseg_text_regions_host -- the planes' word arithmetic shared with the kernels, a plain y pass and a
two-pass union-find over the page -- against the NumPy / SciPy restatement of tests/regions_cases.py, masks and tables, array_equal
throughout; the hand-made maps; counts above max_regions; every refusal; region_kernels; the wrappers' arguments; and the crack
polygons of every region of the grid (area, even-odd of the pixel centres, box, start corner, the cap protocol).

The polygon is a region's outer boundary.  T = m3 | fill(rt), as the contract fixes it, can have islands (pixels of m3 that a shifted
close lost can ring a hole that fill(rt) never saw: 15 of 194 maps of a grid here have some), so what a polygon encloses is checked
exactly against the region with its islands closed, and for every region without an island -- nearly all of them -- that is the region
itself and the shoelace area is the table's area."""
import ctypes

import numpy as np
import pytest

import regions_cases as C


def _host(cases, **kw):
    import pseg_amd
    return pseg_amd.text_regions([c[1] for c in cases], [pseg_amd.TextRegions(c[2], kernels=c[3]) for c in cases], host=True, **kw)


def _rows(rec):
    r = rec["boxes"].shape[0]
    rows = np.zeros((r, 8), np.int32)
    rows[:, 0:4], rows[:, 4], rows[:, 5:7] = rec["boxes"], rec["areas"], rec["seeds"]
    return rows


def assert_equal(cases, recs, masks=True):
    assert len(recs) == len(cases)
    for c, rec in zip(cases, recs):
        want_mask, want_rows = C.restated(c[1], c[2], *c[3], key=c[0])
        if masks:
            assert rec["mask"].dtype == np.uint8 and rec["mask"].shape == c[1].shape, c[0]
            assert np.array_equal(rec["mask"], want_mask), (c[0], int((rec["mask"] != want_mask).sum()))
        else:
            assert rec["mask"] is None
        assert rec["boxes"].dtype == np.int32 and rec["areas"].dtype == np.int32 and rec["seeds"].dtype == np.int32
        assert np.array_equal(_rows(rec), want_rows), (c[0], _rows(rec)[:4], want_rows[:4])


def test_symbols_and_geometry():
    from pseg_amd import engine as E
    for sym in ("pseg_text_regions", "pseg_text_regions_host", "pseg_regions_geometry", "pseg_trace_regions_host"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    word, band, band_words, th, tw, slots = E.regions_geometry()
    assert word == 64 and band >= 1 and band_words >= 1 and tw == word and th >= 1 and 2 * (th + tw) - 4 <= slots <= 255
    assert ctypes.sizeof(E.REGIONS) == 16


def test_region_kernels():
    import pseg_amd
    assert pseg_amd.region_kernels(30) == (30, 10, 27)
    assert pseg_amd.region_kernels(12) == (12, 4, 10) and pseg_amd.region_kernels(11) == (11, 3, 10)
    assert pseg_amd.region_kernels(7.9) == (7, 2, 7)
    assert pseg_amd.region_kernels(2) == (2, 1, 1) and pseg_amd.region_kernels(0) == (1, 1, 1)
    assert pseg_amd.region_kernels(1000) == (255, 255, 255)
    for c in (7, 11, 12, 23, 40):
        assert pseg_amd.region_kernels(c) == C.region_kernels(c)
        assert pseg_amd.TextRegions(1, char_height=c).kernels == C.region_kernels(c)
    for bad in (None, -1, float("nan"), float("inf"), True):
        with pytest.raises(pseg_amd.PsegError):
            pseg_amd.region_kernels(bad)


def test_the_restatement_on_a_case_worked_by_hand():
    # 1 x 8, a single pixel at x = 3.  k = 2 (anchor 1): out[x] = m[x - 1] | m[x], so dil sets x in {3, 4}: shifted, not centred
    m = np.zeros((1, 8), bool)
    m[0, 3] = True
    assert list(np.flatnonzero(C.dil(m, 2)[0])) == [3, 4]
    assert list(np.flatnonzero(C.ero(C.dil(m, 2), 2)[0])) == [4]             # the even close moves the pixel: not extensive
    assert list(np.flatnonzero(C.dil(m, 3)[0])) == [2, 3, 4]
    full = np.ones((1, 8), bool)
    assert C.ero(full, 5).all()                    # outside counts as set for the erosion
    e = np.ones((1, 8), bool)
    e[0, 0] = False
    assert list(np.flatnonzero(~C.ero(e, 3)[0])) == [0, 1]   # offsets -1..1: x = 0 and x = 1 see the gap
    assert list(np.flatnonzero(~C.ero(e, 2)[0])) == [0, 1]   # offsets -1..0: x = 0 and x = 1


def test_host_entry_equals_the_restatement_over_the_grid():
    cases = C.grid_cases()
    assert len(cases) == len(C.SHAPES) * len(C.TRIPLES) * len(C.DENSITIES)
    recs = _host(cases)
    assert_equal(cases, recs)
    # not a grid of trivial results
    assert sum(len(r["areas"]) > 0 for r in recs) > len(cases) // 2
    assert sum(len(r["areas"]) > 1 for r in recs) > len(cases) // 10
    assert sum(0 < int(r["mask"].sum()) < r["mask"].size for r in recs) > len(cases) // 3
    # without masks, and entries one by one
    assert_equal(cases[::7], _host(cases[::7], masks=False), masks=False)
    for k in range(100, 110):
        assert_equal([cases[k]], _host([cases[k]]))


def test_the_shifted_close_loses_pixels_somewhere_in_the_grid():
    # why T keeps the `m3 |` term: with even sides rt does not contain m3 everywhere
    lost = 0
    for c in C.grid_cases(seed=12, shapes=[(63, 127), (100, 200)]):
        m3, rt = C.stages(c[1], c[2], *c[3])
        lost += bool((m3 & ~rt).any())
    assert lost > 0


def test_hand_made_maps():
    cases = C.hand_cases()
    recs = _host(cases)
    assert_equal(cases, recs)
    by = {}
    for c, rec in zip(cases, recs):
        by[c[0]] = rec
        if c[4] is not None:
            assert len(rec["areas"]) == c[4], (c[0], len(rec["areas"]))
    assert by["all label"]["mask"].all() and not by["none"]["mask"].any()
    assert by["ring over a tile corner"]["areas"][0] == 30 * 60 and by["ring at the map's edge"]["areas"][0] == 40 * 80
    assert by["notch to the edge"]["areas"][0] == 50 * 100 - 5 * 70
    assert by["diagonal pocket"]["areas"][0] == 20 * 30 - 1
    assert by["larger than a tile"]["areas"][0] == 105 * 283
    assert list(by["diagonal neighbours"]["seeds"][1]) == [20, 20]


def test_count_above_max_regions():
    import pseg_amd
    from pseg_amd import engine as E
    name, m, t, ks, want = [c for c in C.hand_cases() if c[0] == "dots"][0]
    full = pseg_amd.text_regions([m], pseg_amd.TextRegions(t, kernels=ks), host=True, max_regions=8)[0]   # the wrapper runs it again alone
    assert len(full["areas"]) == want and np.array_equal(_rows(full), C.restated(m, t, *ks)[1])
    # the C entry: the true count, the rows untouched
    rows = np.full((2, 8, 8), -5, np.int32)
    cnt = np.full(2, -5, np.int32)
    small = np.zeros((4, 4), np.uint8)
    small[1, 1] = 1
    maps = [m, small]
    how = (E.REGIONS * 2)(E.REGIONS(t, 1, 1, 1), E.REGIONS(1, 1, 1, 1))
    P, I = ctypes.c_void_p * 2, ctypes.c_int * 2
    rc = E.lib().pseg_text_regions_host(2, P(*[a.ctypes.data for a in maps]), I(66, 4), I(130, 4), how, None, 8, rows.ctypes.data, cnt.ctypes.data)
    assert rc == 0 and list(cnt) == [want, 1]
    assert (rows[0] == -5).all() and list(rows[1, 0]) == [1, 1, 2, 2, 1, 1, 1, 0] and (rows[1, 1:] == -5).all()
    # no table at all: only counts
    cnt[:] = -5
    rc = E.lib().pseg_text_regions_host(2, P(*[a.ctypes.data for a in maps]), I(66, 4), I(130, 4), how, None, 0, None, cnt.ctypes.data)
    assert rc == 0 and list(cnt) == [want, 1]


def _refusals(call):
    """call(n, maps, H, W, how, masks, max_regions, rows, cnt) -> rc; every refusal leaves the outputs as they were."""
    from pseg_amd import engine as E
    rng = np.random.default_rng(3)
    maps = [C.blob_map(rng, 20, 30, 0.4, 1) for _ in range(4)]
    masks = [np.full((20, 30), 0xA5, np.uint8) for _ in range(4)]
    rows = np.full((4, 4, 8), -5, np.int32)
    cnt = np.full(4, -5, np.int32)
    P, I = ctypes.c_void_p * 4, ctypes.c_int * 4

    def run(H=(20,) * 4, W=(30,) * 4, sides=((3, 1, 2),) * 4, label=1, null_map=None, max_regions=4, table=True, n=4):
        how = (E.REGIONS * 4)(*[E.REGIONS(label, *s) for s in sides])
        ptrs = [a.ctypes.data for a in maps]
        if null_map is not None:
            ptrs[null_map] = None
        rc = call(n, P(*ptrs), I(*H), I(*W), how, P(*[a.ctypes.data for a in masks]), max_regions, rows.ctypes.data if table else None, cnt.ctypes.data)
        return rc, E.lib().pseg_last_error().decode()

    def untouched():
        return all((a == 0xA5).all() for a in masks) and (rows == -5).all() and (cnt == -5).all()
    for k_bad in (0, 256, -3):
        for pos in range(3):
            s = [3, 1, 2]
            s[pos] = k_bad
            rc, msg = run(sides=((3, 1, 2), (3, 1, 2), (3, 1, 2), tuple(s)))
            assert rc != 0 and msg.startswith("map 3:") and untouched(), (k_bad, pos, rc, msg)
    rc, msg = run(null_map=2)
    assert rc != 0 and msg.startswith("map 2:") and untouched()
    rc, msg = run(H=(20, 0, 20, 20))
    assert rc != 0 and msg.startswith("map 1:") and untouched()
    rc, msg = run(W=(30, 30, -1, 30))
    assert rc != 0 and msg.startswith("map 2:") and untouched()
    rc_inval = rc
    rc, msg = run(H=(20, 20, 20, 1 << 16), W=(30, 30, 30, 1 << 15))      # 2^31 pixels: refused before a byte is read
    assert rc != 0 and rc != rc_inval and msg.startswith("map 3:") and untouched()
    rc, msg = run(label=256)
    assert rc == rc_inval and untouched()
    rc, msg = run(table=False)
    assert rc == rc_inval and untouched()
    rc, msg = run(max_regions=-1)
    assert rc == rc_inval and untouched()
    rc, msg = run(n=-1)
    assert rc == rc_inval and untouched()
    rc, msg = run(n=0)                             # nothing to do: OK, nothing touched
    assert rc == 0 and untouched()
    rc, msg = run()
    assert rc == 0 and not untouched()


def test_refusals_leave_the_outputs_untouched():
    from pseg_amd import engine as E
    _refusals(lambda *a: E.lib().pseg_text_regions_host(*a))


def test_wrapper_argument_errors():
    import pseg_amd
    m = np.zeros((5, 5), np.uint8)
    ok = pseg_amd.TextRegions(1, kernels=(1, 1, 1))
    for kw in (dict(label=-1, kernels=(1, 1, 1)), dict(label=256, kernels=(1, 1, 1)), dict(label=1.5, kernels=(1, 1, 1)), dict(label=True, kernels=(1, 1, 1)),
               dict(label=1), dict(label=1, char_height=10, kernels=(1, 1, 1)), dict(label=1, kernels=(1, 1)), dict(label=1, kernels=(0, 1, 1)),
               dict(label=1, kernels=(1, 256, 1)), dict(label=1, kernels=(1, 1, 2.5)), dict(label=1, char_height=-2)):
        with pytest.raises(pseg_amd.PsegError):
            pseg_amd.TextRegions(**kw)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.text_regions([m, m], [ok], host=True)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.text_regions([m], [None], host=True)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.text_regions([np.zeros((2, 2, 3), np.uint8)], ok, host=True)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.text_regions([m], ok, host=True, max_regions=-1)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.trace_regions(np.zeros((2, 2, 2), np.uint8), {"seeds": np.zeros((0, 2), np.int32)})
    with pytest.raises(pseg_amd.PsegError):        # a seed that is no region's first pixel
        pseg_amd.trace_regions(m, {"seeds": np.array([[1, 1]], np.int32)})
    assert pseg_amd.text_regions([], ok, host=True) == []
    assert pseg_amd.TextRegions(1, char_height=30) == pseg_amd.TextRegions(1, kernels=(30, 10, 27))
    assert pseg_amd.trace_regions(m, {"seeds": np.zeros((0, 2), np.int32)}) == []


def check_polygons(mask, rec, polys):
    """The exact properties of the crack polygons of one record -> the number of regions with a white island.  The polygon is the
    region's OUTER boundary, so what it encloses is the region with its islands closed (`whole`); for a region without an island that
    is the region itself, and the shoelace area is the table's area."""
    from scipy import ndimage
    H, W = mask.shape
    assert len(polys) == len(rec["areas"])
    cc, _ = ndimage.label(mask)
    islands = 0
    for i, poly in enumerate(polys):
        assert poly.dtype == np.int32 and poly.ndim == 2 and poly.shape[1] == 2 and poly.shape[0] >= 4 and poly.shape[0] % 2 == 0
        sy, sx = rec["seeds"][i]
        region = cc == cc[sy, sx]
        assert int(region.sum()) == rec["areas"][i]
        whole = ndimage.binary_fill_holes(region, structure=np.ones((3, 3), bool))   # (an island is 8-connected background: the walk keeps diagonal pixels apart)
        if int(whole.sum()) == rec["areas"][i]:
            assert C.shoelace(poly) == rec["areas"][i]
        else:
            islands += 1
        assert C.shoelace(poly) == int(whole.sum())
        assert np.array_equal(C.even_odd(poly, H, W), whole)
        x0, y0, x1, y1 = rec["boxes"][i]
        assert (poly[:, 0].min(), poly[:, 1].min(), poly[:, 0].max(), poly[:, 1].max()) == (x0, y0, x1, y1)
        assert (poly[0, 1], poly[0, 0]) == (sy, sx)                     # the seed's top-left corner
        assert tuple(poly[1]) == (sx + int(np.argmin(np.append(mask[sy, sx:], 0))), sy)   # clockwise: east along the seed's run first
        d = np.roll(poly, -1, axis=0) - poly
        assert ((d[:, 0] == 0) != (d[:, 1] == 0)).all()                 # axis-parallel edges of non-zero length
        d2 = np.roll(d, -1, axis=0)
        assert ((d[:, 0] == 0) != (d2[:, 0] == 0)).all()                # only direction changes are kept
    return islands


def test_polygons_of_every_region_of_the_grid():
    import pseg_amd
    cases = C.grid_cases(seed=13, shapes=[(1, 70), (70, 1), (33, 65), (65, 129), (200, 333)]) + [c[:4] for c in C.hand_cases()]
    recs = _host(cases)
    total = islands = 0
    for c, rec in zip(cases, recs):
        polys = pseg_amd.trace_regions(rec["mask"], rec)
        islands += check_polygons(rec["mask"], rec, polys)
        total += len(polys)
    assert total > 300 and islands < total // 10   # nearly every region is its polygon's inside exactly


def test_small_polygons_and_the_cap_protocol():
    import pseg_amd
    from pseg_amd import engine as E
    m = np.zeros((12, 12), np.uint8)
    m[1, 1] = 1                                    # one pixel: 4 vertices
    m[3:8, 3] = 1                                  # a one-pixel-wide L
    m[7, 3:7] = 1
    for i in range(4):                             # a diagonal staircase of pixels that touch only diagonally: four regions
        m[8 + i, 8 + i] = 1
    m[3, 8:10] = 1                                 # a 4-connected staircase
    m[4, 9:11] = 1
    m[5, 10:12] = 1
    rec = pseg_amd.text_regions([m], pseg_amd.TextRegions(1, kernels=(1, 1, 1)), host=True)[0]
    assert len(rec["areas"]) == 1 + 1 + 1 + 4
    polys = pseg_amd.trace_regions(rec["mask"], rec)
    assert check_polygons(rec["mask"], rec, polys) == 0
    assert [tuple(v) for v in polys[0]] == [(1, 1), (2, 1), (2, 2), (1, 2)]
    by_seed = {tuple(s): p for s, p in zip(rec["seeds"], polys)}
    assert [tuple(v) for v in by_seed[(3, 3)]] == [(3, 3), (4, 3), (4, 7), (7, 7), (7, 8), (3, 8)]
    assert len(by_seed[(3, 8)]) == 12
    for i in range(4):
        assert len(by_seed[(8 + i, 8 + i)]) == 4
    # the cap protocol of the C entry
    r = len(polys)
    need = sum(len(p) for p in polys)
    table = np.zeros((r, 8), np.int32)
    table[:, 5:7] = rec["seeds"]
    first = np.full(r + 1, -9, np.int64)
    xy = np.full((need, 2), -9, np.int32)
    rc = E.lib().pseg_trace_regions_host(m.ctypes.data, 12, 12, r, table.ctypes.data, xy.ctypes.data, need - 1, first.ctypes.data)
    assert rc == 0 and first[r] == need and (first[:r] == -9).all() and (xy == -9).all()
    rc = E.lib().pseg_trace_regions_host(m.ctypes.data, 12, 12, r, table.ctypes.data, None, 0, first.ctypes.data)
    assert rc == 0 and first[r] == need
    rc = E.lib().pseg_trace_regions_host(m.ctypes.data, 12, 12, r, table.ctypes.data, xy.ctypes.data, need, first.ctypes.data)
    assert rc == 0 and first[0] == 0 and first[r] == need and np.array_equal(np.diff(first), [len(p) for p in polys])
    assert np.array_equal(xy, np.concatenate(polys))
