"""The polygons of the text regions on the device: pseg_text_regions_poly -- rg_trace_kernel walks every emitted row's boundary on the
region bit plane, a count pass, a scan, a write pass -- equals its host twin and the pixel walk of pseg_trace_regions_host,
array_equal throughout: the host test's grid, shapes around the 64-pixel word, the 128-row band and the 32 x 64 tile, hand-made maps
on which a word-run walk can go wrong, 70 mixed maps in two groups in every order, the capacity protocol, max_regions below a map's
count and the refusals."""
import numpy as np
import pytest

import regions_cases as C
import regions_poly_util as U
import test_regions_poly_host as HT

pytestmark = pytest.mark.gpu

_TWIN = {}


def _dev(cases, **kw):
    import pseg_amd
    return pseg_amd.text_regions([c[1] for c in cases], U.how_of(cases), polygons=True, **kw)


def _twin(cases, key):
    """The host twin's records of a case list, computed once."""
    if key not in _TWIN:
        import pseg_amd
        _TWIN[key] = pseg_amd.text_regions([c[1] for c in cases], U.how_of(cases), host=True, polygons=True)
    return _TWIN[key]


def test_device_equals_the_host_twin_over_the_grid(gpu):
    cases = C.grid_cases()
    dev = _dev(cases)
    U.assert_records_equal(cases, dev, _twin(cases, "grid"))
    U.assert_records_equal(cases, dev, U.yardstick(cases, "grid"))
    assert sum(len(r["polygons"]) for r in dev) > 500


def _geometry_cases():
    from pseg_amd import engine as E
    word, band, band_words, th, tw, slots = E.regions_geometry()
    assert (word, band, th, tw) == (64, 128, 32, 64)
    shapes = [(h + d, w + e) for h in (th, band) for d in (-1, 0, 1) for w in (word,) for e in (-1, 0, 1)]
    assert set(C.SHAPES) & set(shapes) == {(31, 63), (32, 64), (33, 65)}      # the shapes of the grid around the tile, and the band's
    return C.grid_cases(seed=31, shapes=shapes, triples=[(1, 1, 1), (3, 1, 2), C.region_kernels(7)], densities=C.DENSITIES)


def test_shapes_around_the_word_the_band_and_the_tile(gpu):
    cases = _geometry_cases()
    assert len(cases) == 18 * 9
    dev = _dev(cases)
    U.assert_records_equal(cases, dev, _twin(cases, "geometry"))
    assert sum(len(r["polygons"]) for r in dev) > 100


def test_hand_made_maps_equal_the_pixel_walk(gpu):
    cases = [c[:4] for c in C.hand_cases()] + U.word_cases()
    want = U.yardstick(cases, "hand+word")
    U.assert_records_equal(cases, _dev(cases), want)
    U.assert_records_equal(cases, _dev(cases, masks=False), want, masks=False)


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(78)
    shapes = [(int(rng.integers(1, 140)), int(rng.integers(1, 300))) for _ in range(70)]
    cases = []
    for k, (H, W) in enumerate(shapes):
        ks = C.TRIPLES[k % len(C.TRIPLES)]
        t = int(rng.integers(0, 4))
        cases.append(("poly mixed %d %dx%d k=%r" % (k, H, W, ks), C.blob_map(rng, H, W, (0.2, 0.45, 0.7)[k % 3], t, 1.0 + 0.1 * min(ks[0], 40)), t, ks))
    return cases


def test_seventy_maps_in_two_groups(gpu, mixed):
    import pseg_amd
    want = _twin(mixed, "mixed")
    assert sum(len(r["polygons"]) for r in want) > 70
    first = _dev(mixed)
    U.assert_records_equal(mixed, first, want)
    U.assert_records_equal(mixed, _dev(mixed), want)                    # twice
    order = np.random.default_rng(6).permutation(len(mixed))
    U.assert_records_equal([mixed[i] for i in order], _dev([mixed[i] for i in order]), [want[i] for i in order])
    for k in range(len(mixed)):                                         # each alone
        U.assert_records_equal([mixed[k]], _dev([mixed[k]], masks=False), [want[k]], masks=False)
    pseg_amd.lib().pseg_release_workspace(0)
    U.assert_records_equal(mixed, _dev(mixed), want)                    # after a workspace release
    U.assert_records_equal(mixed, _dev(mixed, max_regions=2, masks=False), want, masks=False)   # crowded maps run again alone


def test_capacity_protocol(gpu):
    HT.check_capacity_protocol(0)


def test_max_regions_below_the_count(gpu):
    HT.check_max_regions_overflow(0)


def test_refusals_leave_the_outputs_untouched(gpu):
    HT.check_refusals(0)


def test_plain_entry_is_unchanged_by_the_polygon_call(gpu, mixed):
    """pseg_text_regions after pseg_text_regions_poly on the same workspace: the same masks and tables."""
    import pseg_amd
    maps, hows = [c[1] for c in mixed[:9]], U.how_of(mixed[:9])
    plain = pseg_amd.text_regions(maps, hows)
    poly = _dev(mixed[:9])
    again = pseg_amd.text_regions(maps, hows)
    for a, b, c in zip(plain, poly, again):
        for k in ("mask", "boxes", "areas", "seeds"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
        assert "polygons" not in a and "polygons" not in c
