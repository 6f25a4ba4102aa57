"""The text regions on the device: pseg_text_regions (bit-plane morphology, the closed / open tile scheme twice) = the host entry = the
NumPy / SciPy restatement of tests/regions_cases.py, array_equal throughout: the host test's grid and hand-made maps, shapes around
every constant of pseg_regions_geometry, a list of 70 maps in two groups in every order and mode, one large page, the refusals, and
the mirror package's get_text_regions / Predictor.predict_regions against predict + the host entry."""
import numpy as np
import pytest

import regions_cases as C
from test_regions_host import _refusals, _rows, assert_equal, check_polygons

pytestmark = pytest.mark.gpu


def _how(cases):
    import pseg_amd
    return [pseg_amd.TextRegions(c[2], kernels=c[3]) for c in cases]


def _dev(cases, **kw):
    import pseg_amd
    return pseg_amd.text_regions([c[1] for c in cases], _how(cases), **kw)


def _same(a, b, masks=True):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if masks:
            assert np.array_equal(x["mask"], y["mask"]), k
        assert np.array_equal(_rows(x), _rows(y)), k


def test_device_equals_host_equals_restatement_over_the_grid(gpu):
    cases = C.grid_cases() + [c[:4] for c in C.hand_cases()]
    dev = _dev(cases, max_regions=64)              # (the dots and other crowded maps run again alone)
    assert_equal(cases, dev)
    _same(dev, _dev(cases, host=True))


def _geometry_cases():
    from pseg_amd import engine as E
    word, band, band_words, th, tw, slots = E.regions_geometry()
    rows = sorted({v + d for v in (th, band) for d in (-1, 0, 1)})
    cols = sorted({v + d for v in (word, tw, word * band_words) for d in (-1, 0, 1)})
    return C.grid_cases(seed=23, shapes=[(h, w) for h in rows for w in cols], triples=[(3, 1, 2), C.region_kernels(23)], densities=[0.4])


def test_shapes_around_every_constant(gpu):
    cases = _geometry_cases()
    assert len(cases) >= 6 * 6 * 2                 # three values around each of two row constants and at least two column constants
    assert_equal(cases, _dev(cases))


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(77)
    shapes = [(int(rng.integers(1, 140)), int(rng.integers(1, 300))) for _ in range(70)]
    cases = []
    for k, (H, W) in enumerate(shapes):
        ks = C.TRIPLES[k % len(C.TRIPLES)]
        t = int(rng.integers(0, 4))
        cases.append(("mixed %d %dx%d k=%r" % (k, H, W, ks), C.blob_map(rng, H, W, (0.2, 0.45, 0.7)[k % 3], t, 1.0 + 0.1 * min(ks[0], 40)), t, ks))
    return cases


def test_seventy_maps_in_two_groups(gpu, mixed):
    import pseg_amd
    first = _dev(mixed)
    assert_equal(mixed, first)
    _same(first, _dev(mixed))                                           # twice
    order = np.random.default_rng(5).permutation(len(mixed))
    perm = _dev([mixed[i] for i in order])
    _same([first[i] for i in order], perm)
    for k in range(len(mixed)):                                         # each alone
        _same([first[k]], _dev([mixed[k]]))
    pseg_amd.lib().pseg_release_workspace(0)
    _same(first, _dev(mixed))                                           # after a workspace release
    assert_equal(mixed, _dev(mixed, masks=False), masks=False)          # without masks
    none = _dev(mixed, max_regions=0)                                   # without a table: the wrapper asks again for the pages that have regions
    _same(first, none)


def test_counts_and_single_masks_of_the_c_entry(gpu, mixed):
    import ctypes
    from pseg_amd import engine as E
    n = len(mixed)
    want = [C.restated(c[1], c[2], *c[3], key=c[0]) for c in mixed]
    how = (E.REGIONS * n)(*[E.REGIONS(c[2], *c[3]) for c in mixed])
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    maps = [np.ascontiguousarray(c[1]) for c in mixed]
    masks = [np.full(m.shape, 0xA5, np.uint8) for m in maps]
    ptrs = [a.ctypes.data if k % 3 else None for k, a in enumerate(masks)]   # single entries may be NULL
    cap = 3
    rows = np.full((n, cap, 8), -5, np.int32)
    cnt = np.full(n, -5, np.int32)
    rc = E.lib().pseg_text_regions(0, n, P(*[m.ctypes.data for m in maps]), I(*[m.shape[0] for m in maps]), I(*[m.shape[1] for m in maps]),
                                   how, P(*ptrs), cap, rows.ctypes.data, cnt.ctypes.data)
    assert rc == 0, E.lib().pseg_last_error()
    over = 0
    for k in range(n):
        r = want[k][1].shape[0]
        assert cnt[k] == r
        if k % 3:
            assert np.array_equal(masks[k], want[k][0])
        else:
            assert (masks[k] == 0xA5).all()
        if r <= cap:
            assert np.array_equal(rows[k, :r], want[k][1]) and (rows[k, r:] == -5).all()
        else:
            over += 1
            assert (rows[k] == -5).all()            # the rows of a page above the cap are untouched
    assert 0 < over < n
    cnt[:] = -5
    rc = E.lib().pseg_text_regions(0, n, P(*[m.ctypes.data for m in maps]), I(*[m.shape[0] for m in maps]), I(*[m.shape[1] for m in maps]),
                                   how, None, 0, None, cnt.ctypes.data)
    assert rc == 0 and [int(v) for v in cnt] == [w[1].shape[0] for w in want]


def test_refusals_leave_the_outputs_untouched(gpu):
    from pseg_amd import engine as E
    _refusals(lambda *a: E.lib().pseg_text_regions(0, *a))
    import pseg_amd
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.text_regions([np.zeros((4, 4), np.uint8)], pseg_amd.TextRegions(1, kernels=(1, 1, 1)), device=99)


def test_one_large_page(gpu):
    import pseg_amd
    rng = np.random.default_rng(9)
    H, W = 2048, 1536
    lab = np.zeros((H, W), np.uint8)
    for y in range(60, H - 60, 45):                                     # text lines of 30 pixels: words of random length
        x = 80 + int(rng.integers(0, 40))
        while x < W - 120:
            w = int(rng.integers(30, 160))
            lab[y:y + 22, x:min(x + w, W - 80)] = rng.random((22, min(x + w, W - 80) - x)) < 0.55
            x += w + int(rng.integers(8, 30)) + (400 if rng.random() < 0.05 else 0)
        if rng.random() < 0.15:
            lab[y:y + 30, :] = 0
    lab[900:1300, 200:700] = 2                                          # an image block, another label
    ks = pseg_amd.region_kernels(30)
    case = ("large page", lab, 1, ks)
    dev = _dev([case])
    assert_equal([case], dev)
    assert 2 <= len(dev[0]["areas"]) <= 256


def test_get_text_regions_and_predict_regions(gpu, oracle_mod):
    import dataclasses
    import pseg_amd
    from test_eval_pages_gpu import _predictor_and_dataset
    from ocr4all_pixel_classifier.lib import pc_segmentation as S
    for posts, high_res in (([], False), (["cc_majority"], True)):
        pred, ds = _predictor_and_dataset(gpu, oracle_mod, posts, high_res)
        for k, d in enumerate(ds.data):
            d.line_height_px = 6 + k
        for chunk in (64, 2):
            got = pred.predict_regions(ds, 1, chunk=chunk)
            assert len(got) == len(ds.data)
            for d, regs in zip(ds.data, got):
                labels = np.asarray(pred.predict_single(d).labels).astype(np.uint8)
                ch = d.line_height_px * labels.shape[0] / d.original_shape[0]
                rec = pseg_amd.text_regions([labels], pseg_amd.TextRegions(1, char_height=ch), host=True)[0]
                polys = pseg_amd.trace_regions(rec["mask"], rec)
                assert len(regs) == len(polys)
                for r, p, b, a in zip(regs, polys, rec["boxes"], rec["areas"]):
                    assert np.array_equal(r.polygon, p) and r.box == tuple(b) and r.area == a
                    assert r.polygon_coords() == [tuple(v) for v in p.tolist()]
                check_polygons(rec["mask"], rec, polys)
                # the same page through get_text_regions: from the label map, and from its colour mask with the ColorMap
                cm = pred.settings.color_map
                one = S.get_text_regions(labels, ch, 1)
                two = S.get_text_regions(cm.lut()[labels], ch, cm)
                for r, q, s in zip(regs, one, two):
                    assert np.array_equal(r.polygon, q.polygon) and np.array_equal(r.polygon, s.polygon) and r.box == q.box == s.box
                assert len(one) == len(two) == len(regs)
                # the painted mask closes the islands and nothing else; a region scaled by 2 has four times the area
                painted = S.render_regions_mask(labels.shape, regs, (255, 0, 0))
                from scipy import ndimage
                whole = np.zeros(labels.shape, bool)
                cc, _ = ndimage.label(rec["mask"])
                for sy, sx in rec["seeds"]:
                    whole |= ndimage.binary_fill_holes(cc == cc[sy, sx], structure=np.ones((3, 3), bool))
                assert np.array_equal((painted == (255, 0, 0)).all(-1), whole)
                for r in regs[:3]:
                    assert r.scale(2).area == 4 * C.shoelace(r.polygon) and r.scale(2).box == tuple(2 * v for v in r.box)
