"""pseg_char_heights' host side, no GPU: the window geometry the kernel was compiled with, the ownership rule that lets a window
decide locally (restated in NumPy with exactly that geometry and compared with the oracle's page-wide labelling), the empty list,
and the histogram-to-median helper."""
import ctypes

import numpy as np
from scipy import ndimage

H_LO, H_HI, W_LO, W_HI = 10, 60, 5, 50          # lib/image_ops.py:72-76


def _glyph(h, w):
    return 0.5 < (w / h) < 2 and H_LO < h < H_HI and W_LO < w < W_HI


def test_window_aprons_cover_the_largest_glyph():
    from pseg_amd import engine as E
    assert "pseg_char_heights" in E.EXPORTED_SYMBOLS and "pseg_char_height_window" in E.EXPORTED_SYMBOLS
    th, tw, above, below, left, right = E.char_height_window()
    assert th >= 1 and tw >= 1
    assert above >= 1 and below >= H_HI - 1 and left >= W_HI - 1 and right >= W_HI - 1
    L = E.lib()
    assert L.pseg_char_height_window(None, None, None, None, None, None) == 0          # every pointer is optional


def _rule_heights(ink, geom, explicit_sides):
    """Heights counted by the tiles' local rule.  explicit_sides: also demand that the fragment has no pixel on a window side whose
    outward neighbour lies inside the scan (the long form of the rule); without it the box filter alone decides (what the kernel does)."""
    th, tw, above, below, left, right = geom
    H, W = ink.shape
    hs = []
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            wy0, wy1, wx0, wx1 = y0 - above, y0 + th + below, x0 - left, x0 + tw + right          # window, end exclusive
            win = np.zeros((wy1 - wy0, wx1 - wx0), bool)
            sy0, sy1, sx0, sx1 = max(wy0, 0), min(wy1, H), max(wx0, 0), min(wx1, W)
            win[sy0 - wy0:sy1 - wy0, sx0 - wx0:sx1 - wx0] = ink[sy0:sy1, sx0:sx1]                   # paper outside the scan
            if not win[above:above + th, left:left + tw].any():
                continue
            lab, n = ndimage.label(win)
            for k, sl in enumerate(ndimage.find_objects(lab), 1):
                fy = sl[0].start                                                                 # first pixel: top-most row, left-most in it
                fx = sl[1].start + int(np.argmax(lab[fy, sl[1]] == k))
                if not (above <= fy < above + th and left <= fx < left + tw):
                    continue
                if explicit_sides:
                    top = sl[0].start == 0 and wy0 - 1 >= 0
                    bottom = sl[0].stop == win.shape[0] and wy1 < H
                    lft = sl[1].start == 0 and wx0 - 1 >= 0
                    rgt = sl[1].stop == win.shape[1] and wx1 < W
                    if top or bottom or lft or rgt:
                        continue
                h, w = sl[0].stop - sl[0].start, sl[1].stop - sl[1].start
                if _glyph(h, w):
                    hs.append(h)
    return sorted(hs)


def _random_page(seed):
    """0/255 page (ink 0): glyph-sized frames and boxes around the filter's bounds, rules, large blobs, speckles."""
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(120, 260)), int(rng.integers(150, 330))
    ink = np.zeros((H, W), bool)
    for _ in range(int(rng.integers(15, 40))):
        h, w = int(rng.choice([3, 10, 11, 12, 20, 35, 58, 59, 60, 75])), int(rng.choice([2, 5, 6, 9, 20, 30, 48, 49, 50, 51, 70]))
        if rng.random() < 0.5:                                                                 # a shape the filter admits
            h = int(rng.integers(H_LO + 1, H_HI))
            w = int(rng.integers(max(W_LO + 1, h // 2 + 1), min(W_HI, 2 * h)))
        y, x = int(rng.integers(-5, H)), int(rng.integers(-5, W))
        ya, yb, xa, xb = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
        if ya >= yb or xa >= xb:
            continue
        ink[ya - 1:yb + 1, max(xa - 1, 0):xb + 1] = False                                      # (mostly) keep shapes apart
        ink[ya:yb, xa:xb] = True
        if rng.random() < 0.5 and yb - ya > 2 and xb - xa > 2:
            ink[ya + 1:yb - 1, xa + 1:xb - 1] = False                                          # a hollow frame
    for _ in range(int(rng.integers(0, 3))):
        if rng.random() < 0.5:
            ink[int(rng.integers(0, H)), :] = True                                             # a rule across the page
        else:
            ink[:, int(rng.integers(0, W))] = True
    if rng.random() < 0.5:
        y, x = int(rng.integers(0, H - 40)), int(rng.integers(0, W - 40))
        blob = ink[y:y + int(rng.integers(61, 120)), x:x + int(rng.integers(51, 150))]          # a view: a ragged blob larger than any glyph
        blob |= rng.random(blob.shape) < 0.8
    ink |= rng.random((H, W)) < 0.01                                                           # speckles join and split shapes
    return np.where(ink, 0, 255).astype(np.uint8)


def test_ownership_rule_equals_page_wide_labelling(oracle_mod):
    from pseg_amd import engine as E
    geom = E.char_height_window()
    counted = 0
    for seed in range(50):
        page = _random_page(seed)
        ink = page == 0
        lab, _ = ndimage.label(ink)
        want = sorted(sl[0].stop - sl[0].start for sl in ndimage.find_objects(lab)
                      if _glyph(sl[0].stop - sl[0].start, sl[1].stop - sl[1].start))
        got = _rule_heights(ink, geom, explicit_sides=False)
        assert got == want, seed                                                               # every qualifying component once, nothing else
        assert _rule_heights(ink, geom, explicit_sides=True) == want, seed                     # the side test adds nothing: the aprons imply it
        counted += len(want)
        median = want[len(want) // 2] if want else None
        assert oracle_mod.compute_char_height_from_gray(page, inverse=False) == median, seed
    assert counted >= 100                                                                      # the pages do hold glyphs: two per page and more


def test_empty_list_needs_no_device():
    from pseg_amd import engine as E
    assert E.lib().pseg_char_heights(0, 0, None, None, None, 0, None, None) == 0
    assert E.lib().pseg_char_heights(99, 0, None, None, None, 1, None, None) == 0              # not even the device index is looked at
    assert E.char_heights([]) == ([], [])


def test_median_from_bins():
    from pseg_amd import engine as E
    rng = np.random.default_rng(7)
    first, nb = H_LO + 1, H_HI - H_LO - 1
    assert E.char_height_median(np.zeros(nb, np.uint32), first) is None
    cases = [[11], [59], [11, 59], [20, 20, 21, 21], [11, 12, 13], [30, 40]]
    cases += [list(rng.integers(first, H_HI, size=int(n))) for n in list(range(1, 12)) + [100, 101, 1000]]
    for hs in cases:
        bins = np.bincount(np.asarray(hs) - first, minlength=nb).astype(np.uint32)
        assert E.char_height_median(bins, first) == sorted(hs)[len(hs) // 2], hs
    h = ctypes.c_int()
    assert E.lib().pseg_char_height_median(None, nb, first, ctypes.byref(h)) != 0
