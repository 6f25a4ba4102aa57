"""What the binarisation tests share (no test in here; `refusals` is run by the host and by the GPU test): the NumPy restatement of
Sauvola's threshold that is their yardstick, the shape x window x k x density grid, the special images and the unevenly lit page."""
import ctypes

import numpy as np


def sauvola(g, w, k=0.2, R=128.0):
    """The ink map (uint8, ink = 1) and the float64 threshold plane of gray image g under Sauvola's threshold over a w x w window,
    indices mirrored without an edge repeat.  Integer box sums from integral images, then float64 in the documented order."""
    r = w // 2
    p = np.pad(g.astype(np.int64), r, mode='reflect')

    def box(a):
        I = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
        I[1:, 1:] = a.cumsum(0).cumsum(1)
        return I[w:, w:] - I[:-w, w:] - I[w:, :-w] + I[:-w, :-w]

    n = float(w * w)
    m = box(p) / n
    s = np.sqrt(np.maximum(box(p * p) / n - m * m, 0.0))
    T = m * (1.0 + k * (s / R - 1.0))
    return (g.astype(np.float64) <= T).astype(np.uint8), T


def fixed(g):
    """The fixed threshold: ink = g <= 127; the threshold plane is 127."""
    return (g <= 127).astype(np.uint8), np.full(g.shape, 127.0)


SHAPES = [(1, 1), (1, 37), (33, 1), (2, 2), (5, 7), (31, 65), (64, 128), (70, 50), (97, 130)]
WINDOWS = [3, 15, 37, 255]
KS = [0.0, 0.2, 0.5]
DENSITIES = [0.05, 0.3, 0.7]


def random_scan(rng, shape, density):
    """Random bytes: a share `density` of dark pixels (0..119) on light ones (130..255), every fifth pixel any byte."""
    dark = rng.random(shape) < density
    g = np.where(dark, rng.integers(0, 120, shape), rng.integers(130, 256, shape))
    g = np.where(rng.random(shape) < 0.2, rng.integers(0, 256, shape), g)
    return g.astype(np.uint8)


def grid_cases(seed=2024):
    """[(name, gray, window, k, R)] over SHAPES x WINDOWS x KS x DENSITIES, from a seed."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in SHAPES:
        for w in WINDOWS:
            for k in KS:
                for d in DENSITIES:
                    out.append(("%dx%d w=%d k=%g d=%g" % (shape[0], shape[1], w, k, d), random_scan(rng, shape, d), w, k, 128.0))
    return out


def special_cases():
    """Flat, two-valued and checkerboard images, every window."""
    rng = np.random.default_rng(7)
    imgs = [("flat %d" % v, np.full((23, 41), v, np.uint8)) for v in (0, 1, 127, 128, 255)]
    imgs.append(("two values", np.where(rng.random((40, 53)) < 0.3, 30, 200).astype(np.uint8)))
    imgs.append(("two neighbouring values", np.where(rng.random((19, 66)) < 0.5, 127, 128).astype(np.uint8)))
    yy, xx = np.mgrid[0:37, 0:70]
    imgs.append(("checkerboard", np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)))
    imgs.append(("checkerboard of 3 x 5 fields", np.where((yy // 3 + xx // 5) % 2 == 0, 40, 210).astype(np.uint8)))
    return [(name + " w=%d" % w, g, w, 0.2, 128.0) for name, g in imgs for w in WINDOWS]


def restated(cases):
    """[(ink, T)] of the restatement for a list of cases; window 0 is the fixed threshold."""
    return [fixed(g) if w == 0 else sauvola(g, w, k, R) for _, g, w, k, R in cases]


def uneven_page(seed=5, H=384, W=512, line_height=16):
    """A page of glyph-like strokes under uneven light: -> (gray uint8, glyph map uint8 with ink = 1, line height).  The paper falls
    from 235 at the left edge to about 80 at the right one, ink is 0.35 x paper, and noise of sigma 3 lies on both."""
    rng = np.random.default_rng(seed)
    glyph = np.zeros((H, W), np.uint8)
    pitch = line_height * 2
    for top in range(line_height, H - pitch, pitch):
        x = 12
        while x < W - 24:
            gw = int(rng.integers(8, 14))
            if rng.random() < 0.15:                               # a space between words
                x += gw
                continue
            box = glyph[top:top + line_height, x:x + gw]
            box[:, :2] = 1                                        # a stem, a bar and sometimes a second stem or a foot: 2-pixel strokes
            box[int(rng.integers(0, line_height - 2)):, :][:2, :] = 1
            if rng.random() < 0.6:
                box[:, -2:] = 1
            if rng.random() < 0.4:
                box[-2:, :] = 1
            x += gw + 4
    paper = np.linspace(235.0, 80.0, W)[None, :] * np.ones((H, 1))
    gray = np.where(glyph != 0, 0.35 * paper, paper) + rng.normal(0.0, 3.0, (H, W))
    return np.clip(np.rint(gray), 0, 255).astype(np.uint8), glyph, line_height


def lit_text_scan(k, H, W, dark=0.4):
    """A synthetic text scan (ink dark) whose light falls off to `dark` of its level at the right edge: scan <= 127 turns that side
    into ink, an adaptive threshold does not."""
    from pseg_amd import synth
    scan = (255 - synth.synth_page(k, H, W, 3)[0]).astype(np.float64)
    return np.rint(scan * np.linspace(1.0, dark, W)[None, :]).astype(np.uint8)


def _call(L, host, n, ptrs, Hs, Ws, how, outs, thrs):
    args = (n, ptrs, Hs, Ws, how, outs, thrs)
    return L.pseg_binarize_scans_host(*args) if host else L.pseg_binarize_scans(0, *args)


def refusals(L, host):
    """Every refusal of the list entries leaves the outputs untouched and names the scan (shared with the GPU test)."""
    from pseg_amd import engine as E
    rng = np.random.default_rng(11)
    n = 3
    gs = [random_scan(rng, s, 0.3) for s in ((9, 11), (12, 7), (8, 8))]
    inks = [np.full(g.shape, 0xA5, np.uint8) for g in gs]
    thrs = [np.full(g.shape, -7.0) for g in gs]
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    ptrs, outs, tp = P(*[g.ctypes.data for g in gs]), P(*[a.ctypes.data for a in inks]), P(*[a.ctypes.data for a in thrs])
    Hs, Ws = I(*[g.shape[0] for g in gs]), I(*[g.shape[1] for g in gs])

    def table(*entries):
        return (E.BINARIZE * n)(*[E.BINARIZE(*e) for e in entries])

    ok = (15, 0.2, 128.0)
    bad = [("even window", (14, 0.2, 128.0)), ("window 1", (1, 0.2, 128.0)), ("window 257", (257, 0.2, 128.0)), ("negative window", (-3, 0.2, 128.0)),
           ("k below 0", (15, -0.01, 128.0)), ("k above 1", (15, 1.01, 128.0)), ("k nan", (15, float("nan"), 128.0)),
           ("R zero", (15, 0.2, 0.0)), ("R negative", (15, 0.2, -1.0)), ("R nan", (15, 0.2, float("nan")))]
    untouched = lambda: all((a == 0xA5).all() for a in inks) and all((t == -7.0).all() for t in thrs)
    for name, e in bad:
        # in the last scan: refused before the first one is worked on
        assert _call(L, host, n, ptrs, Hs, Ws, table(ok, (0, 0.0, 0.0), e), outs, tp) == -1, name
        assert b"scan 2" in L.pseg_last_error() and untouched(), (name, L.pseg_last_error())
    how = table(ok, ok, ok)
    assert _call(L, host, n, P(gs[0].ctypes.data, None, gs[2].ctypes.data), Hs, Ws, how, outs, tp) == -1 and b"scan 1" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, Hs, Ws, how, P(inks[0].ctypes.data, inks[1].ctypes.data, None), tp) == -1 and b"scan 2" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, I(9, 0, 8), Ws, how, outs, tp) == -1 and b"scan 1" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, Hs, I(11, 7, -8), how, outs, tp) == -1 and b"scan 2" in L.pseg_last_error()
    for k in range(1, 6):                                       # each array NULL in turn
        args = [ptrs, Hs, Ws, how, outs]
        args[k - 1] = None
        assert _call(L, host, n, *args, tp) == -1, k
    assert _call(L, host, -1, ptrs, Hs, Ws, how, outs, tp) == -1
    assert untouched()
    assert _call(L, host, 0, None, None, None, None, None, None) == 0
    # the threshold array, or an entry of it, may be NULL; a fixed entry does not read k and R
    assert _call(L, host, n, ptrs, Hs, Ws, table(ok, (0, 9.0, -1.0), ok), outs, P(thrs[0].ctypes.data, None, None)) == 0
    assert np.array_equal(inks[0], sauvola(gs[0], 15)[0]) and np.array_equal(thrs[0], sauvola(gs[0], 15)[1])
    assert np.array_equal(inks[1], (gs[1] <= 127).astype(np.uint8)) and (thrs[1] == -7.0).all() and (thrs[2] == -7.0).all()
    for a in inks:
        a[...] = 0xA5
    assert _call(L, host, n, ptrs, Hs, Ws, how, outs, None) == 0
    assert all(np.array_equal(a, sauvola(g, 15)[0]) for a, g in zip(inks, gs))
