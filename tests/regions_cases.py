"""The text regions' contract restated in NumPy / SciPy (include/pseg.h, pseg_text_regions), and the cases the host and
the GPU tests share.  The 1-D passes are prefix sums over padded arrays, so a side of 255 on a large map stays cheap."""
import numpy as np
from scipy import ndimage

SHAPES = [(1, 1), (1, 70), (70, 1), (31, 63), (32, 64), (33, 65), (63, 127), (64, 128), (65, 129), (100, 200), (200, 333)]
DENSITIES = [0.15, 0.4, 0.7]


def region_kernels(ch):
    return tuple(min(255, max(1, int(v))) for v in (ch, ch / 3, ch / 1.1))


TRIPLES = [(1, 1, 1), (2, 2, 2), (3, 1, 2), (4, 1, 3)] + [region_kernels(c) for c in (7, 11, 12, 23, 40)] + \
          [(64, 21, 58), (65, 22, 59), (255, 85, 231)]


def _window_sum(m, k, axis, outside):
    """sum over d in 0..k-1 of m[i + d - k//2] along axis, m = outside beyond the map."""
    a = k // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (a + 1, k - 1 - a)                 # one more in front: the prefix sum's zero
    p = np.pad(m.astype(np.int64), pad, constant_values=int(outside))
    c = np.cumsum(p, axis=axis)
    n = m.shape[axis]
    hi = np.take(c, np.arange(k, k + n), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return hi - lo


def dil(m, k):
    x = _window_sum(m, k, 1, 0) > 0
    return _window_sum(x, k, 0, 0) > 0


def ero(m, k):
    x = _window_sum(m, k, 1, 1) == k
    return _window_sum(x, k, 0, 1) == k


def stages(lab, t, k1, k2, k3):
    m0 = np.asarray(lab) == t
    m1 = ero(dil(m0, k1), k1)
    m3 = dil(ero(m1, k2), k2)
    rt = ero(dil(dil(m3, k3), k3), k3)
    return m3, rt


_REF = {}


def restated(lab, t, k1, k2, k3, key=None):
    """-> (mask uint8, rows (r,8) int32) as the contract states them.  key: cache the result under it (the reference is computed once
    and shared)."""
    if key is not None and key in _REF:
        return _REF[key]
    m3, rt = stages(lab, t, k1, k2, k3)
    T = m3 | ndimage.binary_fill_holes(rt)
    cc, r = ndimage.label(T)                       # the cross: 4-connectivity
    rows = np.zeros((r, 8), np.int32)
    areas = np.bincount(cc.ravel(), minlength=r + 1)
    for i, sl in enumerate(ndimage.find_objects(cc)):
        y0, y1, x0, x1 = sl[0].start, sl[0].stop, sl[1].start, sl[1].stop
        sx = x0 + int(np.argmax(cc[y0, x0:x1] == i + 1))
        rows[i] = (x0, y0, x1, y1, areas[i + 1], y0, sx, 0)
    if r:
        order = np.lexsort((rows[:, 6], rows[:, 5]))
        rows = rows[order]
    out = (T.astype(np.uint8), rows)
    if key is not None:
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        _REF[key] = out
    return out


def blob_map(rng, H, W, density, t, sigma=2.5):
    """A label map whose label t forms blobs (smoothed noise cut at the density's quantile); other ids elsewhere."""
    noise = ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma, mode="nearest")
    cut = np.quantile(noise, 1.0 - density)
    lab = rng.integers(0, 4, (H, W)).astype(np.uint8)
    lab[lab == t] = (t + 1) % 4
    lab[noise >= cut] = t
    return lab


def grid_cases(seed=11, shapes=SHAPES, triples=TRIPLES, densities=DENSITIES):
    """(name, label map, t, (k1, k2, k3)) over shapes x triples x densities.  The name is the key of the cached reference: it holds
    everything the map is drawn from (the shapes, sides and densities are drawn in order from the seed: callers that pass other lists
    pass another seed)."""
    rng = np.random.default_rng(seed)
    cases = []
    for (H, W) in shapes:
        for ks in triples:
            for d in densities:
                t = int(rng.integers(0, 4))
                sigma = 1.0 + 0.12 * ks[0] if ks[0] < 64 else 6.0
                cases.append(("seed %d: %dx%d k=%r d=%g" % (seed, H, W, ks, d), blob_map(rng, H, W, d, t, sigma), t, ks))
    return cases


def hand_cases():
    """Hand-made maps, sides (1, 1, 1) unless said: (name, label map, t, ks, expected number of regions or None)."""
    out = []
    ident = (1, 1, 1)

    def blank(H, W, v=0):
        return np.full((H, W), v, np.uint8)
    out.append(("all label", blank(40, 70, 2), 2, ident, 1))
    out.append(("none", blank(40, 70, 2), 1, ident, 0))
    m = blank(80, 160)                             # a ring whose hole spans the four-tile corner at (32, 64)
    m[20:50, 40:100] = 1
    m[25:45, 45:95] = 0
    out.append(("ring over a tile corner", m, 1, ident, 1))
    m = blank(70, 140)                             # a ring touching the map's edge: its inside is still a hole
    m[0:40, 0:80] = 1
    m[5:35, 5:75] = 0
    out.append(("ring at the map's edge", m, 1, ident, 1))
    m = blank(70, 140)                             # a background notch that reaches the edge: not a hole
    m[10:60, 0:100] = 1
    m[30:35, 0:70] = 0
    out.append(("notch to the edge", m, 1, ident, 1))
    m = blank(50, 90)                              # a pocket joined to the outside only diagonally: a hole
    m[10:30, 10:40] = 1
    m[11:20, 11:20] = 0
    m[10, 10] = 0                                  # the corner pixel opens a diagonal way out of the pocket at (11, 11)
    out.append(("diagonal pocket", m, 1, ident, 1))
    m = blank(50, 90)                              # two regions touching only diagonally: two rows
    m[10:20, 10:20] = 1
    m[20:30, 20:30] = 1
    out.append(("diagonal neighbours", m, 1, ident, 2))
    m = blank(120, 300)                            # a region larger than a tile, with a large hole and an island in it
    m[5:110, 7:290] = 1
    m[20:90, 30:250] = 0
    m[40:60, 100:180] = 1
    out.append(("larger than a tile", m, 1, ident, 1))
    m = blank(60, 130, 7)
    m[10:30, 20:90] = 0
    out.append(("label id 0", m, 0, ident, 1))
    m = blank(60, 130, 7)
    m[10:30, 20:90] = 255
    m[40:50, 100:129] = 255
    out.append(("label id 255", m, 255, ident, 2))
    m = blank(64, 128)                             # a serpentine: one component folding across tile edges many times
    for y in range(0, 64, 2):
        m[y, :] = 1
    for i, y in enumerate(range(1, 63, 2)):
        m[y, 127 if i % 2 == 0 else 0] = 1
    out.append(("serpentine", m, 1, ident, 1))
    m = blank(66, 130)                             # a checkerboard: every unset pixel inside is a hole of its own, one region remains
    m[::2, ::2] = 1
    m[1::2, 1::2] = 1
    out.append(("checkerboard", m, 1, ident, None))
    m = blank(66, 130)                             # dots: every set pixel its own region
    m[::2, ::2] = 1
    out.append(("dots", m, 1, ident, 33 * 65))
    m = blank(90, 200)                             # real sides on a hand-made page: two text lines that the join merges
    m[20:30, 20:180:3] = 1
    m[40:50, 20:180:3] = 1
    out.append(("two lines", m, 1, region_kernels(12), None))
    return out


def shoelace(poly):
    x, y = poly[:, 0].astype(np.int64), poly[:, 1].astype(np.int64)
    return int(abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) // 2)


def even_odd(poly, H, W):
    """The pixels whose centres lie inside the rectilinear polygon (even-odd rule): every vertical edge toggles what is right of it."""
    inside = np.zeros((H, W), bool)
    nxt = np.roll(poly, -1, axis=0)
    for (x0, y0), (x1, y1) in zip(poly, nxt):
        if x0 == x1 and y0 != y1:
            inside[min(y0, y1):max(y0, y1), x0:] ^= True
    return inside
