"""What the despeckling tests share (no test in here; `refusals` is run by the host and by the GPU test): the scipy.ndimage
restatement that is their yardstick, the shape x connectivity x max_area x density grid and the hand-placed maps."""
import ctypes

import numpy as np
from scipy import ndimage

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
ONES = np.ones((3, 3), bool)


def restated(ink, max_area, connectivity):
    """(out uint8, counts int64[3]) of the contract: components of at most max_area pixels erased, kept ink 1; counts are the
    components erased, the pixels erased and the components kept."""
    lab, n = ndimage.label(ink != 0, CROSS if connectivity == 4 else ONES)
    size = np.bincount(lab.ravel(), minlength=n + 1)
    out = ((lab > 0) & (size[lab] > max_area)).astype(np.uint8)
    comp = size[1:]
    small = comp <= max_area
    return out, np.array([small.sum(), comp[small].sum(), (~small).sum()], np.int64)


SHAPES = [(1, 1), (1, 37), (33, 1), (2, 2), (31, 65), (32, 64), (33, 63), (64, 128), (70, 50), (97, 130)]
CONNECTIVITIES = [4, 8]
AREAS = [1, 2, 9, 64, 5000]
DENSITIES = [0.05, 0.3, 0.7, 0.9]


def random_map(rng, shape, density):
    return (rng.random(shape) < density).astype(np.uint8)


def grid_cases(seed=2025, shapes=SHAPES):
    """[(name, ink, max_area, connectivity)] over shapes x CONNECTIVITIES x AREAS x DENSITIES, from a seed."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        for c in CONNECTIVITIES:
            for a in AREAS:
                for d in DENSITIES:
                    out.append(("%dx%d c=%d a=%d d=%g" % (shape[0], shape[1], c, a, d), random_map(rng, shape, d), a, c))
    return out


def serpentine(H, W):
    """One 1-pixel path that runs along every second row and turns at alternating ends: a single component at either connectivity."""
    m = np.zeros((H, W), np.uint8)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def hand_cases():
    """[(name, ink, max_area, connectivity, expected counts or None)]."""
    out = []
    for c in CONNECTIVITIES:
        for a in (1, 6, 40):
            m = np.zeros((20, 90), np.uint8)
            m[3, 2:2 + a] = 1                                      # exactly max_area pixels: erased
            m[9, 2:3 + a] = 1                                      # max_area + 1 pixels: kept
            out.append(("a and a + 1, a=%d c=%d" % (a, c), m, a, c, [1, a, 1]))
        out.append(("all ink c=%d" % c, np.ones((40, 70), np.uint8), 2799, c, [0, 0, 1]))
        out.append(("all ink, erased c=%d" % c, np.ones((40, 70), np.uint8), 2800, c, [1, 2800, 0]))
        out.append(("all paper c=%d" % c, np.zeros((40, 70), np.uint8), 5, c, [0, 0, 0]))
        s = serpentine(75, 141)
        out.append(("serpentine kept c=%d" % c, s, int(s.sum()) - 1, c, [0, 0, 1]))
        out.append(("serpentine erased c=%d" % c, s, int(s.sum()), c, [1, int(s.sum()), 0]))
    yy, xx = np.mgrid[0:37, 0:70]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    out.append(("checkerboard c=4", board, 1, 4, [int(board.sum()), int(board.sum()), 0]))
    out.append(("checkerboard c=8", board, 1, 8, [0, 0, 1]))
    rng = np.random.default_rng(3)
    b = (random_map(rng, (45, 77), 0.3) * rng.integers(1, 256, (45, 77))).astype(np.uint8)   # non-zero bytes other than 1
    out.append(("bytes other than 1 c=8", b, 4, 8, None))
    out.append(("bytes other than 1 c=4", b, 4, 4, None))
    return out


def _call(L, host, n, ptrs, Hs, Ws, how, outs, cnt):
    args = (n, ptrs, Hs, Ws, how, outs, cnt)
    return L.pseg_despeckle_maps_host(*args) if host else L.pseg_despeckle_maps(0, *args)


def refusals(L, host):
    """Every refusal of the list entries leaves the outputs untouched and names the map (shared with the GPU test)."""
    from pseg_amd import engine as E
    rng = np.random.default_rng(11)
    n = 3
    ms = [random_map(rng, s, 0.3) for s in ((9, 11), (12, 7), (8, 8))]
    outs = [np.full(m.shape, 0xA5, np.uint8) for m in ms]
    cnt = np.full((n, 3), -7, np.int64)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    ptrs, op = P(*[m.ctypes.data for m in ms]), P(*[a.ctypes.data for a in outs])
    Hs, Ws = I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms])

    def table(*entries):
        return (E.DESPECKLE * n)(*[E.DESPECKLE(*e) for e in entries])

    ok = (4, 8)
    untouched = lambda: all((a == 0xA5).all() for a in outs) and (cnt == -7).all()
    bad = [("negative max_area", (-1, 8)), ("max_area above the range", ((1 << 24) + 1, 8)), ("connectivity 3", (4, 3)),
           ("connectivity 0", (4, 0)), ("connectivity 6", (4, 6))]
    for name, e in bad:
        # in the last map: refused before the first one is worked on
        assert _call(L, host, n, ptrs, Hs, Ws, table(ok, (0, 0), e), op, cnt.ctypes.data) == -1, name
        assert b"map 2" in L.pseg_last_error() and untouched(), (name, L.pseg_last_error())
    how = table(ok, ok, ok)
    assert _call(L, host, n, P(ms[0].ctypes.data, None, ms[2].ctypes.data), Hs, Ws, how, op, cnt.ctypes.data) == -1 and b"map 1" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, Hs, Ws, how, P(outs[0].ctypes.data, outs[1].ctypes.data, None), cnt.ctypes.data) == -1 and b"map 2" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, I(9, 0, 8), Ws, how, op, cnt.ctypes.data) == -1 and b"map 1" in L.pseg_last_error()
    assert _call(L, host, n, ptrs, Hs, I(11, 7, -8), how, op, cnt.ctypes.data) == -1 and b"map 2" in L.pseg_last_error()
    # a shape of 2^31 pixels or more (what check_shape refuses): unsupported, before a byte is read
    assert _call(L, host, n, ptrs, I(9, 12, 65536), I(11, 7, 32768), how, op, cnt.ctypes.data) == -5 and b"map 2" in L.pseg_last_error()
    for k in range(1, 6):                                       # each array NULL in turn
        args = [ptrs, Hs, Ws, how, op]
        args[k - 1] = None
        assert _call(L, host, n, *args, cnt.ctypes.data) == -1, k
    assert _call(L, host, -1, ptrs, Hs, Ws, how, op, cnt.ctypes.data) == -1
    assert untouched()
    assert _call(L, host, 0, None, None, None, None, None, None) == 0
    # the counts may be NULL; an entry with max_area 0 does not read its connectivity and leaves the bytes as they are
    src1 = (ms[1] * 77).astype(np.uint8)
    assert _call(L, host, n, P(ms[0].ctypes.data, src1.ctypes.data, ms[2].ctypes.data), Hs, Ws, table(ok, (0, 3), (2, 4)), op, None) == 0
    assert np.array_equal(outs[0], restated(ms[0], 4, 8)[0]) and np.array_equal(outs[1], src1) and np.array_equal(outs[2], restated(ms[2], 2, 4)[0])
    assert (cnt == -7).all()
