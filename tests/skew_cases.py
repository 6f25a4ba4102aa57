"""What the deskewing tests share (no test in here; `refusals` is run by the host and by the GPU test): the NumPy restatement of the
contract in include/pseg.h -- written from its text, with whole-array arithmetic, not from the C core --, the case grid and the
hand-made maps."""
import ctypes

import numpy as np

STRIP = 32


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def strip_counts(ink):
    """R[y][k]: ink pixels (non-zero bytes) of row y in strip k, int64."""
    H, W = ink.shape
    K = -(-W // STRIP)
    pad = np.zeros((H, K * STRIP), np.int64)
    pad[:, :W] = ink != 0
    return pad.reshape(H, K, STRIP).sum(2)


def offsets(a, W, D):
    K = -(-W // STRIP)
    cx2 = 64 * np.arange(K, dtype=np.int64) + 32 - W
    return (a * cx2 + D) // (2 * D)                                   # NumPy's // floors


def restated_skew(ink, A, D):
    """(index, scores): scores is uint64 (2 A + 1,), candidate a at a + A."""
    R = strip_counts(ink)
    H, K = R.shape
    W = ink.shape[1]
    offs = np.array([offsets(a, W, D) for a in range(-A, A + 1)])
    M = int(np.abs(offs).max())
    scores = []
    for off in offs:
        P = np.zeros(H + 2 * M, np.int64)
        for k in range(K):                                            # R[y][k] is P[j]'s term for j + off = y
            P[M - off[k]:M - off[k] + H] += R[:, k]
        assert P.sum() == R.sum()                                     # the apron drops nothing
        scores.append(sum(int(p) * int(p) for p in P[P != 0]))
    best = max(range(-A, A + 1), key=lambda a: (scores[a + A], -abs(a), a > 0))
    return best, np.array(scores, np.uint64)


def rotation_constants(a, D):
    r = np.sqrt(np.float64(D * D + a * a))
    C = int(np.floor(16384.0 * D / r + 0.5))
    S = int(np.floor(16384.0 * abs(a) / r + 0.5))
    return C, S if a >= 0 else -S


def restated_rotate(src, a, D, order, fill):
    H, W = src.shape
    C, S = rotation_constants(a, D)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    u, v = 2 * x - (W - 1), 2 * y - (H - 1)
    X = C * u - S * v + (W - 1) * 16384
    Y = S * u + C * v + (H - 1) * 16384
    assert np.abs(X).max() < 1 << 30 and np.abs(Y).max() < 1 << 30

    def tap(ys, xs):
        inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
        return np.where(inside, src[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], fill).astype(np.int64)

    if order == 0:
        return tap((Y + 16384) >> 15, (X + 16384) >> 15).astype(np.uint8)
    x0, fx, y0, fy, w = X >> 15, X & 32767, Y >> 15, Y & 32767, 32768
    out = ((w - fx) * (w - fy) * tap(y0, x0) + fx * (w - fy) * tap(y0, x0 + 1) + (w - fx) * fy * tap(y0 + 1, x0)
           + fx * fy * tap(y0 + 1, x0 + 1) + (1 << 29)) >> 30
    return out.astype(np.uint8)


# ---- the grid ------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 33), (33, 1), (2, 31), (31, 32), (32, 33), (64, 65), (63, 95), (70, 50), (129, 257)]
STEPS = [(1, 64), (16, 64), (89, 1024), (128, 512), (128, 4096)]
DENSITIES = [0.0, 0.02, 0.2, 1.0]
ORDERS = [0, 1]
FILLS = [0, 7, 255]


def random_ink(rng, shape, density):
    """An ink map of the density whose ink bytes are anything in 1..255."""
    return ((rng.random(shape) < density) * rng.integers(1, 256, shape)).astype(np.uint8)


def skew_grid(seed=2026, shapes=SHAPES):
    """[(name, ink, A, D)] over shapes x STEPS x DENSITIES, from a seed."""
    rng = np.random.default_rng(seed)
    return [("%dx%d A=%d D=%d d=%g" % (s[0], s[1], A, D, d), random_ink(rng, s, d), A, D)
            for s in shapes for A, D in STEPS for d in DENSITIES]


def rotate_grid(seed=2027, shapes=SHAPES):
    """[(name, src, index, D, order, fill)] over shapes x STEPS x ORDERS x FILLS x (0, +-1, +-A), from a seed."""
    rng = np.random.default_rng(seed)
    out = []
    for s in shapes:
        src = rng.integers(0, 256, s).astype(np.uint8)
        for A, D in STEPS:
            for order in ORDERS:
                for fill in FILLS:
                    for a in (0, 1, -1, A, -A):
                        out.append(("%dx%d a=%d D=%d order=%d fill=%d" % (s[0], s[1], a, D, order, fill), src, a, D, order, fill))
    return out


def crossing_lines(H=80, W=128, num=8, den=64):
    """Two one-pixel lines of slopes +num/den and -num/den through the centre: mirror-symmetric, W a multiple of the strip."""
    m = np.zeros((H, W), np.uint8)
    x = np.arange(W)
    t = num * (2 * x - (W - 1))                                       # doubled horizontal distance from the centre times num
    for sign in (1, -1):
        y = (H // 2) + sign * ((t + den) // (2 * den))
        m[y, x] = 1
    assert np.array_equal(m, m[:, ::-1])
    return m


def hand_cases():
    """[(name, ink, A, D)]: the maps made by hand."""
    out = []
    first = np.zeros((40, 100), np.uint8)
    first[0, :] = 200
    last = np.zeros((40, 100), np.uint8)
    last[-1, :] = 1
    for A, D in ((16, 64), (89, 1024)):
        out.append(("ink only in the first row A=%d" % A, first, A, D))
        out.append(("ink only in the last row A=%d" % A, last, A, D))
    ragged = np.zeros((45, 70), np.uint8)
    ragged[5::7, 64:] = 3
    out.append(("ink only in the last, ragged strip", ragged, 16, 64))
    rng = np.random.default_rng(5)
    out.append(("W < 32", random_ink(rng, (50, 20), 0.3), 16, 64))
    out.append(("1 x 16384 of ink", np.ones((1, 16384), np.uint8), 128, 512))
    out.append(("16384 x 512 of ink: a score of 2^32", np.full((16384, 512), 255, np.uint8), 1, 64))
    plateau = np.zeros((30, 64), np.uint8)
    plateau[10, :] = 1
    plateau[17, 3:50] = 1
    out.append(("a plateau of equal scores around 0", plateau, 89, 1024))
    one_strip = random_ink(rng, (30, 32), 0.2)
    out.append(("one strip: every score equal", one_strip, 128, 512))
    out.append(("a tie between +a and -a only", crossing_lines(), 16, 64))
    return out


def boundary_shapes():
    """Shapes one below, at and one above the constants the kernels use: the strip (32 columns), the 8-byte run and the 16-byte
    load (widths that move the rows' alignment), the rotation workgroup (8 rows x 32 runs) and the stride of the score workgroup
    (256 profile rows: H + 2 M around it)."""
    shapes = [(5, w) for w in (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 247, 248, 249, 255, 256, 257)]
    shapes += [(h, 40) for h in (7, 8, 9, 255, 256, 257)]
    # A = 16, D = 64, W = 40: M = 7, so H + 2 M = 255, 256, 257 at H = 241, 242, 243
    assert int(max(np.abs(offsets(a, 40, 64)).max() for a in (-16, 16))) == 7
    shapes += [(h, 40) for h in (241, 242, 243)]
    return shapes


# ---- the refusals ----------------------------------------------------------------------------------------------------------------

def refusals(L, host):
    """Every refusal of the list entries leaves the outputs untouched and names the map (shared with the GPU test)."""
    from pseg_amd import engine as E
    rng = np.random.default_rng(11)
    n = 3
    ms = [random_ink(rng, s, 0.3) for s in ((9, 11), (12, 7), (8, 8))]
    outs = [np.full(m.shape, 0xA5, np.uint8) for m in ms]
    idx = np.full(n, -77, np.int32)
    sc = [np.full(2 * 128 + 1, 0xA5A5, np.uint64) for _ in ms]
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    ptrs, op, sp = P(*[m.ctypes.data for m in ms]), P(*[a.ctypes.data for a in outs]), P(*[a.ctypes.data for a in sc])
    Hs, Ws = I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms])
    untouched = lambda: all((a == 0xA5).all() for a in outs) and (idx == -77).all() and all((a == 0xA5A5).all() for a in sc)
    err = lambda: L.pseg_last_error()

    def skew(n_, p, h, w, how, ix, s):
        return L.pseg_skew_maps_host(n_, p, h, w, how, ix, s) if host else L.pseg_skew_maps(0, n_, p, h, w, how, ix, s)

    def rotate(n_, p, h, w, rot, o):
        return L.pseg_rotate_maps_host(n_, p, h, w, rot, o) if host else L.pseg_rotate_maps(0, n_, p, h, w, rot, o)

    def deskew(n_, g, k, h, w, how, o, ix):
        return L.pseg_deskew_scans_host(n_, g, k, h, w, how, o, ix) if host else L.pseg_deskew_scans(0, n_, g, k, h, w, how, o, ix)

    sk = lambda *e: (E.SKEW * n)(*[E.SKEW(*x) for x in e])
    ro = lambda *e: (E.ROTATE * n)(*[E.ROTATE(*x) for x in e])
    ok, rok = (16, 64), (3, 64, 1, 255)
    # every limit one past its edge, in the last map: refused before the first one is worked on
    for name, e in [("steps 0", (0, 64)), ("steps 129", (129, 4096)), ("4 steps above denom", (17, 64)), ("negative steps", (-1, 64)),
                    ("denom 63", (1, 63)), ("denom 4097", (16, 4097))]:
        assert skew(n, ptrs, Hs, Ws, sk(ok, ok, e), idx.ctypes.data, sp) == -1 and b"map 2" in err() and untouched(), (name, err())
        assert deskew(n, ptrs, None, Hs, Ws, sk(ok, ok, e), op, idx.ctypes.data) == -1 and b"map 2" in err() and untouched(), (name, err())
    for name, e in [("4 |index| above denom", (17, 64, 0, 0)), ("the same, negative", (-17, 64, 0, 0)), ("order 2", (1, 64, 2, 0)),
                    ("order -1", (1, 64, -1, 0)), ("fill 256", (1, 64, 0, 256)), ("fill -1", (1, 64, 0, -1)), ("denom 63", (1, 63, 0, 0)),
                    ("denom 4097", (1, 4097, 0, 0))]:
        assert rotate(n, ptrs, Hs, Ws, ro(rok, rok, e), op) == -1 and b"map 2" in err() and untouched(), (name, err())
    how, rot = sk(ok, ok, ok), ro(rok, rok, rok)
    # shapes: empty, and 16385 pixels on a side (no byte of such a map is read)
    for hs, ws, item in ((I(9, 0, 8), Ws, b"map 1"), (Hs, I(11, 7, -8), b"map 2"), (I(9, 16385, 8), Ws, b"map 1"), (Hs, I(11, 7, 16385), b"map 2")):
        assert skew(n, ptrs, hs, ws, how, idx.ctypes.data, sp) == -1 and item in err() and untouched()
        assert rotate(n, ptrs, hs, ws, rot, op) == -1 and item in err() and untouched()
        assert deskew(n, ptrs, None, hs, ws, how, op, idx.ctypes.data) == -1 and item in err() and untouched()
    # NULL pointers: an entry, then each array in turn
    holed = P(ms[0].ctypes.data, None, ms[2].ctypes.data)
    oholed = P(outs[0].ctypes.data, outs[1].ctypes.data, None)
    assert skew(n, holed, Hs, Ws, how, idx.ctypes.data, sp) == -1 and b"map 1" in err()
    assert rotate(n, holed, Hs, Ws, rot, op) == -1 and b"map 1" in err()
    assert rotate(n, ptrs, Hs, Ws, rot, oholed) == -1 and b"map 2" in err()
    assert deskew(n, holed, None, Hs, Ws, how, op, idx.ctypes.data) == -1 and b"map 1" in err()
    assert deskew(n, ptrs, None, Hs, Ws, how, oholed, idx.ctypes.data) == -1 and b"map 2" in err()
    assert rotate(n, ptrs, Hs, Ws, rot, ptrs) == -1 and b"map 0" in err()          # an output cannot be its own source
    for k in range(5):
        a = [ptrs, Hs, Ws, how, idx.ctypes.data]
        a[k] = None
        assert skew(n, *a, sp) == -1, k
        a = [ptrs, Hs, Ws, rot, op]
        a[k] = None
        assert rotate(n, *a) == -1, k
    for k in range(6):
        a = [ptrs, Hs, Ws, how, op, idx.ctypes.data]
        a[k] = None
        assert deskew(n, a[0], None, *a[1:]) == -1, k
    assert skew(-1, ptrs, Hs, Ws, how, idx.ctypes.data, sp) == -1 and rotate(-1, ptrs, Hs, Ws, rot, op) == -1
    assert deskew(-1, ptrs, None, Hs, Ws, how, op, idx.ctypes.data) == -1
    assert untouched()
    # n == 0 touches nothing, not even a device
    assert skew(0, None, None, None, None, None, None) == 0 and rotate(0, None, None, None, None, None) == 0
    assert deskew(0, None, None, None, None, None, None, None) == 0
    # the scores may be NULL, as an array or entry by entry
    assert skew(n, ptrs, Hs, Ws, how, idx.ctypes.data, None) == 0
    want = [restated_skew(m, 16, 64) for m in ms]
    assert list(idx) == [w[0] for w in want]
    idx[:] = -77
    assert skew(n, ptrs, Hs, Ws, how, idx.ctypes.data, P(None, sc[1].ctypes.data, None)) == 0
    assert list(idx) == [w[0] for w in want] and np.array_equal(sc[1][:33], want[1][1])
    assert (sc[0] == 0xA5A5).all() and (sc[2] == 0xA5A5).all() and (sc[1][33:] == 0xA5A5).all()
