"""Shared by tests/test_label_masks_host.py and tests/test_label_masks_gpu.py: colour tables, masks, the grid of shapes and the
restatement -- oracle.resize.resize_nearest(ColorMap.to_labels(rgb), shape) and NumPy counts.  Built once per process."""
import functools

import numpy as np

# source shape -> output shape (two different scales on the two axes among them)
SHAPES = [((1, 1), (1, 1)), ((1, 37), (1, 19)), ((33, 1), (70, 1)), ((70, 50), (35, 25)), ((35, 25), (70, 50)), ((64, 48), (64, 48)),
          ((97, 131), (41, 77))]
TABLES = [0, 1, 3, 8, 17, 256]

# the first entries of every table: black with a non-zero id, a colour with id 0, neighbours that differ by 1 in one channel only, ids
# in no order
FIRST = [((0, 0, 0), 5), ((255, 0, 0), 0), ((255, 0, 1), 3), ((254, 0, 0), 200), ((255, 1, 0), 1), ((0, 0, 1), 255), ((0, 1, 0), 2), ((1, 0, 0), 77)]


def table(n, seed=11):
    """n distinct colours and their ids -> (colors (n,3) uint8, ids (n,) uint8)."""
    rng = np.random.default_rng(seed)
    entries = list(FIRST[:n])
    seen = {c for c, _ in entries}
    while len(entries) < n:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        if c not in seen and c[0] < 250:                    # (250.., x, y) stays free for the unknown colours
            seen.add(c)
            entries.append((c, int(rng.integers(0, 256))))
    return (np.array([c for c, _ in entries], np.uint8).reshape(-1, 3), np.array([i for _, i in entries], np.uint8))


def color_map(colors, ids):
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    return ColorMap({tuple(int(v) for v in c): (int(i), "label %d" % k) for k, (c, i) in enumerate(zip(colors, ids))})


def rgb_mask(rng, shape, colors, unknown=0.08):
    """Flat regions of the table's colours, with single pixels of colours no table holds -- some of them one step from a table colour."""
    H, W = shape
    n = len(colors)
    out = np.empty((H, W, 3), np.uint8)
    bh, bw = max(1, H // 5), max(1, W // 6)
    if n:
        block = rng.integers(0, n, (H // bh + 1, W // bw + 1))
        pick = np.where(rng.random((H, W)) < 0.15, rng.integers(0, n, (H, W)), block[np.arange(H)[:, None] // bh, np.arange(W)[None, :] // bw])
        out[:] = colors[pick]
    else:
        out[:] = rng.integers(0, 256, (H, W, 3))
    odd = rng.random((H, W)) < unknown
    strange = np.stack([rng.integers(250, 254, (H, W)), rng.integers(0, 3, (H, W)), rng.integers(0, 3, (H, W))], -1).astype(np.uint8)
    out[odd] = strange[odd]
    return out


def id_mask(rng, shape):
    """A 1-channel source: label ids, every byte value where the mask is large enough."""
    m = rng.integers(0, 256, shape).astype(np.uint8)
    flat = m.reshape(-1)
    k = min(256, flat.size)
    flat[rng.permutation(flat.size)[:k]] = np.arange(k, dtype=np.uint8)
    return m


def restate(mask, shape, colors, ids):
    """-> (labels uint8 (H,W), counts int64[257]) by the issue's reference: lookup on the whole mask, then the order-0 resize."""
    from oracle import resize as oresize
    if mask.ndim == 2:
        lab0, unk0 = mask, np.zeros(mask.shape, np.uint8)
    else:
        lab0 = color_map(colors, ids).to_labels(mask)
        key = (mask[..., 0].astype(np.int64) << 16) | (mask[..., 1].astype(np.int64) << 8) | mask[..., 2]
        known = (colors[:, 0].astype(np.int64) << 16) | (colors[:, 1].astype(np.int64) << 8) | colors[:, 2]
        unk0 = (~np.isin(key, known)).astype(np.uint8)
    lab = oresize.resize_nearest(lab0, shape)
    assert lab.dtype == np.float64
    lab = lab.astype(np.uint8)
    counts = np.zeros(257, np.int64)
    counts[:256] = np.bincount(lab.reshape(-1), minlength=256)
    counts[256] = int(oresize.resize_nearest(unk0, shape).sum())
    return lab, counts


def geometry_shapes():
    """Output widths one below, at and one above the kernel's pixels per thread, per workgroup row and per workgroup, over heights
    around the workgroup's rows."""
    from pseg_amd import engine as E
    run, runs, rows = E.label_masks_geometry()[:3]
    out = []
    for k, w in enumerate(sorted({run, run * runs, run * runs * rows})):
        for d in (-1, 0, 1):
            out.append(((6 + d + k, 23), (rows + d, w + d)))
    return out


@functools.lru_cache(maxsize=None)
def grid():
    """[(name, mask, out_shape, n_colors)] over SHAPES + geometry_shapes() x TABLES (RGB), and the 1-channel sources; with
    want[i] = restate(...).  Computed once, shared and left unchanged."""
    rng = np.random.default_rng(2024)
    cases = []
    for src, dst in SHAPES + geometry_shapes():
        for n in TABLES:
            cases.append(("%dx%d->%dx%d rgb %d" % (src + dst + (n,)), rgb_mask(rng, src, table(n)[0]), dst, n))
        cases.append(("%dx%d->%dx%d ids" % (src + dst), id_mask(rng, src), dst, 8))
    want = [restate(m, dst, *table(n)) for _, m, dst, n in cases]
    for c in cases:
        c[1].setflags(write=False)
    return cases, want


def run(cases, n, **kw):
    """pseg_amd.label_masks over the cases of one table size, counts on."""
    import pseg_amd
    colors, ids = table(n)
    return pseg_amd.label_masks([c[1] for c in cases], [c[2] for c in cases], colors, ids, counts=True, **kw)


def by_table(cases):
    return {n: [k for k, c in enumerate(cases) if c[3] == n] for n in sorted({c[3] for c in cases})}


def assert_equal(cases, got, want):
    assert len(got) == len(want) == len(cases)
    for c, (lab, cnt), (rlab, rcnt) in zip(cases, got, want):
        assert lab.dtype == np.uint8 and lab.shape == tuple(c[2]) and cnt.dtype == np.int64 and cnt.shape == (257,), c[0]
        assert np.array_equal(lab, rlab), (c[0], int((lab != rlab).sum()))
        assert np.array_equal(cnt, rcnt), (c[0], np.flatnonzero(cnt != rcnt)[:8])
        assert cnt[:256].sum() == lab.size and cnt[256] <= cnt[0]


def mixed_list(seed=5, n=70):
    """n masks of about 40x30 with mixed shapes and both channel counts, for the 8-colour table -> [(name, mask, out_shape, 8)]."""
    rng = np.random.default_rng(seed)
    colors = table(8)[0]
    cases = []
    for k in range(n):
        src = (int(rng.integers(28, 50)), int(rng.integers(20, 40)))
        dst = (int(rng.integers(10, 60)), int(rng.integers(5, 45)))
        m = id_mask(rng, src) if k % 4 == 3 else rgb_mask(rng, src, colors)
        cases.append(("mixed %d" % k, m, dst, 8))
    return cases


def refusals(L, host):
    """Every refusal of pseg_label_masks_host (host=True) or pseg_label_masks on device 0: PSEG_EINVAL, a message that names the
    mask, and outputs that keep their fill."""
    import ctypes
    from pseg_amd import engine as E
    colors, ids = table(8)
    rng = np.random.default_rng(1)
    srcs = [rgb_mask(rng, (9, 7), colors), id_mask(rng, (5, 6)), rgb_mask(rng, (4, 4), colors)]
    shapes = [(5, 4), (7, 9), (3, 3)]
    n = len(srcs)
    outs = [np.full(s, 0xA5, np.uint8) for s in shapes]
    counts = np.full((n, 257), -3, np.int64)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n

    def call(tab=None, H=None, W=None, col=colors, idv=ids, nc=8, out=None, null=None):
        tab = tab if tab is not None else (E.MASK_SRC * n)(*[E.MASK_SRC(a.ctypes.data, a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1) for a in srcs])
        args = [n, tab, I(*(H or [s[0] for s in shapes])), I(*(W or [s[1] for s in shapes])), None if col is None else col.ctypes.data,
                None if idv is None else idv.ctypes.data, nc, out if out is not None else P(*[o.ctypes.data for o in outs]), counts.ctypes.data]
        if null is not None:
            args[null] = None
        rc = L.pseg_label_masks_host(*args) if host else L.pseg_label_masks(0, *args)
        msg = L.pseg_last_error().decode()
        assert rc == -1, (rc, msg)
        assert all((o == 0xA5).all() for o in outs) and (counts == -3).all(), msg
        return msg

    def src_table(k, **kw):
        f = [dict(px=a.ctypes.data, H0=a.shape[0], W0=a.shape[1], channels=3 if a.ndim == 3 else 1) for a in srcs]
        f[k].update(kw)
        return (E.MASK_SRC * n)(*[E.MASK_SRC(d["px"], d["H0"], d["W0"], d["channels"]) for d in f])

    for null in (1, 2, 3, 7):                                         # masks, H, W, out_labels
        assert "NULL" in call(null=null)
    assert "mask 1" in call(tab=src_table(1, px=None))
    assert "mask 2" in call(out=P(outs[0].ctypes.data, outs[1].ctypes.data, None))
    assert "mask 2" in call(tab=src_table(2, H0=0)) and "mask 0" in call(tab=src_table(0, W0=-1))
    assert "mask 1" in call(H=[5, 0, 3]) and "mask 2" in call(W=[4, 9, 0])
    for ch in (0, 2, 4):
        assert "mask 1" in call(tab=src_table(1, channels=ch))
    assert "colours" in call(nc=257) and "colours" in call(nc=-1)
    dup = colors.copy()
    dup[6] = dup[2]
    msg = call(col=dup)
    assert "colour 6" in msg and "colour 2" in msg
    assert "mask 0" in call(col=None) and "mask 0" in call(idv=None)
    return True
