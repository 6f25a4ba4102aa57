"""What the polygon tests of the text regions share (tests/test_regions_poly_host.py, tests/test_regions_poly_gpu.py): the yardstick --
pseg_text_regions_host + pseg_trace_regions_host, the pixel walk over a byte mask -- computed once per case list, the raw C call with
sentinel-filled outputs, and hand-made maps on which a walk that takes its horizontal stretches a word at a time can go wrong."""
import ctypes

import numpy as np

import regions_cases as C

SENTINEL = -9
_YARD = {}


def how_of(cases):
    import pseg_amd
    return [pseg_amd.TextRegions(c[2], kernels=c[3]) for c in cases]


def yardstick(cases, key):
    """One record per case: the host entry's mask, boxes, areas and seeds, and "polygons" from the pixel walk.  Cached under key and
    never changed."""
    if key not in _YARD:
        import pseg_amd
        recs = pseg_amd.text_regions([c[1] for c in cases], how_of(cases), host=True, max_regions=256)
        for rec in recs:
            rec["polygons"] = pseg_amd.trace_regions(rec["mask"], rec)
            for a in [rec["mask"], rec["boxes"], rec["areas"], rec["seeds"]] + rec["polygons"]:
                a.setflags(write=False)
        _YARD[key] = recs
    return _YARD[key]


def assert_records_equal(cases, got, want, masks=True):
    assert len(got) == len(want) == len(cases)
    for c, g, w in zip(cases, got, want):
        if masks:
            assert np.array_equal(g["mask"], w["mask"]), c[0]
        for k in ("boxes", "areas", "seeds"):
            assert g[k].dtype == np.int32 and np.array_equal(g[k], w[k]), (c[0], k)
        assert len(g["polygons"]) == len(w["polygons"]) == len(w["boxes"]), c[0]
        for r, (p, q) in enumerate(zip(g["polygons"], w["polygons"])):
            assert p.dtype == np.int32 and p.shape == q.shape and np.array_equal(p, q), (c[0], r, p[:6], q[:6])


def raw(maps, hows, max_regions, cap, device=None, masks=False, drop=()):
    """The C entry itself (device None: the host twin) with every output filled with SENTINEL (masks: 0xA5) beforehand.  drop: names of
    pointers passed as NULL ("first", "status", "xy").  -> dict rc, msg, masks, rows, cnt, xy, first, status."""
    from pseg_amd import engine as E
    n = len(maps)
    ms = [np.ascontiguousarray(m, np.uint8) for m in maps]
    table = (E.REGIONS * n)(*[E.REGIONS(e.label, *e.kernels) for e in hows])
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    out = {"masks": [np.full(m.shape, 0xA5, np.uint8) for m in ms] if masks else None,
           "rows": np.full((n, max(max_regions, 0), 8), SENTINEL, np.int32), "cnt": np.full(n, SENTINEL, np.int32),
           "xy": np.full((max(cap, 0), 2), SENTINEL, np.int32), "first": np.full((n, max(max_regions, 0) + 1), SENTINEL, np.int64),
           "status": np.full(n, SENTINEL, np.int32)}
    args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
            P(*[a.ctypes.data for a in out["masks"]]) if masks else None, int(max_regions), out["rows"].ctypes.data if max_regions > 0 else None,
            out["cnt"].ctypes.data, None if "xy" in drop or cap <= 0 else out["xy"].ctypes.data, int(cap),
            None if "first" in drop else out["first"].ctypes.data, None if "status" in drop else out["status"].ctypes.data)
    out["rc"] = E.lib().pseg_text_regions_poly_host(*args) if device is None else E.lib().pseg_text_regions_poly(int(device), *args)
    out["msg"] = E.lib().pseg_last_error().decode()
    return out


def untouched(out):
    return all((out[k] == SENTINEL).all() for k in ("rows", "cnt", "xy", "first", "status")) and \
        (out["masks"] is None or all((a == 0xA5).all() for a in out["masks"]))


def word_cases():
    """(name, label map, 1, (1, 1, 1)): maps whose regions' horizontal stretches end at the bits a word scan has to get right."""
    out = []
    ident = (1, 1, 1)

    def blank(H, W):
        return np.zeros((H, W), np.uint8)
    for x1 in (1, 63, 64, 65, 128):                # runs from column 0 that end exactly at bit 0, 62/63, 63/64 and at two words
        m = blank(5, 200)
        m[1:3, 0:x1] = 1
        out.append(("run 0..%d" % x1, m, 1, ident))
    for x0 in (63, 64, 65):                        # runs that start at a word seam
        m = blank(5, 200)
        m[1:3, x0:150] = 1
        out.append(("run %d..150" % x0, m, 1, ident))
    for W in (70, 64, 65, 127, 129):               # runs that end at the map's last column, W % 64 != 0 among them
        m = blank(4, W)
        m[1:3, 3:W] = 1
        out.append(("run to the last column of %d" % W, m, 1, ident))
    m = blank(6, 260)                              # a run across three words and more, with a notch above it that ends its left side
    m[2:4, 10:250] = 1
    m[1, 100:130] = 1
    out.append(("three words", m, 1, ident))
    m = blank(80, 140)                             # a staircase of one-pixel steps down to the right and back
    for i in range(70):
        m[5 + i, 2:4 + i] = 1
    out.append(("staircase right", m, 1, ident))
    m = blank(80, 140)
    for i in range(70):
        m[5 + i, 139 - i:140] = 1
    out.append(("staircase left", m, 1, ident))
    m = blank(10, 140)                             # pixels that meet only diagonally at a word seam: two regions, neither walk crosses
    m[2:5, 60:64] = 1
    m[5:8, 64:70] = 1
    out.append(("diagonal at a word seam", m, 1, ident))
    m = blank(70, 140)                             # ... and at the corner of four tiles
    m[20:32, 50:64] = 1
    m[32:40, 64:80] = 1
    m[20:32, 64:80] = 0
    out.append(("diagonal at a four-tile corner", m, 1, ident))
    m = blank(70, 140)                             # the other diagonal
    m[20:32, 64:80] = 1
    m[32:40, 50:64] = 1
    out.append(("anti-diagonal at a four-tile corner", m, 1, ident))
    out.append(("the whole map", np.ones((33, 130), np.uint8), 1, ident))
    out.append(("the whole map, one word", np.ones((32, 64), np.uint8), 1, ident))
    m = blank(50, 200)                             # a ring: the hole is filled, the outer boundary alone is traced
    m[5:45, 10:190] = 1
    m[15:35, 30:170] = 0
    out.append(("ring", m, 1, ident))
    m = blank(50, 200)                             # a ring cut open
    m[5:45, 10:190] = 1
    m[15:35, 30:170] = 0
    m[25, 10:30] = 0                               # a channel from the hole to the outside: the inside is background, the outer boundary has a slit
    out.append(("ring with a slit", m, 1, ident))
    out.append(("one row", np.array([[1, 1, 0, 1] * 40 + [1] * 70], np.uint8), 1, ident))
    out.append(("one column", np.array([[1, 1, 0, 1] * 40 + [1] * 70], np.uint8).T.copy(), 1, ident))
    m = blank(9, 131)                              # a comb: every other column, teeth up and down, across two seams
    m[4, :] = 1
    m[1:4, ::2] = 1
    m[5:8, 1::2] = 1
    out.append(("comb", m, 1, ident))
    rng = np.random.default_rng(5)                 # salt: every run length and every turn
    out.append(("salt", (rng.random((67, 197)) < 0.6).astype(np.uint8), 1, ident))
    return out
