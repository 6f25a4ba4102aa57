"""Training masks as label maps without a GPU: pseg_label_masks_host -- the coordinate and lookup functions the device kernel is
compiled from -- against oracle.resize.resize_nearest(ColorMap.to_labels(rgb), shape) and NumPy counts (tests/labelmasks_cases.py),
integer array_equal throughout; every refusal; ColorMap.table(); the arguments of the Python entry; the group cut."""
import ctypes

import numpy as np
import pytest

import labelmasks_cases as C


def test_symbols_and_geometry():
    from pseg_amd import engine as E
    for sym in ("pseg_label_masks", "pseg_label_masks_host", "pseg_label_masks_geometry", "pseg_label_masks_groups"):
        assert sym in E.EXPORTED_SYMBOLS and hasattr(E.lib(), sym)
    run, runs, rows, gm, gb = E.label_masks_geometry()
    assert run >= 4 and runs >= 1 and rows >= 1 and run * runs * rows >= 64 and (gm, gb) == (64, 64 << 20)
    assert ctypes.sizeof(E.MASK_SRC) == 24


def test_host_entry_equals_the_restatement_over_the_grid():
    cases, want = C.grid()
    assert len(cases) == (len(C.SHAPES) + 9) * (len(C.TABLES) + 1)
    for n, ks in C.by_table(cases).items():
        sub = [cases[k] for k in ks]
        got = C.run(sub, n, host=True)
        C.assert_equal(sub, got, [want[k] for k in ks])
        # counts off: the same label maps
        import pseg_amd
        plain = pseg_amd.label_masks([c[1] for c in sub], [c[2] for c in sub], *C.table(n), host=True)
        assert all(np.array_equal(a, b[0]) for a, b in zip(plain, got))
        # every mask alone
        for c, g in list(zip(sub, got))[::5]:
            C.assert_equal([c], C.run([c], n, host=True), [g])
    # the grid is not a grid of trivial maps: unknown colours, several ids, and both kinds of source
    assert sum(w[1][256] > 0 for w in want) > len(cases) // 3
    assert sum((w[1][:256] > 0).sum() >= 3 for w in want) > len(cases) // 3
    assert any(c[1].ndim == 2 for c in cases)


def test_the_table_rules():
    """Black with a non-zero id next to unknown colours; a colour with id 0 that is no unknown; neighbours one step apart; ids in no
    order; no colours at all."""
    import pseg_amd
    colors, ids = C.table(8)
    assert tuple(colors[0]) == (0, 0, 0) and ids[0] == 5 and ids[1] == 0 and list(ids) != sorted(ids)
    assert any(np.abs(colors[a].astype(int) - colors[b].astype(int)).sum() == 1 for a in range(8) for b in range(a))
    px = np.array([[(0, 0, 0), (255, 0, 0), (255, 0, 1), (254, 0, 0), (253, 0, 0), (0, 0, 2), (255, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 0)]], np.uint8)
    lab, cnt = pseg_amd.label_masks([px], [(1, 10)], colors, ids, counts=True, host=True)[0]
    assert lab.tolist() == [[5, 0, 3, 200, 0, 0, 1, 0, 255, 77]]
    assert cnt[256] == 3 and cnt[0] == 4 and cnt[5] == 1 and cnt[200] == 1 and cnt[:256].sum() == 10
    rlab, rcnt = C.restate(px, (1, 10), colors, ids)
    assert np.array_equal(lab, rlab) and np.array_equal(cnt, rcnt)
    # no colours: every pixel is unknown, with and without the table's arrays
    none = np.zeros((0, 3), np.uint8), np.zeros((0,), np.uint8)
    lab, cnt = pseg_amd.label_masks([px], [(2, 5)], *none, counts=True, host=True)[0]
    assert not lab.any() and cnt[0] == cnt[256] == 10
    lab, cnt = pseg_amd.label_masks([px], [(2, 5)], [], [], counts=True, host=True)[0]
    assert not lab.any() and cnt[0] == cnt[256] == 10


def test_one_channel_sources_keep_every_byte_value():
    import pseg_amd
    ids = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for colors in (C.table(256), C.table(0)):
        lab, cnt = pseg_amd.label_masks([ids], [(16, 16)], *colors, counts=True, host=True)[0]
        assert np.array_equal(lab, ids) and (cnt[:256] == 1).all() and cnt[256] == 0
    lab, cnt = pseg_amd.label_masks([ids], [(48, 32)], *C.table(3), counts=True, host=True)[0]
    rlab, rcnt = C.restate(ids, (48, 32), *C.table(3))
    assert np.array_equal(lab, rlab) and np.array_equal(cnt, rcnt) and (cnt[:256] == 6).all()
    # a mask of bools that were viewed as bytes
    b = (ids > 100).view(np.uint8)
    assert np.array_equal(pseg_amd.label_masks([b], [(5, 7)], [], [], host=True)[0], C.restate(b, (5, 7), *C.table(0))[0])


def test_refusals_leave_the_outputs_untouched():
    import pseg_amd
    assert C.refusals(pseg_amd.lib(), True)


def test_no_masks_is_no_work():
    import pseg_amd
    L = pseg_amd.lib()
    assert pseg_amd.label_masks([], [], *C.table(3), host=True) == [] and pseg_amd.label_masks([], [], *C.table(3)) == []
    assert L.pseg_label_masks(0, 0, None, None, None, None, None, 0, None, None) == 0           # before a device is touched
    assert L.pseg_label_masks_host(0, None, None, None, None, None, 0, None, None) == 0


def test_group_cut():
    """64 masks, or 64 MiB of source bytes -- three bytes a pixel for an RGB mask, one for an id map; only the shapes are read."""
    import pseg_amd
    small = [np.zeros((3, 4, 3), np.uint8)] * 70
    assert pseg_amd.label_mask_groups(small) == [0] * 64 + [1] * 6
    rgb = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (4096, 2048, 3), (0, 0, 1))   # 24 MiB, were it dense: two fit, three do not
    ids = np.lib.stride_tricks.as_strided(np.zeros(1, np.uint8), (4096, 2048), (0, 0))         # 8 MiB
    L, E = pseg_amd.lib(), pseg_amd.engine

    def groups(shapes):
        tab = (E.MASK_SRC * len(shapes))(*[E.MASK_SRC(None, a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1) for a in shapes])
        out = (ctypes.c_int * len(shapes))()
        assert L.pseg_label_masks_groups(len(shapes), tab, out) == 0
        return list(out)
    assert groups([rgb, rgb, rgb]) == [0, 0, 1]
    assert groups([rgb, rgb, ids, ids, ids, rgb]) == [0, 0, 0, 0, 1, 1]
    assert groups([ids] * 9) == [0] * 8 + [1]
    big = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (8192, 4096, 3), (0, 0, 1))    # 96 MiB: a group of its own
    assert groups([ids, big, ids]) == [0, 1, 2]
    assert pseg_amd.label_mask_groups([]) == []


def test_color_map_table():
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    cm = ColorMap({(255, 255, 255): (0, "bg"), (0, 0, 255): (2, "img"), "(255, 0, 0)": (1, "text"), (0, 0, 0): (7, "ink")})
    colors, ids = cm.table()
    assert colors.dtype == ids.dtype == np.uint8 and colors.shape == (4, 3) and ids.shape == (4,)
    assert colors.tolist() == [[255, 255, 255], [0, 0, 255], [255, 0, 0], [0, 0, 0]] and ids.tolist() == [0, 2, 1, 7]     # mapping order
    colors, ids = ColorMap({}).table()
    assert colors.shape == (0, 3) and ids.shape == (0,) and colors.dtype == ids.dtype == np.uint8
    with pytest.raises(Exception, match="256"):
        ColorMap({(1, 2, 3): (256, "too large")}).table()
    with pytest.raises(Exception, match="-1"):
        ColorMap({(1, 2, 3): (-1, "negative")}).table()
    with pytest.raises(Exception, match="300"):
        ColorMap({(300, 2, 3): (1, "no colour")}).table()
    # the table gives what to_labels gives
    import pseg_amd
    rng = np.random.default_rng(0)
    rgb = C.rgb_mask(rng, (30, 40), cm.table()[0])
    assert np.array_equal(pseg_amd.label_masks([rgb], [(30, 40)], *cm.table(), host=True)[0], cm.to_labels(rgb))


def test_wrapper_argument_errors():
    import pseg_amd
    Err = pseg_amd.PsegError
    colors, ids = C.table(3)
    ok = np.zeros((4, 5, 3), np.uint8)

    def call(masks, shapes=None, col=colors, idv=ids):
        return pseg_amd.label_masks(masks, shapes if shapes is not None else [(2, 2)] * len(masks), col, idv, host=True)
    with pytest.raises(Err, match="mask 1.*shape"):
        call([ok, np.zeros((4,), np.uint8)])                                  # rank
    with pytest.raises(Err, match="mask 0.*shape"):
        call([np.zeros((2, 3, 4, 3), np.uint8)])
    with pytest.raises(Err, match="mask 1.*shape"):
        call([ok, np.zeros((4, 5, 2), np.uint8)])
    with pytest.raises(Err, match="mask 2.*dtype"):
        call([ok, ok, np.zeros((4, 5, 3), np.int64)])
    with pytest.raises(Err, match="mask 1.*dtype"):
        call([ok, np.zeros((4, 5), np.float32)])
    with pytest.raises(Err, match="mask 1.*alpha"):
        call([ok, np.zeros((4, 5, 4), np.uint8)])                             # RGBA
    with pytest.raises(Err, match="0..255"):
        call([ok], idv=[0, 256, 3])
    with pytest.raises(Err, match="0..255"):
        call([ok], idv=[0, -1, 3])
    with pytest.raises(Err, match="at most 256"):
        call([ok], col=np.zeros((257, 3), np.uint8), idv=np.zeros(257, np.uint8))
    with pytest.raises(Err, match="colour 2 repeats colour 0"):
        call([ok], col=[(1, 2, 3), (3, 2, 1), (1, 2, 3)], idv=[1, 2, 3])
    with pytest.raises(Err, match="shapes"):
        call([ok], col=colors, idv=ids[:2])
    with pytest.raises(Err, match="one entry per mask"):
        call([ok, ok], shapes=[(2, 2)])
    with pytest.raises(Err, match="mask 1.*empty"):
        call([ok, ok], shapes=[(2, 2), (0, 3)])
    # refused before anything was made, also for an empty list
    with pytest.raises(Err, match="repeats"):
        pseg_amd.label_masks([], [], [(1, 2, 3), (1, 2, 3)], [1, 2], host=True)
