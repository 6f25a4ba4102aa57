"""pseg_despeckle_maps on the device: the list entry against the host entry and the scipy.ndimage restatement of
tests/despeckle_cases.py, maps and counts, array_equal throughout.  The grid of the host test, shapes around one and two tiles in
each axis, and the maps on which a tile scheme can go wrong: components split by tile edges and corners, diagonal-only contacts, a
rim that saturates the root slots, blobs larger than a tile, lists in groups, one large map.  The kernels' constants come from
pseg_despeckle_geometry."""
import numpy as np
import pytest

import despeckle_cases as C

pytestmark = pytest.mark.gpu


def _geom():
    from pseg_amd import engine as E
    return E.despeckle_geometry()


def _how(gpu, cases):
    return [None if c[2] == 0 else gpu.Despeckle(c[2], c[3]) for c in cases]


def _tile_shapes():
    th, tw, _, _ = _geom()
    return [(H, W) for H in (th - 1, th, th + 1, 2 * th - 1, 2 * th, 2 * th + 1) for W in (tw - 1, tw, tw + 1, 2 * tw - 1, 2 * tw, 2 * tw + 1)]


def _tile_cases():
    """[(name, ink, max_area, connectivity, expected counts or None)] placed by the tile size."""
    th, tw, slots, _ = _geom()
    out = []
    H, W = 3 * th, 3 * tw
    for a in (2, 6, 31):
        for c in C.CONNECTIVITIES:
            # a bar across the vertical edge x = tw and one across the horizontal edge y = th; one of a pixels (erased), one of a + 1 (kept)
            m = np.zeros((H, W), np.uint8)
            m[5, tw - a // 2:tw - a // 2 + a] = 1
            m[9, tw - a // 2:tw - a // 2 + a + 1] = 1
            m[th - (a + 1) // 2:th - (a + 1) // 2 + a, 7] = 1
            m[th - (a + 1) // 2:th - (a + 1) // 2 + a + 1, 11] = 1
            out.append(("bars across an edge a=%d c=%d" % (a, c), m, a, c, [2, 2 * a, 2]))
    for c in C.CONNECTIVITIES:
        # across the corner (th, tw) of four tiles: a 2 x 2 block with one arm into each tile, 12 pixels, each part 3
        for y0, x0, a, want in ((th, tw, 12, [1, 12, 0]), (th, tw, 11, [0, 0, 1]), (2 * th, 2 * tw, 12, [1, 12, 0]), (2 * th, tw, 11, [0, 0, 1])):
            m = np.zeros((H, W), np.uint8)
            m[y0 - 1:y0 + 1, x0 - 1:x0 + 1] = 1
            m[y0 - 3:y0 - 1, x0 - 1] = 1
            m[y0 - 1, x0:x0 + 3] = 1
            m[y0, x0 - 3:x0] = 1
            m[y0:y0 + 3, x0] = 1
            assert int(m.sum()) == 12
            out.append(("four-tile corner (%d,%d) a=%d c=%d" % (y0, x0, a, c), m, a, c, want))
    # contact by a diagonal only: at a four-tile corner (both diagonals) and along a vertical and a horizontal edge
    m = np.zeros((H, W), np.uint8)
    m[th - 1, tw - 1] = m[th, tw] = 1
    m[th - 1, 2 * tw] = m[th, 2 * tw - 1] = 1
    m[5, tw - 1] = m[6, tw] = 1
    m[2 * th - 1, 9] = m[2 * th, 10] = 1
    m[2 * th, 40] = m[2 * th - 1, 41] = 1
    for a, c, want in ((1, 8, [0, 0, 5]), (2, 8, [5, 10, 0]), (1, 4, [10, 10, 0])):
        out.append(("diagonal contacts a=%d c=%d" % (a, c), m, a, c, want))
    # the rim of the middle tile carries ink on every second pixel, each with a partner across the edge: at connectivity 4 every one
    # of them is an open root of its own
    m = np.zeros((H, W), np.uint8)
    for x in range(tw, 2 * tw, 2):
        m[th - 1:th + 1, x] = 1
        m[2 * th - 1:2 * th + 1, x + 1] = 1
    for y in range(th + 2, 2 * th - 2, 2):
        m[y, tw - 1:tw + 1] = 1
        m[y + 1, 2 * tw - 1:2 * tw + 1] = 1
    n_pairs = int(m.sum()) // 2
    assert n_pairs >= (th + tw) - 6 and n_pairs <= slots
    out.append(("saturated rim a=1 c=4", m, 1, 4, [0, 0, n_pairs]))
    out.append(("saturated rim a=2 c=4", m, 2, 4, [n_pairs, 2 * n_pairs, 0]))
    out.append(("saturated rim a=2 c=8", m, 2, 8, None))
    # every second pixel of the whole rim and of the ring around it, all of the map beyond: one large component at the door of every slot
    m = np.ones((H, W), np.uint8)
    m[th - 1:2 * th + 1, tw - 1:2 * tw + 1] = 0
    m[th:2 * th, tw:2 * tw] = 0
    m[th, tw:2 * tw:2] = 1
    m[2 * th - 1, tw:2 * tw:2] = 1
    m[th:2 * th:2, tw] = 1
    m[th:2 * th:2, 2 * tw - 1] = 1
    m[th - 1, tw:2 * tw:2] = 1
    m[2 * th, tw:2 * tw:2] = 1
    m[th:2 * th:2, tw - 1] = 1
    m[th:2 * th:2, 2 * tw] = 1
    for c in C.CONNECTIVITIES:
        out.append(("rim into the surrounding ink c=%d" % c, m, 3, c, None))
    # max_area above a tile's pixel count, a blob over several tiles just below and just above it
    px = th * tw
    m = np.zeros((3 * th, 4 * tw), np.uint8)
    m[th // 2:th // 2 + 2 * th, tw // 2:tw // 2 + tw + 9] = 1
    s = int(m.sum())
    assert s > px + 1
    for c in C.CONNECTIVITIES:
        out.append(("blob of %d, a=%d c=%d" % (s, s, c), m, s, c, [1, s, 0]))
        out.append(("blob of %d, a=%d c=%d" % (s, s - 1, c), m, s - 1, c, [0, 0, 1]))
    sp = C.serpentine(2 * th + 5, 2 * tw + 13)
    out.append(("serpentine over tiles, kept", sp, int(sp.sum()) - 1, 4, [0, 0, 1]))
    out.append(("serpentine over tiles, erased", sp, int(sp.sum()), 4, [1, int(sp.sum()), 0]))
    return out


@pytest.fixture(scope="module")
def cases(gpu):
    """The cases and, computed once: the restatement, the host entry, the device entry (one list call over all of them)."""
    cs = C.grid_cases() + C.grid_cases(seed=99, shapes=_tile_shapes()) + [c[:4] for c in C.hand_cases()] + [c[:4] for c in _tile_cases()]
    maps, how = [c[1] for c in cs], _how(gpu, cs)
    want = [C.restated(c[1], c[2], c[3]) for c in cs]
    host = gpu.despeckle_maps(maps, how, host=True, counts=True)
    dev = gpu.despeckle_maps(maps, how, counts=True)
    return cs, want, host, dev


def test_device_equals_host_equals_restatement(gpu, cases):
    cs, want, host, dev = cases
    assert len(cs) > 1800 and len(dev[0]) == len(cs)
    for k, (c, w) in enumerate(zip(cs, want)):
        assert np.array_equal(host[0][k], w[0]) and np.array_equal(host[1][k], w[1]), ("host", c[0])
        d = dev[0][k]
        assert d.dtype == np.uint8 and d.shape == c[1].shape, c[0]
        assert np.array_equal(d, w[0]), ("map", c[0], int((d != w[0]).sum()))
        assert np.array_equal(dev[1][k], w[1]), ("counts", c[0], dev[1][k], w[1])


def test_tile_cases_have_the_known_counts(gpu):
    cs = _tile_cases() + C.hand_cases()
    outs, cnt = gpu.despeckle_maps([c[1] for c in cs], _how(gpu, cs), counts=True)
    known = 0
    for k, c in enumerate(cs):
        want, wc = C.restated(c[1], c[2], c[3])
        assert np.array_equal(outs[k], want) and np.array_equal(cnt[k], wc), c[0]
        if c[4] is not None:
            assert list(cnt[k]) == c[4], (c[0], cnt[k])
            known += 1
    assert known >= 40
    # idempotent on the device as well
    again, cnt2 = gpu.despeckle_maps(outs, _how(gpu, cs), counts=True)
    for k, c in enumerate(cs):
        assert np.array_equal(again[k], outs[k]) and list(cnt2[k]) == [0, 0, cnt[k][2]], c[0]


def test_lists_and_groups(gpu, cases):
    cs, want, _, _ = cases
    rng = np.random.default_rng(5)
    # 70 maps: two groups; mixed shapes, thresholds and connectivities, entries that are not despeckled among them
    pick = [int(k) for k in rng.permutation(len(cs))[:70]]
    sub = [cs[k] if j % 5 else (cs[k][0], (cs[k][1] * 200).astype(np.uint8), 0, 8) for j, k in enumerate(pick)]
    ref = [want[k] if j % 5 else (sub[j][1], np.zeros(3, np.int64)) for j, k in enumerate(pick)]
    assert len({c[2] for c in sub}) >= 4 and {c[3] for c in sub if c[2]} == {4, 8} and len({c[1].shape for c in sub}) > 8
    maps, how = [c[1] for c in sub], _how(gpu, sub)

    def same(got, order=None):
        outs, cnt = got
        idx = range(len(outs)) if order is None else order
        return all(np.array_equal(outs[j], ref[k][0]) and np.array_equal(cnt[j], ref[k][1]) for j, k in enumerate(idx))

    for run in range(2):                                       # twice: the workspace is reused
        assert same(gpu.despeckle_maps(maps, how, counts=True)), run
    assert gpu.lib().pseg_release_workspace(0) == 0             # the workspace goes and comes back
    # without counts; in another order; each map alone
    assert all(np.array_equal(g, r[0]) for g, r in zip(gpu.despeckle_maps(maps, how), ref))
    order = [int(k) for k in rng.permutation(70)]
    assert same(gpu.despeckle_maps([maps[k] for k in order], [how[k] for k in order], counts=True), order)
    for k in range(70):
        outs, cnt = gpu.despeckle_maps([maps[k]], [how[k]], counts=True)
        assert np.array_equal(outs[0], ref[k][0]) and np.array_equal(cnt[0], ref[k][1]), sub[k][0]
    C.refusals(gpu.lib(), False)
    assert gpu.despeckle_maps([], gpu.Despeckle(2)) == []
    # a list of maps that are not despeckled touches no kernel and hands the bytes back
    assert all(np.array_equal(a, b) for a, b in zip(gpu.despeckle_maps(maps[:3], None), maps[:3]))


def test_one_large_map(gpu):
    rng = np.random.default_rng(8)
    m = C.random_map(rng, (2048, 1536), 0.3)
    for a, conn in ((9, 8), (3, 4)):
        want, wc = C.restated(m, a, conn)
        (out,), cnt = gpu.despeckle_maps([m], gpu.Despeckle(a, conn), counts=True)
        assert np.array_equal(out, want), int((out != want).sum())
        assert np.array_equal(cnt[0], wc) and wc[0] > 1000 and wc[2] > 100
