"""pseg_skew_maps, pseg_rotate_maps and pseg_deskew_scans on the device: the list entries against the host twins and the NumPy
restatement of tests/skew_cases.py -- indices, whole score arrays and rotated bytes, array_equal throughout.  The grid and the
hand-made maps of the host test, shapes around every constant of the kernels, lists in groups, the combined entry with and without
ink maps, one large map, the refusals."""
import numpy as np
import pytest

import skew_cases as C
from test_skew_host import _how

pytestmark = pytest.mark.gpu


def _skew_list(gpu, cases, host=False):
    return gpu.skew_maps([c[1] for c in cases], [_how(c[2], c[3]) for c in cases], scores=True, host=host)


def _rotate_list(gpu, cases, host=False):
    outs = [None] * len(cases)
    groups = {}
    for k, c in enumerate(cases):                                      # one call per (denom, order, fill)
        groups.setdefault(c[3:], []).append(k)
    for (D, order, fill), ks in groups.items():
        got = gpu.rotate_maps([cases[k][1] for k in ks], [cases[k][2] for k in ks], denom=D, order=order, fill=fill, host=host)
        for k, o in zip(ks, got):
            outs[k] = o
    return outs


@pytest.fixture(scope="module")
def skew_cases(gpu):
    """The estimate's cases and, computed once: the restatement, the host twin, the device (one list call over all of them)."""
    assert gpu.engine.skew_geometry()[0] == C.STRIP
    cs = C.skew_grid() + C.hand_cases()
    rng = np.random.default_rng(41)
    for s in C.boundary_shapes():
        for A, D in ((16, 64), (89, 1024)):
            cs.append(("boundary %dx%d A=%d" % (s[0], s[1], A), C.random_ink(rng, s, 0.15), A, D))
    want = [C.restated_skew(c[1], c[2], c[3]) for c in cs]
    return cs, want, _skew_list(gpu, cs, host=True), _skew_list(gpu, cs)


def test_skew_device_equals_host_equals_restatement(gpu, skew_cases):
    cs, want, host, dev = skew_cases
    assert len(cs) > 260 and len(dev[0]) == len(cs) and dev[0].dtype == np.int32
    for k, (c, w) in enumerate(zip(cs, want)):
        assert host[0][k] == w[0] and np.array_equal(host[1][k], w[1]), ("host", c[0])
        assert dev[1][k].dtype == np.uint64 and np.array_equal(dev[1][k], w[1]), ("scores", c[0])
        assert dev[0][k] == w[0], ("index", c[0], dev[0][k], w[0])
    by = {c[0]: int(dev[0][k]) for k, c in enumerate(cs)}
    assert by["a tie between +a and -a only"] > 0 and by["a plateau of equal scores around 0"] == 0


def test_rotation_device_equals_host_equals_restatement(gpu):
    cs = C.rotate_grid()
    rng = np.random.default_rng(42)
    for s in C.boundary_shapes():
        src = rng.integers(0, 256, s).astype(np.uint8)
        for order in C.ORDERS:
            for a in (0, 3, -16):
                cs.append(("boundary %dx%d a=%d order=%d" % (s[0], s[1], a, order), src, a, 64, order, 7))
    host, dev = _rotate_list(gpu, cs, host=True), _rotate_list(gpu, cs)
    for c, h, d in zip(cs, host, dev):
        want = C.restated_rotate(*c[1:])
        assert np.array_equal(h, want), ("host", c[0])
        assert d.dtype == np.uint8 and d.shape == want.shape and np.array_equal(d, want), (c[0], int((d != want).sum()))
        if c[2] == 0:
            assert np.array_equal(d, c[1]), c[0]


def test_lists_and_groups(gpu, skew_cases):
    cs, want, _, _ = skew_cases
    rng = np.random.default_rng(5)
    small = [k for k, c in enumerate(cs) if c[1].size <= 1 << 16]
    pick = [small[int(j)] for j in rng.permutation(len(small))[:70]]   # 70 maps of mixed shapes and steps: two groups
    sub = [cs[k] for k in pick]
    assert len({c[1].shape for c in sub}) > 8 and len({(c[2], c[3]) for c in sub}) >= 4
    ref_i, ref_s = [want[k][0] for k in pick], [want[k][1] for k in pick]
    src = [rng.integers(0, 256, c[1].shape).astype(np.uint8) for c in sub]
    turn = [int(rng.integers(-c[2], c[2] + 1)) if c[3] == 64 else 0 for c in sub]
    ref_r = [C.restated_rotate(s, a, 64, 1, 9) for s, a in zip(src, turn)]

    def same(order=None, scores=True):
        idx = list(range(70)) if order is None else order
        got = _skew_list(gpu, [sub[k] for k in idx]) if scores else \
            (gpu.skew_maps([sub[k][1] for k in idx], [_how(sub[k][2], sub[k][3]) for k in idx]), None)
        ok = all(got[0][j] == ref_i[k] and (not scores or np.array_equal(got[1][j], ref_s[k])) for j, k in enumerate(idx))
        rot = gpu.rotate_maps([src[k] for k in idx], [turn[k] for k in idx], denom=64, order=1, fill=9)
        return ok and all(np.array_equal(rot[j], ref_r[k]) for j, k in enumerate(idx))

    for run in range(2):                                               # twice: the workspace is reused
        assert same(), run
    assert gpu.lib().pseg_release_workspace(0) == 0                     # the workspace goes and comes back
    assert same(scores=False)
    assert same([int(k) for k in rng.permutation(70)])
    for k in range(70):                                                # each alone
        i1, s1 = _skew_list(gpu, [sub[k]])
        assert i1[0] == ref_i[k] and np.array_equal(s1[0], ref_s[k]), sub[k][0]
        assert np.array_equal(gpu.rotate_maps([src[k]], turn[k], denom=64, order=1, fill=9)[0], ref_r[k]), sub[k][0]


def test_combined_entry(gpu):
    """deskew_scans equals skew_maps(gray <= 127) followed by rotate_maps(order=1, fill=255), with and without ink maps."""
    from pseg_amd import synth
    rng = np.random.default_rng(9)
    scans = [gpu.rotate_maps([(255 - synth.synth_page(i, 150, 210)[0]).astype(np.uint8)], a0, order=1, fill=255, host=True)[0]
             for i, a0 in enumerate((-40, 0, 23, 88))]
    scans += [rng.integers(0, 256, s).astype(np.uint8) for s in ((1, 1), (33, 65), (7, 300))]
    how = gpu.Skew()
    want_i = gpu.skew_maps([s <= 127 for s in scans], how)
    assert len(set(want_i.tolist())) >= 4
    want_r = [gpu.rotate_maps([s], int(a), order=1, fill=255)[0] for s, a in zip(scans, want_i)]
    outs, idx = gpu.deskew_scans(scans, how)
    assert np.array_equal(idx, want_i) and all(np.array_equal(o, w) for o, w in zip(outs, want_r))
    houts, hidx = gpu.deskew_scans(scans, how, host=True)
    assert np.array_equal(hidx, idx) and all(np.array_equal(o, w) for o, w in zip(houts, outs))
    # ink maps for some scans: the estimate is theirs, the rotation still the scan's
    inks = [None if k % 2 else C.random_ink(rng, s.shape, 0.1) for k, s in enumerate(scans)]
    ink_i = gpu.skew_maps([(s <= 127) if m is None else m for s, m in zip(scans, inks)], how)
    outs2, idx2 = gpu.deskew_scans(scans, how, inks=inks)
    assert np.array_equal(idx2, ink_i) and not np.array_equal(idx2, idx)
    assert all(np.array_equal(o, gpu.rotate_maps([s], int(a), order=1, fill=255)[0]) for o, s, a in zip(outs2, scans, idx2))
    houts2, hidx2 = gpu.deskew_scans(scans, how, inks=inks, host=True)
    assert np.array_equal(hidx2, idx2) and all(np.array_equal(o, w) for o, w in zip(houts2, outs2))
    # 70 scans: two groups
    many = [scans[k % len(scans)] for k in range(70)]
    outs3, idx3 = gpu.deskew_scans(many, how)
    assert all(idx3[k] == idx[k % len(scans)] and np.array_equal(outs3[k], outs[k % len(scans)]) for k in range(70))


def test_one_large_map(gpu):
    from pseg_amd import synth
    scan = gpu.rotate_maps([(255 - synth.synth_page(1, 2048, 1536)[0]).astype(np.uint8)], -37, order=1, fill=255, host=True)[0]
    how = gpu.Skew()
    (hi,), (hs,) = gpu.skew_maps([scan <= 127], how, scores=True, host=True)
    (di,), (ds,) = gpu.skew_maps([scan <= 127], how, scores=True)
    assert di == hi and np.array_equal(ds, hs) and di != 0
    (out,), idx = gpu.deskew_scans([scan], how)
    assert idx[0] == hi and np.array_equal(out, C.restated_rotate(scan, int(hi), 1024, 1, 255))
    assert np.array_equal(gpu.rotate_maps([scan], 256, order=0, fill=3)[0], C.restated_rotate(scan, 256, 1024, 0, 3))


def test_refusals_on_the_device_entries(gpu):
    C.refusals(gpu.lib(), False)
    outs, idx = gpu.deskew_scans([], gpu.Skew())
    assert outs == [] and len(idx) == 0 and len(gpu.skew_maps([], gpu.Skew())) == 0 and gpu.rotate_maps([], []) == []
