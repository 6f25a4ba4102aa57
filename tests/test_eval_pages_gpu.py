"""A list of pages scored in one device call (pseg_eval_pages) against the NumPy / scipy restatement of the
reference's per-page evaluation: the joint histogram from np.add.at, the component verdicts from oracle.evaluation's
run_per_component summed.  Every comparison is an integer array_equal."""
import ctypes
import dataclasses

import numpy as np
import pytest

from oracle import evaluation as O

pytestmark = pytest.mark.gpu

_CC_MEMO = {}
_cc_with_stats = O.connected_components_with_stats


@pytest.fixture(autouse=True)
def _label_once(monkeypatch):
    """run_per_component labels the page anew for every rule: keep the restatement's labelling per (binarisation, connectivity)."""
    def memo(binary, connectivity=4):
        b = np.ascontiguousarray(binary)
        key = (b.shape, b.tobytes(), connectivity)
        if key not in _CC_MEMO:
            _CC_MEMO[key] = _cc_with_stats(b, connectivity)
        return _CC_MEMO[key]
    monkeypatch.setattr(O, "connected_components_with_stats", memo)


def _page(seed, H, W, C, specks=0.08):
    """tests/test_eval_gpu.py's pages: synth layout, 7 % flipped labels, 8 % specks of ink."""
    from pseg_amd import synth
    img, binary, mask = synth.synth_page(seed, max(H, 96), max(W, 96), C)
    binary, mask = np.ascontiguousarray(binary[:H, :W]), np.ascontiguousarray(mask[:H, :W])
    rng = np.random.default_rng(seed)
    pred = mask.astype(np.int64)
    flip = rng.random(mask.shape) < 0.07
    pred[flip] = rng.integers(0, C, int(flip.sum()))
    binary = (binary | (rng.random((H, W)) < specks)).astype(np.uint8)
    return binary, mask.astype(np.uint8), pred.astype(np.uint8)


# a rule: ("m", (label, tp, fp[, mask])) or ("e", (threshold,)), then the only_label filter or None
RULES = [("m", (1, .5, .1), None), ("m", (2, .5, .1, .3), None), ("e", (.9,), None), ("e", (.5,), (2, .5))]


def _lib_rules(rules):
    from ocr4all_pixel_classifier.lib import evaluation as E
    out = []
    for kind, args, flt in rules:
        obj = E.cc_matching(*args) if kind == "m" else E.cc_equal(*args)
        out.append(obj if flt is None else (obj, flt))
    return out


def _want_page(mask, pred, binary, rules, conn, ncls):
    """(counts, components, verdicts) of one page from the restatement."""
    counts = np.zeros((2, ncls + 1, ncls + 1), np.int64)
    b = np.ones(mask.shape, int) if binary is None else (binary != 0).astype(int)
    np.add.at(counts, (b, mask.astype(int), pred.astype(int)), 1)
    ver = np.zeros((len(rules), 4), np.int64)
    if binary is None:
        return counts, 0, ver
    m, p = mask.astype(np.int64), pred.astype(np.int64)
    comps = len(O.run_per_component(m, p, binary, lambda a, c: 0, conn))
    for k, (kind, args, flt) in enumerate(rules):
        f = O.cc_matching(*args) if kind == "m" else O.cc_equal(*args)
        res = O.run_per_component(m, p, binary, f, conn, flt[0] if flt else None, flt[1] if flt else None)
        if kind == "m":
            ver[k, :3] = np.sum(res, axis=0) if res else 0
        else:
            t = sum(bool(x) for x in res)
            ver[k, :3] = (t, len(res) - t, 0)
        ver[k, 3] = len(res)
    return counts, comps, ver


def _check(gpu, pages, rules, conn, ncls=None):
    """pages: (binary or None, mask, pred).  One evaluate_pages call against the restatement; returns the raw arrays."""
    from ocr4all_pixel_classifier.lib import evaluation as E
    if ncls is None:
        ncls = max([int(max(m.max(initial=0), p.max(initial=0))) for _, m, p in pages] + [max(a[0] if k == "m" else 0, f[0] if f else 0) for k, a, f in rules] + [0]) + 1
    scores = E.evaluate_pages([m for _, m, _ in pages], [p for _, _, p in pages], [b for b, _, _ in pages], _lib_rules(rules), conn)
    assert len(scores) == len(pages)
    for k, ((b, m, p), s) in enumerate(zip(pages, scores)):
        counts, comps, ver = _want_page(m, p, b, rules, conn, ncls)
        assert np.array_equal(s.counts, counts), (k, conn)
        assert s.num_components == comps, (k, conn, s.num_components, comps)
        assert np.array_equal(s.verdicts, ver), (k, conn, s.verdicts, ver)
        assert all(s.cc(i) == tuple(ver[i]) for i in range(len(rules)))
    return scores


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (70, 1), (31, 63), (32, 64), (33, 65), (65, 129), (257, 131), (160, 192)])
def test_shapes_at_the_tile_grid(gpu, shape, C):
    binary, mask, pred = _page(11, shape[0], shape[1], C)
    rules = RULES + [("e", (.5,), (C + 1, .5)), ("m", (1, .5, .1), (C + 1, 0.))]      # a filter label that never occurs: only threshold 0 keeps anything
    for conn in (4, 8):
        _check(gpu, [(binary, mask, pred)], rules, conn)


def test_thresholds_exactly_on_a_quotient(gpu):
    binary = np.zeros((40, 70), np.uint8)
    mask, pred = np.zeros((40, 70), np.uint8), np.zeros((40, 70), np.uint8)
    binary[3, 5:9] = 1                                                  # s = 4
    pred[3, 5:7] = 1                                                    # P[1] = 2: 2 / 4 >= 0.5
    mask[3, 5:8] = 1                                                    # M[1] = 3: 3 / 4 >= 0.75
    binary[30:33, 60:66] = 1                                            # s = 18, across a tile corner
    pred[30, 60:66] = 1                                                 # P[1] = 6: 6 / 18 against the doubles 1 / 3 and 6 / 18
    rules = [("m", (1, .5, .5, .75), None), ("m", (1, .5000000000000001, .5, .75), None), ("m", (1, .5, .5, .7500000000000001), None),
             ("m", (1, 1 / 3, 6 / 18, .1), None), ("e", (.25,), None), ("e", (.5,), (1, .75))]
    for conn in (4, 8):
        s = _check(gpu, [(binary, mask, pred)], rules, conn)[0]
        assert s.num_components == 2
        assert s.cc(0)[0] == 1 and s.cc(1)[0] == 0 and s.cc(1)[2] == 1 and s.cc(2)[0] == 0


def test_random_ink(gpu):
    rng = np.random.default_rng(123)
    for (H, W) in [(48, 200), (130, 70)]:
        mask = rng.integers(0, 3, (H, W)).astype(np.uint8)
        pred = np.where(rng.random((H, W)) < 0.3, rng.integers(0, 3, (H, W)), mask).astype(np.uint8)
        pages = [((rng.random((H, W)) < dens).astype(np.uint8), mask, pred) for dens in (0.05, 0.35, 0.5, 0.62, 0.9)]
        pages += [(np.ones((H, W), np.uint8), mask, pred), (np.zeros((H, W), np.uint8), mask, pred)]
        for conn in (4, 8):
            s = _check(gpu, pages, RULES, conn)
            assert s[-2].num_components == 1 and s[-1].num_components == 0
    # one serpentine component over many tiles
    b = np.zeros((70, 200), np.uint8)
    b[::2, :] = 1
    b[1::4, -1] = 1
    b[3::4, 0] = 1
    mask = np.ones((70, 200), np.uint8)
    pred = (np.arange(200)[None, :] % 3 == 0).astype(np.uint8) * np.ones((70, 1), np.uint8)
    for conn in (4, 8):
        s = _check(gpu, [(b, mask, pred)], RULES, conn)[0]
        assert s.num_components == 1 and s.cc(0)[3] == 1


def test_hand_placed_pages(gpu):
    """3 x 3 tiles of 32 x 64; connectivity 4 and 8 must give different, known component counts."""
    b = np.zeros((96, 192), np.uint8)
    b[31, 63] = b[32, 64] = 1                                            # diagonal across the junction (32, 64): bottom right / top left corners
    b[63, 64] = b[64, 63] = 1                                            # anti-diagonal across the junction (64, 64): bottom left / top right corners
    b[31, 10] = b[32, 11] = b[31, 20] = b[32, 19] = 1                    # diagonal pairs along a horizontal tile edge
    b[10, 63] = b[11, 64] = b[20, 64] = b[21, 63] = 1                    # ... and along a vertical one
    b[5:8, 140:143] = 1                                                  # closed in its tile
    b[12, 120:136] = 1                                                   # open: crosses x = 128
    b[32, 90] = b[63, 95] = b[45, 64] = b[50, 127] = 1                   # one pixel on each rim of tile (1, 1)
    mask = np.ones(b.shape, np.uint8)
    pred = np.ones(b.shape, np.uint8)
    pred[32:, :] = 2                                                     # the lower pixel of every pair across the edge y = 32 disagrees
    want = {4: 18, 8: 12}
    for conn in (4, 8):
        s = _check(gpu, [(b, mask, pred)], RULES + [("e", (.6,), None)], conn)[0]
        assert s.num_components == want[conn]
    # cc_equal(.6): a pair joined across y = 32 is half right (false); apart, its upper pixel is right and its lower one wrong
    s4 = _check(gpu, [(b, mask, pred)], [("e", (.6,), None)], 4)[0]
    s8 = _check(gpu, [(b, mask, pred)], [("e", (.6,), None)], 8)[0]
    assert s4.cc(0) == (9, 9, 0, 18) and s8.cc(0) == (4, 8, 0, 12)
    # the same ink shifted, so that the tile edges fall elsewhere, gives the same counts
    big = np.zeros((96 + 7, 192 + 9), np.uint8)
    big[7:, 9:] = b
    for conn in (4, 8):
        assert _check(gpu, [(big, np.ones(big.shape, np.uint8), np.ones(big.shape, np.uint8))], [], conn)[0].num_components == want[conn]


def _small_pages(n, with_none=True):
    shapes = [(20, 30), (33, 65), (40, 70), (1, 5), (64, 64), (70, 130), (9, 200)]
    pages = []
    for k in range(n):
        H, W = shapes[k % len(shapes)]
        binary, mask, pred = _page(100 + k, H, W, 3, specks=0.15)
        pages.append((None if with_none and k % 9 == 4 else binary, mask, pred))
    return pages


def _raw(gpu, pages, rules, conn=4, ncls=3):
    from ocr4all_pixel_classifier.lib import evaluation as E
    return gpu.eval_pages([p for _, _, p in pages], [m for _, m, _ in pages], [b for b, _, _ in pages], ncls, conn,
                          [E.rule_tuple(r) for r in _lib_rules(rules)])


def _same(a, b, idx=None):
    return all(np.array_equal(a[k] if idx is None else a[k][idx], b[k]) for k in ("counts", "components", "verdicts"))


def test_list_behaviour(gpu):
    pages = _small_pages(70)
    assert len(gpu.eval_page_groups([m.shape for _, m, _ in pages])) >= 2
    rules = RULES[:1] + RULES[3:]
    _check(gpu, pages, rules, 8, ncls=3)
    got = _raw(gpu, pages, rules, 8)
    assert got["components"][4] == 0 and not got["verdicts"][4].any()    # binary None: no components
    assert got["counts"][4][0].sum() == 0                                # ... and every pixel in the ink plane
    assert _same(_raw(gpu, pages, rules, 8), got)                        # a second call
    perm = np.random.default_rng(5).permutation(len(pages))
    assert _same(got, _raw(gpu, [pages[k] for k in perm], rules, 8), perm)
    for k in range(len(pages)):                                          # the list equals each page alone
        assert _same(got, _raw(gpu, [pages[k]], rules, 8), [k])
    # workspace reuse: a large list after a small one, then the small one again
    small = pages[:3]
    large = [_page(7 + k, 300, 400, 3) for k in range(3)] + pages
    a = _raw(gpu, small, rules, 4)
    _check(gpu, large[:3], rules, 4, ncls=3)
    b = _raw(gpu, large, rules, 4)
    assert _same(b, a, slice(3, 6)) and _same(_raw(gpu, small, rules, 4), a)
    gpu.lib().pseg_release_workspace(0)
    assert _same(_raw(gpu, small, rules, 4), a)


def test_null_outputs_and_no_rules(gpu):
    from pseg_amd import engine as E
    pages = _small_pages(5, with_none=False)
    full = _raw(gpu, pages, RULES, 4)
    none = _raw(gpu, pages, [], 4)
    assert none["verdicts"].shape == (5, 0, 4) and np.array_equal(none["counts"], full["counts"]) and np.array_equal(none["components"], full["components"])
    L = gpu.lib()
    keep = [(np.ascontiguousarray(p), np.ascontiguousarray(m), np.ascontiguousarray(b)) for b, m, p in pages]
    arr = (E.EVAL_PAGE * 5)(*[E.EVAL_PAGE(p.ctypes.data, m.ctypes.data, b.ctypes.data, p.shape[0], p.shape[1]) for p, m, b in keep])
    from ocr4all_pixel_classifier.lib import evaluation as LE
    cr = (E.EVAL_RULE * len(RULES))(*[E.EVAL_RULE(*LE.rule_tuple(r)) for r in _lib_rules(RULES)])
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    comps, ver, counts = np.zeros(5, np.int64), np.zeros((5, len(RULES), 4), np.int64), np.zeros((5, 2, 4, 4), np.int64)
    assert L.pseg_eval_pages(0, 5, arr, 3, 4, len(RULES), cr, None, ptr(comps), None) == 0 and np.array_equal(comps, full["components"])
    assert L.pseg_eval_pages(0, 5, arr, 3, 4, len(RULES), cr, None, None, ptr(ver)) == 0 and np.array_equal(ver, full["verdicts"])
    assert L.pseg_eval_pages(0, 5, arr, 3, 4, 0, None, ptr(counts), None, None) == 0 and np.array_equal(counts, full["counts"])
    assert L.pseg_eval_pages(0, 5, arr, 3, 4, len(RULES), cr, None, None, None) == 0
    # refusals: the outputs stay as they were
    before = (counts.copy(), comps.copy(), ver.copy())
    bad = (E.EVAL_RULE * 1)(E.EVAL_RULE(*E.eval_rule(0, 3, .5, .1, .5)))
    nine = (E.EVAL_RULE * 9)(*[cr[0]] * 9)
    for args in [(3, 4, 1, bad), (3, 4, 9, nine), (3, 6, len(RULES), cr)]:
        assert L.pseg_eval_pages(0, 5, arr, *args, ptr(counts), ptr(comps), ptr(ver)) == -1
        assert all(np.array_equal(x, y) for x, y in zip((counts, comps, ver), before))
    with pytest.raises(gpu.PsegError, match="page 1"):
        gpu.eval_pages([keep[0][0], keep[1][0]], [keep[0][1], keep[2][1]], None, 3)


@pytest.fixture(scope="module")
def big_page():
    return _page(2, 2048, 1536, 3, specks=0.0)


@pytest.mark.parametrize("conn", [4, 8])
def test_one_large_page_against_the_component_tables(gpu, big_page, conn):
    """2048 x 1536: counts against eval_confusion; components and verdicts against sums computed vectorised from this tree's
    cc_label + cc_tables (no Python loop over components at this size)."""
    from ocr4all_pixel_classifier.lib import evaluation as E
    binary, mask, pred = big_page
    rules = RULES + [("e", (.5,), (1, .25))]
    got = _raw(gpu, [big_page], rules, conn)
    assert np.array_equal(got["counts"][0], gpu.eval_confusion(pred, mask, binary, 3))
    n, lab = gpu.cc_label(binary, conn)
    t = gpu.cc_tables(lab, n, pred, mask, 3, want_stats=True)
    s = t["stats"][1:, 4].astype(np.int64)
    e, hp, hm = t["eq"][1:], t["hist_pred"][1:], t["hist_mask"][1:]
    assert got["components"][0] == n - 1 and n > 100
    want = np.zeros((len(rules), 4), np.int64)
    for k, rule in enumerate(_lib_rules(rules)):
        kind, label, ttp, tfp, tm, fl, ft = E.rule_tuple(rule)
        keep = np.ones(len(s), bool) if not fl else (hm[:, fl] / s >= ft) | (hp[:, fl] > 0)
        if kind == 0:
            ptp, pfp, mm = hp[:, label] / s >= ttp, hp[:, label] / s >= tfp, hm[:, label] / s >= tm
            want[k, :3] = [(keep & ptp & mm).sum(), (keep & pfp & ~mm).sum(), (keep & mm & ~ptp).sum()]
        else:
            ok = e / s >= ttp
            want[k, :3] = [(keep & ok).sum(), (keep & ~ok).sum(), 0]
        want[k, 3] = keep.sum()
    assert np.array_equal(got["verdicts"][0], want)


def _predictor_and_dataset(gpu, oracle_mod, posts, high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)                   # a bf16 engine
    net.model.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    data = []
    for k, s in enumerate([(100, 130), (100, 130), (93, 127), (100, 130), (93, 127)]):
        img, binary, mask = synth.synth_page(40 + k, s[0], s[1], 3)
        d = SingleData(image=img, binary=binary, mask=mask.astype(np.uint8), original_shape=img.shape, image_path="page%d.png" % k)
        if high_res:
            orig = (s[0] + 71, s[1] + 41)
            rng = np.random.default_rng(k)
            d = dataclasses.replace(d, original_shape=orig, orig_binary=(rng.random(orig) < 0.2).astype(np.uint8),
                                    mask=rng.integers(0, 3, orig).astype(np.uint8))
        data.append(d)
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor(p) for p in posts], high_res_output=high_res)
    return Predictor(settings, net), Dataset(data, cm)


@pytest.mark.parametrize("posts,high_res", [([], False), (["cc_majority"], False), (["cc_majority"], True)])
def test_evaluate_dataset(gpu, oracle_mod, posts, high_res):
    from ocr4all_pixel_classifier.lib import evaluation as E
    from ocr4all_pixel_classifier.lib import image_ops as I
    pred, ds = _predictor_and_dataset(gpu, oracle_mod, posts, high_res)
    rules = [E.cc_matching(1, .5, .1), E.cc_equal(.9), (E.cc_equal(.5), (2, .5))]
    for chunk in (64, 2):
        scores = pred.evaluate_dataset(ds, rules, connectivity=8, chunk=chunk)
        assert len(scores) == len(ds.data)
        for d, s in zip(ds.data, scores):
            p = pred.predict_single(d)
            labels, binary = np.asarray(p.labels), np.asarray(p.data.binary).astype(np.uint8)
            assert labels.shape == np.shape(d.mask) == tuple(d.original_shape if high_res else d.image.shape)
            for label in range(4):
                assert s.count_matches(label) == E.count_matches(d.mask, labels, label)
            assert s.total_accuracy() == E.total_accuracy(d.mask, labels)
            assert s.fgpa() == I.fgpa(labels, d.mask, binary)
            ev = E.ConnectedComponentEval(d.mask, labels, binary, connectivity=8)
            assert s.num_components == ev.num_labels - 1
            m = list(ev.run_per_component(rules[0]))
            assert s.cc(0) == tuple(int(v) for v in np.sum(m, axis=0)) + (len(m),)
            q = list(ev.run_per_component(rules[1]))
            assert s.cc(1) == (sum(map(bool, q)), len(q) - sum(map(bool, q)), 0, len(q))
            ev.only_label(2, .5)
            q = list(ev.run_per_component(rules[2][0]))
            assert s.cc(2) == (sum(map(bool, q)), len(q) - sum(map(bool, q)), 0, len(q))
    ds.data[3] = dataclasses.replace(ds.data[3], mask=np.zeros((5, 5), np.uint8))
    with pytest.raises(Exception, match="page3.png"):
        pred.evaluate_dataset(ds, rules)
    ds.data[3] = dataclasses.replace(ds.data[3], mask=None)
    with pytest.raises(Exception, match="page3.png"):
        pred.evaluate_dataset(ds, rules)
