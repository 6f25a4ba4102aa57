"""pseg_eval_pages' host side, no GPU: how the list is cut into groups, the argument checks of the C entry (all made before a device
is touched) and of the Python wrapper, the rule normalisation, and PageScore's derivations from a NumPy-built joint histogram
against the restatement of the reference's per-page functions."""
import ctypes

import numpy as np
import pytest

from oracle import evaluation as O

GROUP_PAGES, GROUP_PIXELS = 64, 64 << 20          # include/pseg.h: a group ends after 64 pages or before 64 Mi pixels are passed


def _groups(shapes):
    out, g0 = [], 0
    while g0 < len(shapes):
        g1, px = g0, 0
        while g1 < len(shapes) and g1 - g0 < GROUP_PAGES and (g1 == g0 or px + shapes[g1][0] * shapes[g1][1] <= GROUP_PIXELS):
            px += shapes[g1][0] * shapes[g1][1]
            g1 += 1
        out.append((g0, g1 - g0))
        g0 = g1
    return out


def test_groups_tile_the_list_in_order():
    from pseg_amd import engine as E
    assert "pseg_eval_pages" in E.EXPORTED_SYMBOLS and "pseg_eval_page_groups" in E.EXPORTED_SYMBOLS
    assert E.eval_page_groups([]) == []
    rng = np.random.default_rng(7)
    for trial in range(20):
        n = int(rng.integers(1, 300))
        shapes = [(int(rng.integers(0, 4000)), int(rng.integers(0, 3000))) for _ in range(n)]
        if trial % 3 == 0:
            shapes[int(rng.integers(0, n))] = (9000, 8000)              # above the pixel limit: a group of its own
        got = E.eval_page_groups(shapes)
        assert got == _groups(shapes)
        assert got[0][0] == 0 and sum(c for _, c in got) == n
        assert all(got[k][0] + got[k][1] == got[k + 1][0] for k in range(len(got) - 1))
        for f, c in got:
            assert 1 <= c <= GROUP_PAGES
            assert c == 1 or sum(h * w for h, w in shapes[f:f + c]) <= GROUP_PIXELS
    assert E.eval_page_groups([(9000, 8000)] * 3) == [(0, 1), (1, 1), (2, 1)]
    assert E.eval_page_groups([(10, 10)] * 130) == [(0, 64), (64, 64), (128, 2)]
    # max_groups cuts what is written, not what is counted
    L = E.lib()
    H, W = (ctypes.c_int * 130)(*[10] * 130), (ctypes.c_int * 130)(*[10] * 130)
    first, count = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    assert L.pseg_eval_page_groups(130, H, W, first, count, 2) == 3 and list(first) == [0, 64] and list(count) == [64, 64]
    assert L.pseg_eval_page_groups(130, H, W, None, None, 0) == 3
    H[5] = -1
    assert L.pseg_eval_page_groups(130, H, W, first, count, 2) < 0 and b"page 5" in L.pseg_last_error()


def test_c_entry_refuses_before_any_device_work():
    from pseg_amd import engine as E
    L = E.lib()
    p = np.zeros((4, 5), np.uint8)
    page = (E.EVAL_PAGE * 2)(E.EVAL_PAGE(p.ctypes.data, p.ctypes.data, None, 4, 5), E.EVAL_PAGE(p.ctypes.data, p.ctypes.data, None, 4, 5))
    rule = lambda **kw: E.EVAL_RULE(*E.eval_rule(**{"kind": 0, "label": 1, "threshold_tp": .5, "threshold_fp": .1, "threshold_mask": .5, **kw}))
    rules9 = (E.EVAL_RULE * 9)(*[rule() for _ in range(9)])
    counts = np.full((2, 2, 4, 4), -7, np.int64)
    cp = ctypes.c_void_p(counts.ctypes.data)
    call = lambda n_pages=2, ncls=3, conn=4, n_rules=1, rules=rules9: L.pseg_eval_pages(0, n_pages, page, ncls, conn, n_rules, rules, cp, None, None)
    for kw, word in [(dict(ncls=0), b"n_classes"), (dict(ncls=256), b"n_classes"), (dict(conn=6), b"connectivity"), (dict(n_rules=9), b"rules"),
                     (dict(n_rules=-1), b"rules"), (dict(n_pages=-1), b"page count"),
                     (dict(rules=(E.EVAL_RULE * 2)(rule(), rule(label=3)), n_rules=2), b"rule 1"),
                     (dict(rules=(E.EVAL_RULE * 1)(rule(filter_label=5)), n_rules=1), b"rule 0"),
                     (dict(rules=(E.EVAL_RULE * 1)(rule(kind=2)), n_rules=1), b"rule 0")]:
        assert call(**kw) == -1 and word in L.pseg_last_error(), kw
    page[1].H = -1
    assert call() == -1 and b"page 1" in L.pseg_last_error()
    page[1].H, page[1].pred = 4, None
    assert call() == -1 and b"page 1" in L.pseg_last_error()
    assert (counts == -7).all()                                        # nothing was written
    assert call(n_pages=0) == 0 and (counts == -7).all()                # the empty list: PSEG_OK, no device work


def test_wrapper_argument_errors():
    from pseg_amd import engine as E
    a, b = np.zeros((4, 5), np.uint8), np.zeros((4, 6), np.uint8)
    with pytest.raises(E.PsegError, match="page 1"):
        E.eval_pages([a, a], [a, b])
    with pytest.raises(E.PsegError, match="page 0"):
        E.eval_pages([a], [a], [b])
    with pytest.raises(E.PsegError, match="page 2.*0..254"):
        E.eval_pages([a, a, np.full((4, 5), 255, np.uint8)], [a, a, a])
    with pytest.raises(E.PsegError, match="page 0.*0..254"):
        E.eval_pages([a], [np.full((4, 5), -1, np.int64)])
    with pytest.raises(E.PsegError, match="page 0"):
        E.eval_pages([np.zeros((4, 5, 3), np.uint8)], [a])
    with pytest.raises(E.PsegError, match="one entry per page"):
        E.eval_pages([a, a], [a])
    with pytest.raises(E.PsegError, match="9 rules"):
        E.eval_pages([a], [a], rules=[E.eval_rule(1, 0, .5)] * 9)
    with pytest.raises(E.PsegError, match="connectivity"):
        E.eval_pages([a], [a], connectivity=6)
    with pytest.raises(E.PsegError, match="rule 0"):
        E.eval_pages([a], [a], n_classes=3, rules=[E.eval_rule(0, 3, .5, .1, .5)])
    with pytest.raises(E.PsegError, match="n_classes"):
        E.eval_pages([a], [a], n_classes=0)
    # the empty list needs no device
    r = E.eval_pages([], [], rules=[E.eval_rule(1, 0, .5)])
    assert r["counts"].shape == (0, 2, 2, 2) and r["components"].shape == (0,) and r["verdicts"].shape == (0, 1, 4)


def test_rule_normalisation():
    from ocr4all_pixel_classifier.lib import evaluation as E
    assert E.rule_tuple(E.cc_matching(1, .5, .1)) == (0, 1, .5, .1, .5, 0, 0.0)              # falsy threshold_mask: threshold_tp
    assert E.rule_tuple(E.cc_matching(1, .5, .1, 0)) == (0, 1, .5, .1, .5, 0, 0.0)
    assert E.rule_tuple(E.cc_matching(2, .5, .1, .3)) == (0, 2, .5, .1, .3, 0, 0.0)
    assert E.rule_tuple(E.cc_equal(.9)) == (1, 0, .9, 0.0, 0.0, 0, 0.0)
    assert E.rule_tuple((E.cc_equal(.5), (2, .5))) == (1, 0, .5, 0.0, 0.0, 2, .5)
    assert E.rule_tuple((E.cc_equal(.5), (0, .7))) == (1, 0, .5, 0.0, 0.0, 0, 0.0)            # filter label 0: no filter (_filter)
    assert E.rule_tuple((E.cc_matching(1, .5, .1), None)) == (0, 1, .5, .1, .5, 0, 0.0)
    with pytest.raises(Exception):
        E.rule_tuple(lambda m, p: 0)


def _joint(pred, mask, binary, ncls):
    c = np.zeros((2, ncls + 1, ncls + 1), np.int64)
    b = np.ones(pred.shape, int) if binary is None else (binary != 0).astype(int)
    np.add.at(c, (b, mask, pred), 1)
    return c


@pytest.mark.parametrize("ncls,ink", [(3, 0.4), (6, 0.4), (4, 0.0), (3, 1.0)])
def test_page_score_derivations_match_the_restatement(ncls, ink):
    from ocr4all_pixel_classifier.lib import evaluation as E
    rng = np.random.default_rng(ncls)
    mask = rng.integers(0, ncls, (37, 53))
    pred = np.where(rng.random(mask.shape) < 0.2, rng.integers(0, ncls, mask.shape), mask)
    binary = (rng.random(mask.shape) < ink).astype(np.uint8)
    s = E.PageScore(_joint(pred, mask, binary, ncls), 5, np.array([[1, 2, 3, 6], [4, 1, 0, 5]]))
    for label in range(ncls + 2):
        assert s.count_matches(label) == O.count_matches(mask, pred, label)
    assert s.count_matches(-1) == (0, 0, 0)
    assert s.total_accuracy() == O.total_accuracy(mask, pred)
    if ink:
        assert s.fgpa() == O.fgpa(pred, mask, binary)
    else:
        with pytest.raises(ZeroDivisionError):                         # a page without ink, as image_ops.fgpa
            s.fgpa()
    for n in (ncls, ncls - 1, ncls + 2):                               # fewer / more classes asked for than the table has slots
        got, want = s.fgoverlap_per_class(n), O.fgoverlap_per_class(pred, mask, binary, n)
        for g, w in zip(got, want):
            assert len(g) == n + 1 and all((a == b) or (np.isnan(a) and np.isnan(b)) for a, b in zip(g, w))
    assert s.num_components == 5 and s.cc(0) == (1, 2, 3, 6) and s.cc(1) == (4, 1, 0, 5)
    # without a binarisation every pixel is ink
    s = E.PageScore(_joint(pred, mask, None, ncls), 0, np.zeros((0, 4), np.int64))
    assert s.fgpa() == O.fgpa(pred, mask, np.ones_like(mask)) and s.total_accuracy() == O.total_accuracy(mask, pred)
