"""Every weight-gradient kernel, one layer at a time, against a float64 NumPy reference -- under every strip plan a device could
give it.

The train-step tests (test_train_gpu.py, test_train_arch_gpu.py, test_large_pages_gpu.py section C) reach these kernels through
whole networks on small pages: one row per strip, mostly one column group, and a 2e-3-of-scale bar that cannot see one lost
pixel column.  Here Engine.wgrad_layer (pseg_train_wgrad_layer) runs the launch the train step makes for ONE layer on given
tensors, takes the number of workgroup slots the strip planners size their grids by as an argument, and reports the plan that ran.

Exact regime.  X and dY are integers in -4..4 (many zeros in X), the ReLU mask is in {-1, 0, 1} (so `> 0` is decided at exactly
0): every product and partial sum is an integer below 2^24 (at most 16 x Hy x Wy, maps of a few thousand pixels), the result
does not depend on the summation order -- MFMA, strips, ordered reduction or float atomics -- and the assertion is
np.array_equal.  One dropped, doubled or misplaced pixel fails it.

Float regime (one case per kernel family, standard-normal data): |g - r| <= n * 2^-23 * S elementwise, S = the same sum over
|Xz| and |dY'|, n = terms per element (pixels of the walk + strips).  This is the recursive-summation bound n * u * S, valid for
any order; it is taken with 2^-23 rather than u = 2^-24 because how v_mfma_f32_16x16x4_f32 rounds its internal adds has not
been measured here.

Plans.  Every row of g_flat / g_blk / g_pair (csrc/pseg_wgrad_flat.hip; test_wgrad_layers_host.py holds the case list to the
tables) runs with slots = 0 (the device's own plan), 1, and the smallest value that reaches each of
  (a) one row per strip, one column group            (b) >= 2 rows per strip, one group walking >= 2 pieces
  (c) >= 2 rows per strip, >= 2 groups                (d) a last row strip shorter than the others
  (e) a ragged last piece (and, where reachable, a last group with fewer pieces: "e-group")
  (f) pair kernels: >= 2 rows per strip, >= 2 pieces per group and >= 2 groups (the real deconv5 plan)
and strip counts below and above WGR_GROUP = 16 (both levels of the ordered reduction).  The assertions read the REPORTED plans.
What the planners cannot produce for any slots in 1..4096 (shown from their arithmetic in wgrad_cases.py, which is itself
compared with every reported plan):
  * flat / blk, every case: a ragged last GROUP.  The halving loop of wgrad_flat_plan / wgrad_blk_plan only ever ends at
    cgroups == pieces per row or at 1 (fewer groups mean more row strips, so fewer rows per strip: a count that failed the
    min_rows test keeps failing it), and both divide the pieces evenly.
  * flat instances with KYN == 1 (conv6, conv7, deconv1, deconv3; min_rows = 2): (b).  One group is reached only when one piece
    per group already gave one row per strip, and then one group gives one row per strip as well.
  * pair: nothing; their cases are five pieces wide because with three pieces (f) is out of reach.
The kernels of pseg_train.hip take strip_rows from the caller: their cases pass it.  Every variant launch_wgrad can choose
(PAIR, FLAT / BLK, C1, KX5, TAP, WIDE) has a case.
"""
import numpy as np
import pytest

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64              # floats of sentinel on either side of dW / dB


@pytest.fixture(scope="module")
def engines(gpu):
    """Engines by plan switches (tuple of names set to 1), created on demand, train_init done."""
    made = {}

    def get(*switches):
        if switches not in made:
            e = gpu.Engine("fcn", 3, mode=gpu.MODE_F32_EXACT, plan={s: "1" for s in switches})
            e.train_init()
            made[switches] = e
        return made[switches]
    yield get
    for e in made.values():
        e.close()


class Layer:
    """A case with its data on the device and its float64 reference (computed once)."""

    def __init__(self, case, seed=1, kind="int"):
        import torch
        self.case, self.kind = case, kind
        self.host = wc.make_data(case, seed, kind)
        self.dev = [None if a is None else torch.from_numpy(a).cuda() for a in self.host]
        self.ref_dW, self.ref_dB = wc.reference(case, *self.host)
        self.XC = case["XC0"] + case["XC1"]
        torch.cuda.synchronize()

    def run(self, eng, slots=0, strip_rows=0, ci0=0, Cin=None, bias=True, source=None, zero=False):
        """-> (dW[KW][KW][XC][Cout] of the written channel block, dB or None, reported plan).  Asserts that nothing outside that
        block changed.  source 0 / 1: the launch the train step makes for ONE concat source where no two-source instance runs
        (its channel block of the layer's dW; the caller gives the second no bias)."""
        import torch
        c = self.case
        X0, X1, dY, maskY = self.dev
        XC0, XC1, xc = c["XC0"], c["XC1"], self.XC
        if source is not None:
            X0, XC0, ci0, Cin = (X0, XC0, 0, self.XC) if source == 0 else (X1, XC1, XC0, self.XC)
            X1, XC1, xc = None, 0, XC0
        Cin = Cin or xc
        k, Cout = c["KW"], c["Cout"]
        fill = 0.0 if zero else SENTINEL
        wbuf = torch.full((2 * GUARD + k * k * Cin * Cout,), SENTINEL, dtype=torch.float32, device="cuda")
        bbuf = torch.full((2 * GUARD + Cout,), SENTINEL, dtype=torch.float32, device="cuda")
        wbuf[GUARD:-GUARD] = fill
        bbuf[GUARD:-GUARD] = fill if bias else SENTINEL
        torch.cuda.synchronize()
        plan = eng.wgrad_layer(X0, dY, wbuf[GUARD:], mode=c["mode"], KW=k, Cin=Cin, Cout=Cout, Hx=c["Hx"], Wx=c["Wx"], Hy=c["Hy"], Wy=c["Wy"],
                               XC0=XC0, X1=X1, XC1=XC1, ci0=ci0, maskY=maskY, dB=bbuf[GUARD:] if bias else None, stride=c["stride"],
                               xup=c["xup"], in_relu=c["in_relu"], logits=c["logits"], xpitch=c["xpitch"], slots=slots, strip_rows=strip_rows)
        w, b = wbuf.cpu().numpy(), bbuf.cpu().numpy()
        assert (w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all(), "dW guard overwritten"
        assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), "dB guard overwritten"
        w = w[GUARD:-GUARD].reshape(k, k, Cin, Cout)
        other = np.ones(Cin, bool)
        other[ci0:ci0 + xc] = False
        assert (w[:, :, other] == fill).all(), "channels of dW outside ci0 .. ci0 + XC were written"
        if not bias:
            assert (b == SENTINEL).all(), "dB written although none was asked for"
        return w[:, :, ci0:ci0 + xc].copy(), (b[GUARD:-GUARD].copy() if bias else None), plan

    def want(self, source=None):
        x0 = self.case["XC0"]
        return (self.ref_dW if source is None else self.ref_dW[:, :, :x0] if source == 0 else self.ref_dW[:, :, x0:]), self.ref_dB

    def check(self, eng, **kw):
        """Exact comparison of one run; -> the reported plan."""
        assert self.kind == "int"
        w, b, plan = self.run(eng, **kw)
        rw, rb = self.want(kw.get("source"))
        bad = np.argwhere(w != rw)
        assert bad.size == 0, "dW differs at %d of %d elements, first (ky, kx, ci, co) = %s: %r vs %r under %r" % (
            len(bad), w.size, tuple(bad[0]), w[tuple(bad[0])], rw[tuple(bad[0])], plan)
        if b is not None:
            assert np.array_equal(b, rb), ("dB", plan, b, rb)
        return plan

    def check_float(self, eng, **kw):
        assert self.kind == "float"
        w, b, plan = self.run(eng, **kw)
        sw, sb = wc.reference(self.case, *self.host, absolute=True)
        c = self.case
        n = (c["Hx"] * c["Wx"] if c["mode"] == 1 else c["Hy"] * c["Wy"]) + plan["nstrips"]
        ew, bw = np.abs(w - self.ref_dW), n * 2.0 ** -23 * sw
        print("float %r: max |dW err| / bound = %.3g, plan %r" % (c, float((ew / np.maximum(bw, 1e-300)).max()), plan))
        assert (ew <= bw).all(), (float(ew.max()), plan)
        if b is not None:
            eb, bb = np.abs(b - self.ref_dB), (c["Hy"] * c["Wy"] + plan["nstrips"]) * 2.0 ** -23 * sb     # (terms of dB: every dY pixel)
            print("      max |dB err| / bound = %.3g" % float((eb / np.maximum(bb, 1e-300)).max()))
            assert (eb <= bb).all(), (float(eb.max()), plan)
        return plan


def _walk_extent(case):
    return (case["Hx"], case["Wx"]) if case["mode"] == 1 else (case["Hy"], case["Wy"])


def _planned(engines, family, row, case, variant, instance):
    """Runs `case` exactly under every slots value of its list, holds every reported plan to the planners' arithmetic, and
    asserts the coverage of the module docstring from the REPORTED plans."""
    eng = engines()
    lay = Layer(case)
    itH, itW = _walk_extent(case)
    seen = {}
    for slots in wc.slots_list(family, row, case):
        plan = lay.check(eng, slots=slots)
        assert (plan["variant"], plan["instance"], plan["piece_width"], plan["deterministic"]) == (variant, instance, wc.piece_width(family, row), 1), plan
        assert plan["nstrips"] == wc.cdiv(itH, plan["strip_rows"]) * plan["cgroups"], plan
        if slots > 0:
            assert (plan["strip_rows"], plan["cgroups"], plan["nstrips"]) == wc.model_plan(family, row, case, slots), (slots, plan)
        for p in wc.plan_properties(itH, itW, plan["piece_width"], plan["strip_rows"], plan["cgroups"], plan["nstrips"]):
            seen.setdefault(p, slots)
    need = {"a", "b", "c", "d", "e", "few", "many"} | ({"f", "e-group"} if family == "pair" else set())
    cannot = set()
    if family != "pair":
        cannot.add("e-group")
        if family == "flat" and row[3] == 1:
            cannot.add("b")
    # what the docstring calls out of reach is out of reach for EVERY slots value (arithmetic, checked against the reports above)
    assert not (cannot & set(wc.reachable(family, row, case))), (cannot, wc.reachable(family, row, case))
    assert need - cannot <= set(seen), "regimes not run: %s (ran %r)" % (sorted(need - cannot - set(seen)), seen)
    return lay, eng


@pytest.mark.parametrize("k", range(len(wc.FLAT_ROWS)), ids=["flat%d_%dto%d" % (k, r[0], r[1]) for k, r in enumerate(wc.FLAT_ROWS)])
def test_flat_instance_under_every_plan(engines, k):
    row = wc.FLAT_ROWS[k]
    lay, eng = _planned(engines, "flat", row, wc.flat_case(row), "FLAT", k)
    # one source of a wider layer (deconv3 runs this instance for both sources of its concat): only its channel block of dW,
    # and no bias gradient for the second source
    XC = row[0]
    lay.check(eng, slots=6, ci0=XC + 3, Cin=2 * XC + 5, bias=False)
    lay.check(eng, slots=1, ci0=0, Cin=XC + 2)


@pytest.mark.parametrize("k,j", [(k, j) for k in range(len(wc.BLK_ROWS)) for j in range(3)],
                         ids=["blk%d_%s" % (k, n) for k in range(len(wc.BLK_ROWS)) for n in ("block", "xc_blocks", "co_blocks")])
def test_blk_instance_under_every_plan(engines, k, j):
    row = wc.BLK_ROWS[k]
    case = wc.blk_cases(row)[j]
    assert (case["XC0"] // row[0]) * (case["Cout"] // row[1]) == (1, 2 if row[0] == 64 else 3, 2 if row[1] == 64 else 3)[j]   # blockIdx.z > 0
    lay, eng = _planned(engines, "blk", row, case, "BLK", k)
    if j == 0:
        lay.check(eng, slots=6, ci0=row[0], Cin=2 * row[0], bias=False)


@pytest.mark.parametrize("k,j", [(k, j) for k, r in enumerate(wc.PAIR_ROWS) for j in range(len(wc.pair_cases(r)))],
                         ids=["pair%d_%s" % (k, "deconv" if r[0] == 1 else "logits_co%d" % c["Cout"])
                              for k, r in enumerate(wc.PAIR_ROWS) for c in wc.pair_cases(r)])
def test_pair_instance_under_every_plan(engines, k, j):
    row = wc.PAIR_ROWS[k]
    _planned(engines, "pair", row, wc.pair_cases(row)[j], "PAIR", k)


@pytest.mark.parametrize("k", [k for k, r in enumerate(wc.PAIR_ROWS) if r[0] == 0])
def test_logits_instances_on_a_page_inside_a_wider_canvas(engines, k):
    """Odd page widths under a wider row pitch with Hy < Hx (the canvas beyond the page holds non-zero values that must not be
    read), a map narrower than one piece, a one-row map."""
    eng = engines()
    for case in wc.pair_edge_cases(wc.PAIR_ROWS[k]):
        lay = Layer(case, seed=2)
        for slots in (0, 1, 2, 18):
            plan = lay.check(eng, slots=slots)
            assert (plan["variant"], plan["instance"]) == ("PAIR", k), plan


# ---- the kernels of pseg_train.hip: (name, plan switches of the engine, case, strip_rows values, expected report)
def _exp(variant, ti, tj, lds=0):
    return dict(variant=variant, ti=ti, tj=tj, lds_staged=lds)


OLD = [
    # every (ti, tj) of the TAP list, k3 on an odd-width map (quads past the right edge), one row and four rows (short last) per strip
    ("tap_1x2", (), wc.conv_case(12, 20, 3, Wx=37), (0, 4), _exp("TAP", 1, 2)),
    ("tap_2x2", (), wc.conv_case(20, 24, 3, Wx=37), (0, 4), _exp("TAP", 2, 2)),
    ("tap_2x3", (), wc.conv_case(24, 40, 3, Wx=37), (0, 4), _exp("TAP", 2, 3)),
    ("tap_3x3", (), wc.conv_case(40, 36, 3, Wx=37), (0, 4), _exp("TAP", 3, 3)),
    ("tap_3x5", (), wc.conv_case(36, 70, 3, Wx=37), (0, 4), _exp("TAP", 3, 5)),
    ("tap_5x3", (), wc.conv_case(70, 40, 3, Wx=37), (0, 4), _exp("TAP", 5, 3)),
    ("tap_5x5", (), wc.conv_case(68, 72, 3, Wx=37), (0, 4), _exp("TAP", 5, 5)),
    ("tap_5x5_k5_no_flat", ("PSEG_WGRAD_NO_FLAT",), wc.conv_case(60, 60, 5, Wx=37), (0, 4), _exp("TAP", 5, 5)),
    ("tap_5x5_k3_no_blk", ("PSEG_WGRAD_NO_BLK",), wc.conv_case(64, 64, 3, Wx=37), (0, 4), _exp("TAP", 5, 5)),
    ("tap_deconv", (), wc.deconv_case(12, 0, 10, Wx=37), (0, 4), _exp("TAP", 1, 2)),
    ("tap_deconv_no_pair", ("PSEG_WGRAD_NO_PAIR",), wc.deconv_case(30, 40, 20, Wx=37), (0, 4), dict(variant="TAP")),       # (30 and 40 channels: two instances)
    ("tap_logits_no_pair", ("PSEG_WGRAD_NO_PAIR",), wc.logits_case(20, 30, 3, Hy=19, Wy=17, Hx=24, Wx=32), (0, 4), _exp("TAP", 2, 2)),
    # KX5, LDS-staged (stride 1): two 64-pixel pieces and a ragged third; the caller's rows are divided by five (15 -> 3)
    ("kx5_lds_1x2", (), wc.conv_case(8, 20, 5), (0, 15), _exp("KX5", 1, 2, 1)),
    ("kx5_lds_2x2", ("PSEG_WGRAD_NO_FLAT",), wc.conv_case(20, 30, 5), (0, 15), _exp("KX5", 2, 2, 1)),
    ("kx5_lds_2x3", (), wc.conv_case(24, 40, 5), (0, 15), _exp("KX5", 2, 3, 1)),
    # KX5, direct (stride 2 / upsampled source)
    ("kx5_direct_1x2", (), wc.conv_case(1, 20, 5, Hx=46, Wx=73, stride=2), (0, 15), _exp("KX5", 1, 2, 0)),
    ("kx5_direct_2x2", (), wc.conv_case(20, 30, 5, Hx=46, Wx=74, xup=True), (0, 15), _exp("KX5", 2, 2, 0)),
    ("kx5_direct_2x3", (), wc.conv_case(24, 40, 5, Hx=45, Wx=74, stride=2, in_relu=True), (0, 15), _exp("KX5", 2, 3, 0)),
    # one-channel input: taps as MFMA rows (TM = 1: up to 16 taps, 2: up to 32) x Cout <= 32 / <= 64; plans its own strips
    # (rows / 1024: the tall map is the smallest with two rows per strip, and 1027 leaves a short last one)
    ("c1_k1_co20", (), wc.conv_case(1, 20, 1, Wx=37), (0,), _exp("C1", 1, 2)),
    ("c1_k3_co40", (), wc.conv_case(1, 40, 3, Wx=37), (0,), _exp("C1", 1, 4)),
    ("c1_k5_co24", (), wc.conv_case(1, 24, 5, Wx=37), (0,), _exp("C1", 2, 2)),
    ("c1_k5_co50", (), wc.conv_case(1, 50, 5, Wx=37), (0,), _exp("C1", 2, 4)),
    ("c1_k5_co20_no_flat", ("PSEG_WGRAD_NO_FLAT",), wc.conv_case(1, 20, 5, Wx=37), (0,), _exp("C1", 2, 2)),
    ("c1_k3_tall", (), wc.conv_case(1, 20, 3, Hx=1027, Wx=9), (0,), _exp("C1", 1, 2)),
    # WIDE: 64 x 64 channel blocks on blockIdx.z, channel counts that are no multiple of 64
    ("wide_stride2", (), wc.conv_case(100, 70, 3, Hx=45, Wx=73, stride=2), (0, 4), _exp("WIDE", 4, 4)),
    ("wide_k2_xup", (), wc.conv_case(130, 40, 2, Hx=24, Wx=38, xup=True), (0, 5), _exp("WIDE", 4, 4)),
    ("wide_in_relu", (), wc.conv_case(70, 130, 3, Wx=37, in_relu=True), (0, 4), _exp("WIDE", 4, 4)),
]


@pytest.mark.parametrize("name,switches,case,strip_rows,expect", OLD, ids=[o[0] for o in OLD])
def test_train_hip_kernels(engines, name, switches, case, strip_rows, expect):
    eng = engines(*switches)
    lay = Layer(case, seed=3)
    itH = _walk_extent(case)[0]
    deconv = case["mode"] == 1                       # (its bias gradient is bias_grad_kernel's, not part of this launch)
    rows_seen = set()
    for sr in strip_rows:
        for source in ((0, 1) if case["XC1"] else (None,)):
            plan = lay.check(eng, strip_rows=sr, bias=not deconv and source != 1, source=source)
            assert {n: plan[n] for n in expect} == expect, plan
            assert plan["nstrips"] == wc.cdiv(itH, plan["strip_rows"]) and plan["cgroups"] == 1, plan
            rows_seen.add(plan["strip_rows"])
    if name == "c1_k3_tall":
        assert rows_seen == {2} and itH % 2 == 1
    elif expect["variant"] != "C1":
        assert 1 in rows_seen and any(r >= 2 and itH % r for r in rows_seen), rows_seen   # one row per strip, and a short last strip


ATOMIC = [
    ("flat", wc.flat_case(wc.FLAT_ROWS[1]), dict(slots=6), "FLAT"),
    ("flat_kyn1", wc.flat_case(wc.FLAT_ROWS[5]), dict(slots=30), "FLAT"),
    ("blk", wc.blk_cases(wc.BLK_ROWS[2])[1], dict(slots=18), "BLK"),
    ("pair_deconv", wc.pair_cases(wc.PAIR_ROWS[0])[0], dict(slots=18), "PAIR"),
    ("pair_logits", wc.pair_cases(wc.PAIR_ROWS[5])[1], dict(slots=18), "PAIR"),
    ("c1", wc.conv_case(1, 24, 5, Wx=37), dict(), "C1"),
    ("kx5", wc.conv_case(24, 40, 5), dict(strip_rows=15), "KX5"),
    ("tap", wc.conv_case(40, 36, 3, Wx=37), dict(strip_rows=4), "TAP"),
    ("wide", wc.conv_case(100, 70, 3, Hx=45, Wx=73, stride=2), dict(strip_rows=4), "WIDE"),
]


@pytest.mark.parametrize("name,case,kw,variant", ATOMIC, ids=[a[0] for a in ATOMIC])
def test_atomic_form_is_exact_on_integer_data(engines, name, case, kw, variant):
    """PSEG_WGRAD_ATOMIC: the strips add into dW / dB (zeroed by the caller, as the train step zeroes its gradient buffer) with
    float atomics; on integer data the arrival order does not matter."""
    eng = engines("PSEG_WGRAD_ATOMIC")
    lay = Layer(case, seed=5)
    plan = lay.check(eng, zero=True, **kw)
    assert plan["variant"] == variant and plan["deterministic"] == 0 and plan["nstrips"] >= 2, plan


FLOAT = [
    ("flat", wc.flat_case(wc.FLAT_ROWS[3]), dict(slots=6)),
    ("flat_kyn1", wc.flat_case(wc.FLAT_ROWS[7]), dict(slots=30)),
    ("blk", wc.blk_cases(wc.BLK_ROWS[0])[0], dict(slots=6)),
    ("pair_deconv", wc.pair_cases(wc.PAIR_ROWS[1])[0], dict(slots=18)),
    ("pair_logits", wc.pair_cases(wc.PAIR_ROWS[5])[1], dict(slots=18)),
    ("c1", wc.conv_case(1, 50, 5, Wx=37), dict()),
    ("kx5_lds", wc.conv_case(24, 40, 5), dict(strip_rows=15)),
    ("kx5_direct", wc.conv_case(24, 40, 5, Hx=45, Wx=74, stride=2, in_relu=True), dict(strip_rows=15)),
    ("tap", wc.conv_case(68, 72, 3, Wx=37), dict(strip_rows=4)),
    ("wide", wc.conv_case(70, 130, 3, Wx=37, in_relu=True), dict(strip_rows=4)),
]


@pytest.mark.parametrize("name,case,kw", FLOAT, ids=[f[0] for f in FLOAT])
def test_float_data_within_the_recursive_summation_bound(engines, name, case, kw):
    """|g - r| <= n * 2^-23 * S elementwise (module docstring): normal-distributed data, one case per kernel family.  2^-23, not
    the unit roundoff 2^-24: the rounding of the f32 MFMA's internal adds has not been measured here."""
    Layer(case, seed=6, kind="float").check_float(engines(), **kw)


def test_repeated_calls_and_a_growing_scratch(engines):
    """Two calls in a row return identical bits (float data: the order matters and is fixed); a call with many strips after one
    with few grows the partial-sum scratch, and the small plan still matches afterwards."""
    import pseg_amd
    eng = pseg_amd.Engine("fcn", 3, mode=pseg_amd.MODE_F32_EXACT, plan={})     # a fresh train state: the scratch starts empty
    eng.train_init()
    try:
        case = wc.flat_case(wc.FLAT_ROWS[2])
        fl = Layer(case, seed=7, kind="float")
        w1, b1, p1 = fl.run(eng, slots=6)
        w2, b2, p2 = fl.run(eng, slots=6)
        assert p1 == p2 and w1.tobytes() == w2.tobytes() and b1.tobytes() == b2.tobytes()
        it = Layer(case, seed=8)
        few = it.check(eng, slots=1)
        many = it.check(eng, slots=24)
        again = it.check(eng, slots=1)
        assert few == again and few["nstrips"] < wc.WGR_GROUP < many["nstrips"], (few, many)
        w3, b3, p3 = fl.run(eng, slots=6)
        assert p3 == p1 and w3.tobytes() == w1.tobytes() and b3.tobytes() == b1.tobytes()
    finally:
        eng.close()


def test_entry_rejects_what_the_train_step_never_launches(engines):
    import torch
    import pseg_amd
    eng = engines()
    t = torch.zeros(4096, dtype=torch.float32, device="cuda")
    geo = dict(KW=3, Cin=4, Cout=4, Hx=4, Wx=4, Hy=4, Wy=4, XC0=4)
    for bad in (dict(geo, Hy=3), dict(geo, XC0=5), dict(geo, stride=3), dict(geo, mode=1), dict(geo, xpitch=3), dict(geo, XC1=2),
                dict(geo, mode=1, KW=2, Hy=8, Wy=8, dB=t)):                    # (no two-source instance for 4 -> 4: no bias gradient)
        with pytest.raises(pseg_amd.PsegError):
            eng.wgrad_layer(t, t, t, **bad)
    fresh = pseg_amd.Engine("fcn", 3, mode=pseg_amd.MODE_F32_EXACT, plan={})
    try:
        with pytest.raises(pseg_amd.PsegError):
            fresh.wgrad_layer(t, t, t, **geo)                                   # pseg_train_init has not run
    finally:
        fresh.close()
