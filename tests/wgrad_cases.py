"""Cases, data and the float64 reference of the per-layer weight-gradient tests (tests/test_wgrad_layers_gpu.py,
tests/test_wgrad_layers_host.py).  Plain module: nothing here needs a GPU.

A case is a dict of the geometry Engine.wgrad_layer takes.  The instance tables below restate the rows of g_flat / g_blk / g_pair
in csrc/pseg_wgrad_flat.hip; the host test parses the source and fails when the two differ, so a new instance row cannot arrive
without a case."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT_SRC = os.path.join(ROOT, "page-segmentation_amd", "csrc", "pseg_wgrad_flat.hip")

# PSEG_FLAT(XC, CO, KW, KYN, NW, MW, PW, OCC)
FLAT_ROWS = [(1, 20, 5, 5, 2, 1, 64, 8), (20, 30, 5, 5, 4, 8, 64, 3), (30, 40, 5, 5, 8, 6, 32, 2), (40, 40, 5, 5, 8, 8, 32, 2),
             (40, 60, 5, 5, 8, 8, 32, 2), (60, 60, 5, 1, 4, 5, 64, 3), (60, 80, 5, 1, 4, 5, 64, 2), (80, 80, 5, 1, 4, 7, 64, 2),
             (60, 40, 5, 1, 4, 5, 64, 3)]
# PSEG_BLK(XC, CO, KW, NW, MW, PW, OCC)
BLK_ROWS = [(64, 64, 3, 4, 9, 32, 1), (32, 64, 3, 4, 5, 32, 2), (32, 32, 3, 4, 5, 32, 4)]
# PSEG_PAIR(MODE, XC0, XC1, CO, WM, WN, MW, NTW, PW, OCC)
PAIR_ROWS = [(1, 30, 40, 20, 1, 5, 5, 1, 32, 3), (1, 40, 60, 30, 1, 8, 7, 1, 32, 2), (1, 80, 0, 60, 1, 8, 5, 2, 32, 2),
             (1, 30, 0, 20, 1, 5, 2, 1, 32, 3), (1, 40, 0, 30, 1, 8, 3, 1, 32, 2), (0, 20, 30, 16, 4, 1, 1, 1, 64, 4),
             (0, 20, 0, 16, 2, 1, 1, 1, 64, 4)]

WGR_GROUP = 16      # strips per first-level group of the ordered reduction (pseg_train.hip)
H_MAP = 23          # prime, > 2 * KYN + 2: every strip_rows > 1 leaves a short last strip


def source_rows(macro):
    """The argument tuples of every `macro(...)` row in the instance tables of pseg_wgrad_flat.hip (the #define itself has
    no digits in its argument list)."""
    src = open(FLAT_SRC).read()
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"^\s*%s\(([0-9,\s]+)\)" % macro, src, flags=re.M)]


def cdiv(a, b):
    return -(-a // b)


def conv_case(XC, Cout, KW, Hx=H_MAP, Wx=148, stride=1, xup=False, in_relu=False, mask=True):
    return dict(mode=0, KW=KW, stride=stride, xup=xup, in_relu=in_relu, logits=False, XC0=XC, XC1=0, Cout=Cout, Hx=Hx, Wx=Wx,
                Hy=cdiv(Hx, stride), Wy=cdiv(Wx, stride), xpitch=Wx >> int(xup), mask=mask)


def deconv_case(XC0, XC1, Cout, Hx=H_MAP, Wx=148, mask=True):
    return dict(mode=1, KW=2, stride=1, xup=False, in_relu=False, logits=False, XC0=XC0, XC1=XC1, Cout=Cout, Hx=Hx, Wx=Wx,
                Hy=2 * Hx, Wy=2 * Wx, xpitch=Wx, mask=mask)


def logits_case(XC0, XC1, Cout, Hy=H_MAP, Wy=276, Hx=None, Wx=None):
    """The page (Hy, Wy) in the top-left corner of an (Hx, Wx) canvas; no padding, no mask."""
    Hx, Wx = Hx or Hy, Wx or Wy
    return dict(mode=0, KW=1, stride=1, xup=False, in_relu=False, logits=True, XC0=XC0, XC1=XC1, Cout=Cout, Hx=Hx, Wx=Wx, Hy=Hy, Wy=Wy,
                xpitch=Wx, mask=False)


def flat_case(row):
    XC, CO, KW, KYN, NW, MW, PW, OCC = row
    return conv_case(XC, CO, KW, Wx=2 * PW + 20)          # two full pieces and a ragged third: 148 / 84


def blk_cases(row):
    """The block itself, and multiples of it on either side so that blockIdx.z > 0 runs (the planner takes the WIDEST block that
    divides a tensor: a 32-channel side is multiplied by 3, not 2)."""
    XC, CO, KW, NW, MW, PW, OCC = row
    mx, mo = (2 if XC == 64 else 3), (2 if CO == 64 else 3)
    return [conv_case(XC, CO, KW, Wx=2 * PW + 20), conv_case(XC * mx, CO, KW, Wx=2 * PW + 20), conv_case(XC, CO * mo, KW, Wx=2 * PW + 20)]


def pair_cases(row):
    """Mode 1: extents are X's, dY is twice that.  Five pieces per row (4 x PW + 20): with three, no plan has row strips of >= 2
    rows, >= 2 pieces per group AND >= 2 groups at once -- the shape of the real deconv5 plan."""
    MODE, XC0, XC1, CO, WM, WN, MW, NTW, PW, OCC = row
    if MODE == 1:
        return [deconv_case(XC0, XC1, CO, Wx=4 * PW + 20)]
    return [logits_case(XC0, XC1, co, Wy=4 * PW + 20) for co in (2, 3, 16)]


def pair_edge_cases(row):
    """Logits instances only: an odd page width under a wider canvas with Hy < Hx (narrower than one piece: 17; ragged: 77), a
    one-row map."""
    MODE, XC0, XC1, CO, WM, WN, MW, NTW, PW, OCC = row
    assert MODE == 0
    return [logits_case(XC0, XC1, 3, Hy=19, Wy=17, Hx=24, Wx=32), logits_case(XC0, XC1, 5, Hy=21, Wy=77, Hx=24, Wx=96),
            logits_case(XC0, XC1, 16, Hy=1, Wy=148)]


# ---- the planners' arithmetic (csrc/pseg_wgrad_flat.hip), used ONLY to find `slots` values worth running and to show that a
# plan shape is out of the planner's reach; every plan it predicts for a value that runs is compared with the reported one
def model_flat(Hy, Wy, PW, kyg, min_rows, target):
    cpr = cdiv(Wy, PW)
    cg = cpr
    while True:
        rows = cdiv(Hy, max(1, target // (cg * kyg)))
        if rows >= min_rows or cg == 1:
            break
        cg = cdiv(cg, 2)
    cg = cdiv(cpr, cdiv(cpr, cg))
    return rows, cg, cdiv(Hy, rows) * cg


def model_pair(itH, itW, PW, target):
    cpr = cdiv(itW, PW)
    best = None
    for cg in range(1, cpr + 1):
        cper = cdiv(cpr, cg)
        cge = cdiv(cpr, cper)
        rows = cdiv(itH, max(1, min(itH, target // cge)))
        if best is None or rows * cper < best[0]:
            best = (rows * cper, rows, cge)
    return best[1], best[2], cdiv(itH, best[1]) * best[2]


def model_plan(family, row, case, slots):
    """(strip_rows, cgroups, nstrips) the planner gives `case` with `slots` workgroup slots."""
    if family == "flat":
        XC, CO, KW, KYN, NW, MW, PW, OCC = row
        return model_flat(case["Hy"], case["Wy"], PW, KW // KYN, 8 if KYN > 1 else 2, slots)
    if family == "blk":
        XC, CO, KW, NW, MW, PW, OCC = row
        nz = (case["XC0"] // XC) * (case["Cout"] // CO)
        return model_flat(case["Hy"], case["Wy"], PW, 1, 8, max(1, slots // nz))
    MODE, XC0, XC1, CO, WM, WN, MW, NTW, PW, OCC = row
    return model_pair(case["Hx"] if MODE == 1 else case["Hy"], case["Wx"] if MODE == 1 else case["Wy"], PW, slots)


def piece_width(family, row):
    return row[-2]


def plan_properties(itH, itW, PW, strip_rows, cgroups, nstrips):
    """Which of the walk's regimes a plan runs (the letters of the coverage list in test_wgrad_layers_gpu.py)."""
    cpr = cdiv(itW, PW)
    cper = cdiv(cpr, cgroups)
    p = set()
    if strip_rows == 1 and cgroups == 1:
        p.add("a")
    if strip_rows >= 2 and cgroups == 1 and cper >= 2:
        p.add("b")
    if strip_rows >= 2 and cgroups >= 2:
        p.add("c")
    if itH % strip_rows != 0:
        p.add("d")
    if itW % PW != 0:
        p.add("e")                    # the last piece of a row is ragged
    if cpr % cper != 0:
        p.add("e-group")              # the last group has fewer pieces than the others
    if strip_rows >= 2 and cper >= 2 and cgroups >= 2:
        p.add("f")
    p.add("few" if nstrips < WGR_GROUP else ("many" if nstrips > WGR_GROUP else "group"))
    return p


SLOTS_RANGE = range(1, 4097)


def reachable(family, row, case):
    """{property: smallest slots that reaches it} over SLOTS_RANGE, from the model."""
    MODE = row[0] if family == "pair" else 0
    itH, itW = (case["Hx"], case["Wx"]) if MODE == 1 else (case["Hy"], case["Wy"])
    first = {}
    for s in SLOTS_RANGE:
        for p in plan_properties(itH, itW, piece_width(family, row), *model_plan(family, row, case, s)):
            first.setdefault(p, s)
    return first


def slots_list(family, row, case):
    """0 (the device's own plan), 1, and the smallest value for every regime the planner can reach."""
    return [0] + sorted({1} | set(reachable(family, row, case).values()))


# ---- data and reference
def make_data(case, seed, kind="int"):
    """Host arrays of a case: X0 / X1 as stored ((Hx, xpitch, XC) -- at half resolution when xup), dY, maskY (or None).
    kind "int": integer-valued float32 (X, dY in -4..4 with many zeros in X, the mask in {-1, 0, 1}): every product and partial
    sum is an integer below 2^24, so the gradient does not depend on the summation order.  kind "float": standard normal."""
    rng = np.random.default_rng(seed)
    up = int(case["xup"])
    hs, ws = case["Hx"] >> up, case["xpitch"]

    def draw(shape, zeros):
        if kind == "int":
            a = rng.integers(-4, 5, size=shape).astype(np.float32)
            if zeros:
                a[rng.random(shape) < 0.3] = 0.0
            return a
        return rng.standard_normal(shape).astype(np.float32)
    X0 = draw((hs, ws, case["XC0"]), True)
    X1 = draw((hs, ws, case["XC1"]), True) if case["XC1"] else None
    dY = draw((case["Hy"], case["Wy"], case["Cout"]), False)
    maskY = None
    if case["mask"]:
        maskY = rng.integers(-1, 2, size=dY.shape).astype(np.float32) if kind == "int" else rng.standard_normal(dY.shape).astype(np.float32)
    return X0, X1, dY, maskY


def reference(case, X0, X1, dY, maskY, absolute=False):
    """float64 (dW[KW][KW][XC0 + XC1][Cout], dB[Cout]) of the layer; absolute: the same sums over |Xz| and |dY'| (the scale of
    the rounding-error bound)."""
    X = X0.astype(np.float64) if X1 is None else np.concatenate([X0, X1], axis=-1).astype(np.float64)
    dYm = dY.astype(np.float64)
    if maskY is not None:
        dYm = dYm * (maskY > 0)
    if case["xup"]:
        X = X.repeat(2, axis=0).repeat(2, axis=1)
    X = X[:case["Hx"], :case["Wx"]]                       # (rows are xpitch pixels apart; the map is Wx wide)
    if case["in_relu"]:
        X = np.maximum(X, 0.0)
    if absolute:
        X, dYm = np.abs(X), np.abs(dYm)
    k, s, Hy, Wy = case["KW"], case["stride"], case["Hy"], case["Wy"]
    dW = np.zeros((k, k, X.shape[-1], case["Cout"]))
    if case["mode"] == 1:
        for a in range(2):
            for b in range(2):
                dW[a, b] = np.einsum("ijc,ijo->co", X, dYm[a::2, b::2])
    else:
        pt = pl = 0
        if not case["logits"]:                            # TF SAME
            pt = max((Hy - 1) * s + k - case["Hx"], 0) // 2
            pl = max((Wy - 1) * s + k - case["Wx"], 0) // 2
        P = np.zeros((max((Hy - 1) * s + k, pt + X.shape[0]), max((Wy - 1) * s + k, pl + X.shape[1]), X.shape[-1]))
        P[pt:pt + X.shape[0], pl:pl + X.shape[1]] = X
        for ky in range(k):
            for kx in range(k):
                dW[ky, kx] = np.einsum("yxc,yxo->co", P[ky:ky + (Hy - 1) * s + 1:s, kx:kx + (Wy - 1) * s + 1:s], dYm)
    return dW, dYm.sum(axis=(0, 1))
