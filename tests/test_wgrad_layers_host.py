"""Host side of the per-layer weight-gradient tests (no GPU): the case list covers every row of the instance tables, the
float64 reference agrees with torch autograd, and the planner arithmetic that picks `slots` values has the properties the GPU
file's docstring claims."""
import numpy as np
import pytest

import wgrad_cases as wc


@pytest.mark.parametrize("macro,rows", [("PSEG_FLAT", wc.FLAT_ROWS), ("PSEG_BLK", wc.BLK_ROWS), ("PSEG_PAIR", wc.PAIR_ROWS)])
def test_every_instance_row_has_a_case(macro, rows):
    """test_wgrad_layers_gpu.py parametrises over wgrad_cases.*_ROWS: a row added to (or changed in) a table of
    pseg_wgrad_flat.hip without its case fails here."""
    src = wc.source_rows(macro)
    assert len(src) >= 3 and src == rows, (macro, src)


def test_cases_have_the_edges_they_are_there_for():
    for row in wc.FLAT_ROWS:
        c, PW = wc.flat_case(row), row[6]
        assert c["Wy"] == 2 * PW + 20 and c["Wy"] % 4 == 0 and c["Wy"] % PW and c["Hy"] == 23 > 2 * row[3] + 2
    for row in wc.BLK_ROWS:
        for c in wc.blk_cases(row):
            assert c["Wy"] == 2 * row[5] + 20 and c["XC0"] % row[0] == 0 and c["Cout"] % row[1] == 0
    for row in wc.PAIR_ROWS:
        cs = wc.pair_cases(row)
        assert [c["Cout"] for c in cs] == ([row[3]] if row[0] == 1 else [2, 3, 16])
        for c in cs:
            W = c["Wx"] if row[0] == 1 else c["Wy"]
            assert W == 4 * row[8] + 20 and W % 4 == 0 and 16 * c["Hy"] * c["Wy"] < 2 ** 24
        if row[0] == 0:
            e = wc.pair_edge_cases(row)
            assert any(c["Wy"] % 2 and c["Wy"] < row[8] and c["Wy"] < c["xpitch"] and c["Hy"] < c["Hx"] for c in e)
            assert any(c["Wy"] % 2 and c["Wy"] > row[8] and c["Wy"] < c["xpitch"] for c in e) and any(c["Hy"] == 1 for c in e)


def test_reachable_plan_shapes():
    """What the GPU tests require of every case is within the planners' reach, what they document as out of reach is -- for every
    slots value in 1..4096; with three pieces per row the pair planner has no plan of shape (f)."""
    for row in wc.FLAT_ROWS:
        r = set(wc.reachable("flat", row, wc.flat_case(row)))
        assert {"a", "c", "d", "e", "few", "many"} <= r and "e-group" not in r and ("b" in r) == (row[3] > 1), (row, r)
    for row in wc.BLK_ROWS:
        for c in wc.blk_cases(row):
            r = set(wc.reachable("blk", row, c))
            assert {"a", "b", "c", "d", "e", "few", "many"} <= r and "e-group" not in r, (row, r)
    for row in wc.PAIR_ROWS:
        for c in wc.pair_cases(row):
            assert {"a", "b", "c", "d", "e", "e-group", "f", "few", "many"} <= set(wc.reachable("pair", row, c)), row
            assert len(wc.slots_list("pair", row, c)) <= 10
        narrow = wc.deconv_case(row[1], row[2], row[3], Wx=2 * row[8] + 20) if row[0] == 1 else wc.logits_case(row[1], row[2], 3, Wy=2 * row[8] + 20)
        assert "f" not in wc.reachable("pair", row, narrow)


@pytest.mark.parametrize("case", [wc.conv_case(3, 4, 5, Hx=7, Wx=9), wc.conv_case(3, 4, 3, Hx=7, Wx=9, stride=2), wc.conv_case(2, 3, 3, Hx=8, Wx=10, stride=2),
                                  wc.conv_case(3, 2, 2, Hx=6, Wx=8, xup=True), wc.conv_case(3, 4, 3, Hx=5, Wx=6, in_relu=True),
                                  wc.deconv_case(2, 3, 4, Hx=4, Wx=5), wc.logits_case(2, 3, 4, Hy=4, Wy=5, Hx=6, Wx=8)],
                         ids=["k5", "k3s2_odd", "k3s2_even", "k2_xup", "in_relu", "deconv", "logits_canvas"])
def test_reference_agrees_with_torch_autograd(case):
    """The NumPy reference the kernels are held to is the gradient of the layer as torch computes it in float64 (TF SAME
    padding, stride, upsampled and rectified sources, the ReLU mask as a factor on dY)."""
    import torch
    import torch.nn.functional as F
    X0, X1, dY, maskY = wc.make_data(case, 9, "float")
    dW, dB = wc.reference(case, X0, X1, dY, maskY)
    X = torch.from_numpy(np.concatenate([X0] + ([X1] if X1 is not None else []), -1).astype(np.float64)).permute(2, 0, 1)[None]
    if case["xup"]:
        X = F.interpolate(X, scale_factor=2, mode="nearest")
    X = X[:, :, :case["Hx"], :case["Wx"]]
    if case["in_relu"]:
        X = X.relu()
    k, s, Hy, Wy, Cout = case["KW"], case["stride"], case["Hy"], case["Wy"], case["Cout"]
    g = torch.from_numpy(dY.astype(np.float64) * (1.0 if maskY is None else (maskY > 0))).permute(2, 0, 1)[None]
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    if case["mode"] == 1:
        w = torch.zeros(X.shape[1], Cout, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(X, w, b, stride=2).backward(g)
        got = w.grad.permute(2, 3, 0, 1).numpy()
    else:
        w = torch.zeros(Cout, X.shape[1], k, k, dtype=torch.float64, requires_grad=True)
        if case["logits"]:
            X = X[:, :, :Hy, :Wy]
        else:
            th, tw = max((Hy - 1) * s + k - case["Hx"], 0), max((Wy - 1) * s + k - case["Wx"], 0)
            X = F.pad(X, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
        F.conv2d(X, w, b, stride=s).backward(g)
        got = w.grad.permute(2, 3, 1, 0).numpy()
    assert np.abs(got - dW).max() <= 1e-12 * max(1.0, np.abs(dW).max()) and np.abs(b.grad.numpy() - dB).max() <= 1e-12 * max(1.0, np.abs(dB).max())
