"""oracle/exact.py on the host: the bf16 oracle stands in for the engine (forced = its own activations).
(1) the reference stays inside the derived bound at every element, also with the round-to-nearest constant 2^-24 (the oracle
rounds to nearest), so the looser truncation-safe 2^-23 is not what makes it pass; (2) tensors that the engine fuses away may
be missing from `forced`: their group is checked at its output; (3) six kernel faults, each injected into ONE layer of the
stand-in (the layers behind it are computed from the faulty tensor, as a real engine would), are reported in that layer and
in no other -- forcing isolates layers."""
import numpy as np
import pytest

CASES = [("fcn_skip", 3, (70, 50), 1, False), ("fcn_skip", 3, (33, 1), 1, False), ("fcn_skip", 20, (64, 96), 1, False),
         ("fcn_skip", 3, (64, 96), 3, False), ("fcn", 3, (96, 64), 1, False), ("unet", 3, (32, 64), 1, False),
         ("res_unet", 3, (70, 50), 1, False), ("res_unet", 3, (64, 96), 1, True)]


def _setup(oracle_mod, arch, C, shape, in_ch=1, bn=False):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=shape + ((3,) if in_ch == 3 else ()), dtype=np.uint8)
    Wt = oracle_mod.init_weights(arch, C, seed=42, in_ch=in_ch, gain=1.5, bias_scale=0.05, batch_norm=bn)
    return img, Wt


def _violations(exact, layers, tensors):
    """{layer: Report} of every layer that has an engine tensor (the logits among them), and the report text."""
    reps = {n: exact.check(tensors[n], l.s, l.bound, n) for n, l in layers.items() if n in tensors}
    text = "; ".join("%s %.3f" % (n, r.ratio) for n, r in reps.items())
    return reps, "max error / bound per layer: " + text


@pytest.mark.parametrize("arch,C,shape,in_ch,bn", CASES)
def test_exact_oracle_reference_stays_inside_the_bound(oracle_mod, arch, C, shape, in_ch, bn):
    from oracle import exact
    img, Wt = _setup(oracle_mod, arch, C, shape, in_ch, bn)
    z, acts = oracle_mod.forward(arch, Wt, img, "bf16", return_acts=True)
    assert acts["logits"] is z or np.array_equal(acts["logits"], z)
    for u in (exact.U_F32, exact.U_F32_NEAREST):
        layers = exact.evaluate(arch, Wt, img, acts, u=u)
        assert set(acts) <= set(layers) and list(layers)[-1] == "logits"
        reps, text = _violations(exact, layers, acts)
        assert len(reps) == len(acts)
        for n, r in reps.items():
            assert r.count == 0, "u = 2^%d, %s: %d elements over the bound, worst %r\n%s" % (np.log2(u), n, r.count, r.worst, text)
        assert all(layers[n].all_forced for n in acts), text
        # the reference is not far inside either: the bound is not slack (rounding to bf16 alone reaches 2^-8 |s|)
        assert max(r.ratio for n, r in reps.items() if n != "logits") > 0.9, text
        bad, excused = exact.check_labels(np.argmax(z, -1), layers["logits"].s, layers["logits"].bound)
        assert bad == 0 and excused <= 0.02, (bad, excused)


@pytest.mark.parametrize("arch,drop", [
    ("fcn_skip", ("conv2d",)),                                   # conv1 inside conv2's kernel
    ("fcn_skip", ("conv2d_transpose",)),                         # deconv1 in front of deconv2
    ("fcn_skip", ("conv2d_transpose_4",)),                       # the last transposed conv in front of the logits
    ("fcn_skip", ("conv2d_3",)),                                 # a conv output that only its pool reads
    ("fcn_skip", ("conv2d_transpose_3", "conv2d_transpose_4")),  # deconv4 and deconv5 inside the tail
    ("fcn_skip", ("conv2d_1", "conv2d_transpose_4")),            # both sources of the logits layer
    ("fcn", ("conv2d", "conv2d_1")),                             # fcn: conv2 is pool-only, behind the fused conv1
    ("fcn", ("conv2d_transpose", "conv2d_transpose_1")),
    ("unet", ("conv2d_21",)),                                    # the last conv runs the logits in its epilogue
    ("res_unet", ("conv2d", "conv2d_27")),                       # stored after the readers' ReLU / in front of the logits
])
def test_exact_oracle_groups(oracle_mod, arch, drop):
    """Tensors missing from `forced`: their readers take the exact value with its bound instead, so the group is checked at its
    outputs -- with the wider, still derived bound; every remaining check passes, and the logits stay covered."""
    from oracle import exact, core
    img, Wt = _setup(oracle_mod, arch, 3, (32, 64) if arch == "unet" else (70, 50))
    z, acts = oracle_mod.forward(arch, Wt, img, "bf16", return_acts=True)
    full = exact.evaluate(arch, Wt, img, acts)
    forced = {n: a for n, a in acts.items() if n not in drop}
    for n, l in full.items():                                   # the pools: stored tensors of the engine as well
        if n.startswith("max_pooling2d") and l.inputs[0] not in drop:
            forced[n] = core.maxpool2(acts[l.inputs[0]])
    layers = exact.evaluate(arch, Wt, img, forced)
    reps, text = _violations(exact, layers, forced)
    assert "logits" in reps and len(reps) == len(forced)
    assert all(r.count == 0 for r in reps.values()), text
    readers, inside = [], set(drop)                             # the ops that read a group's inside, in graph order
    for n, l in layers.items():
        if set(l.inputs) & inside:
            readers.append(n)
            if n not in forced:
                inside.add(n)
    assert readers and all(not layers[n].all_forced for n in readers)
    assert all(l.all_forced for n, l in layers.items() if n not in readers)
    for n in readers:                                           # a group's bound is wider than the forced one, never tighter
        assert np.all(layers[n].bound >= full[n].bound)
    # the dropped tensors themselves still lie inside their own (forced-input) bound: nothing was lost by not checking them
    assert all(exact.check(acts[n], layers[n].s, layers[n].bound, n).count == 0 for n in drop)


# ---- mutations: a stand-in engine with one faulty layer ------------------------------------------------------------------

def _trunc_bf16(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _mutant_forward(oracle_mod, arch, Wt, img, target, fault):
    """oracle.forward in bf16 mode, with layer `target` computed by fault(ctx, x, kw) -> tensor instead."""
    from oracle import models, core

    class Mutant(models._Ctx):
        def crop(self, x, pads):
            self.uncropped = x
            return models._crop(x, pads)

        def _swap(self, y, x, kw):
            name = next(reversed(self.acts))
            if name == target:
                y = self.acts[name] = fault(self, x, kw)
                self.hit = True
            return y

        def conv(self, x, **kw):
            return self._swap(super().conv(x, **kw), x, kw)

        def tconv5(self, x, **kw):
            return self._swap(super().tconv5(x, **kw), x, kw)

    c = Mutant(Wt, "bf16")
    c.hit = False
    x = c.q(core.preprocess(img))[..., None]
    z = models._fcn(c, x, arch == "fcn_skip")
    assert c.hit
    return z, c.acts


def _fault_dropped_term(c, x, kw):
    """conv2 (no ReLU): the (centre tap, cin) product left out along output column 7, for the liveliest input channel."""
    from oracle import core
    w, b = c.W["conv2d_1/kernel"], c.W["conv2d_1/bias"]
    ci = int(np.argmax(np.abs(x[:, 7]).mean(0)))
    term = x[:, 7, ci, None] * w[2, 2, ci]                       # (H, Cout)
    assert np.count_nonzero(term) > 0.5 * term.size              # a live channel: the term is there to be missed
    y = core.conv2d(x, w, b)
    y[:, 7] -= term
    return c.q(y)


def _fault_truncation(c, x, kw):
    from oracle import core
    return _trunc_bf16(core.conv2d(x, c.W["conv2d_2/kernel"], c.W["conv2d_2/bias"], relu=True))


def _fault_stale_halo(c, x, kw):
    """conv4: the halo column left of the canvas holds its neighbour (column 0) instead of zeros."""
    from oracle import core
    H, W, _ = x.shape
    xp = np.pad(x, ((2, 2), (2, 2), (0, 0)))
    xp[:, 1] = xp[:, 2]
    return c.q(core.conv2d(xp, c.W["conv2d_3/kernel"], c.W["conv2d_3/bias"], pad=(0, 0, H, W)))


def _fault_concat_swapped(c, x, kw):
    """deconv3 reads [conv6, deconv2] instead of [deconv2, conv6] (60 channels each)."""
    from oracle import core
    assert x.shape[2] == 120
    K = c.W["conv2d_transpose_2/kernel"]
    wc = np.ascontiguousarray(np.transpose(K[::-1, ::-1], (0, 1, 3, 2)))
    return c.q(core.conv2d(np.ascontiguousarray(np.concatenate([x[..., 60:], x[..., :60]], -1)), wc, c.W["conv2d_transpose_2/bias"], relu=True))


def _fault_bias_after_rounding(c, x, kw):
    from oracle import core
    b = c.W["conv2d_1/bias"]
    return (c.q(core.conv2d(x, c.W["conv2d_1/kernel"], np.zeros_like(b))) + b).astype(np.float32)


def _fault_logits_from_uncropped_canvas(c, x, kw):
    """Class 1 of the logits walks the un-cropped canvas with the page's row length: right past column W it reads the padding."""
    from oracle import core
    w, b = c.W["logits/kernel"], c.W["logits/bias"]
    z = core.conv2d(x, w, b)
    H, W, _ = z.shape
    assert c.uncropped.shape[1] > W
    z[..., 1] = core.conv2d(c.uncropped, w, b)[..., 1].ravel()[:H * W].reshape(H, W)
    return z


@pytest.mark.parametrize("target,fault", [
    ("conv2d_1", _fault_dropped_term), ("conv2d_2", _fault_truncation), ("conv2d_3", _fault_stale_halo),
    ("conv2d_transpose_2", _fault_concat_swapped), ("conv2d_1", _fault_bias_after_rounding),
    ("logits", _fault_logits_from_uncropped_canvas),
], ids=lambda v: v if isinstance(v, str) else v.__name__[7:])
def test_exact_oracle_catches_a_fault_in_its_own_layer_only(oracle_mod, target, fault):
    from oracle import exact
    img, Wt = _setup(oracle_mod, "fcn_skip", 3, (70, 50))
    z, acts = _mutant_forward(oracle_mod, "fcn_skip", Wt, img, target, fault)
    clean = oracle_mod.forward("fcn_skip", Wt, img, "bf16", return_acts=True)[1]
    assert not np.array_equal(acts[target], clean[target])
    layers = exact.evaluate("fcn_skip", Wt, img, acts)
    reps, text = _violations(exact, layers, acts)
    assert len(reps) == len(acts)
    assert reps[target].count >= 1, text
    assert reps[target].worst[0][0] == target and reps[target].worst[0][4] > reps[target].worst[0][5]
    others = {n: r.count for n, r in reps.items() if n != target and r.count}
    assert not others, "%r\n%s" % (others, text)


def test_exact_oracle_check_reports_coordinates_and_nan():
    from oracle import exact
    s = np.zeros((4, 5, 3))
    bound = np.full((4, 5, 3), 0.5)
    g = s.copy()
    g[2, 3, 1], g[1, 4, 0], g[0, 0, 2] = 2.0, -1.0, np.nan
    r = exact.check(g, s, bound, "x")
    assert r.count == 3 and r.ratio == np.inf
    assert set(w[:4] for w in r.worst) == {("x", 2, 3, 1), ("x", 1, 4, 0), ("x", 0, 0, 2)}
    assert r.worst[0][:4] == ("x", 0, 0, 2) and r.worst[1] == ("x", 2, 3, 1, 2.0, 0.5)
    assert exact.check(s, s, np.zeros_like(s), "x") == exact.Report(0, 0.0, [])
    # labels: a wrong label outside the excused band is an error, inside it the runner-up is accepted and nothing else
    z = np.array([[[1.0, 0.0, 0.5], [1.0, 0.9999, 0.0]]])
    b = np.full(z.shape, 1e-3)
    assert exact.check_labels(np.array([[0, 0]]), z, b) == (0, 0.5)
    assert exact.check_labels(np.array([[2, 1]]), z, b) == (1, 0.5)
    assert exact.check_labels(np.array([[0, 2]]), z, b) == (1, 0.5)
