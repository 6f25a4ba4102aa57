"""The bf16 MFMA engine, layer by layer, against exact float64 sums with a DERIVED bound (oracle/exact.py): every layer of the
oracle graph is fed with the engine's own stored input tensors and evaluated exactly, so the engine's output may differ only
by float32 accumulation error (gamma_K with the truncation-safe u = 2^-23) plus one rounding to bf16 (2^-8), per element.  A
fault in layer L shows at layer L, at the pixels where it happens: no 2 %-of-the-maximum bar, no error inherited from earlier
layers, and no tolerance taken from the engine's own error -- the label rule uses the exact logits' margin and bound.

Three engines per case: (a) every tensor stored (all fusions of mfma_plan_graph switched off), (b) the same on the generic
kernels only (PSEG_GENERIC: what every bit-identity test is anchored to), (c) the default plan, where a fused group is checked
at its outputs with the group's wider, still derived bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STORE_ALL = ("PSEG_NO_TAIL_FUSION", "PSEG_NO_CONV1_FUSION", "PSEG_NO_DQ", "PSEG_NO_POOL_ONLY", "PSEG_NO_SKIPLOG", "PSEG_NO_TAIL2",
             "PSEG_NO_RELU_FWD", "PSEG_NO_TAIL_COMPOSE")
ENGINES = (("stored", STORE_ALL), ("generic", STORE_ALL + ("PSEG_GENERIC",)), ("default", ()))
EXCUSED_CAP = 0.02

CASES = [
    ("fcn_skip", 3, (64, 96), 1, False), ("fcn_skip", 3, (70, 50), 1, False), ("fcn_skip", 3, (33, 1), 1, False),
    ("fcn_skip", 3, (160, 96), 1, False), ("fcn_skip", 3, (256, 320), 1, False), ("fcn_skip", 6, (130, 67), 1, False),
    ("fcn_skip", 20, (64, 96), 1, False), ("fcn_skip", 3, (70, 50), 3, False),
    ("fcn", 3, (96, 64), 1, False), ("fcn", 3, (300, 420), 1, False),          # the 1/8-resolution map has several 8 x 24 tiles
    ("unet", 3, (64, 96), 1, False), ("unet", 40, (32, 64), 1, False),
    ("res_unet", 3, (70, 50), 1, False), ("res_unet", 3, (96, 160), 1, False), ("res_unet", 3, (64, 96), 1, True),
]


def _read(gpu, eng, name):
    """The engine's tensor, or None where the plan never writes it as such (inside a fused kernel / stored after a ReLU)."""
    try:
        return eng.activation(name)
    except gpu.PsegError as ex:
        assert "fused" in str(ex), ex          # both refusals say so: "fused into its consumer", "fused with its readers' pre-activation ReLU"
        return None


def _engine_tensors(gpu, eng, exact, img, layers):
    """{oracle layer name: engine tensor} for every layer the engine has.  A BatchNormalization over a concat is two engine ops
    ("name" on the first source, at that source's resolution, and "name+C0" on the second): the oracle's tensor is their concat."""
    forced = {}
    try:
        forced["input"] = eng.activation("input")
    except gpu.PsegError:
        forced["input"] = exact.input_canvas(img)
    for name, l in layers.items():
        if name == "logits":
            continue
        g = _read(gpu, eng, name)
        if g is not None and g.shape[2] < l.s.shape[2]:
            g1 = _read(gpu, eng, "%s+%d" % (name, g.shape[2]))
            if g1 is not None and g.shape[0] * 2 == g1.shape[0]:
                g = np.repeat(np.repeat(g, 2, axis=0), 2, axis=1)
            g = np.concatenate([g, g1], -1) if g1 is not None else None
        if g is not None:
            forced[name] = g
    return forced


@pytest.mark.parametrize("arch,C,shape,in_ch,bn", CASES)
def test_bf16_layers_inside_the_derived_bound(gpu, oracle_mod, monkeypatch, arch, C, shape, in_ch, bn):
    from oracle import exact
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=shape + ((3,) if in_ch == 3 else ()), dtype=np.uint8)
    Wt = oracle_mod.init_weights(arch, C, seed=42, in_ch=in_ch, gain=1.5, bias_scale=0.05, batch_norm=bn)
    names = exact.evaluate(arch, Wt, img[:1, :1], {})              # the op list of the graph, with channel counts (one pixel: cheap)
    failures, ratios = [], []
    for label, switches in ENGINES:
        for k in switches:
            monkeypatch.setenv(k, "1")
        eng = gpu.Engine(arch, C, in_channels=in_ch, mode=gpu.MODE_BF16, batch_norm=bn)
        for k in switches:
            monkeypatch.delenv(k)
        eng.set_weights(Wt)
        logit, _, pred = eng.predict(img, want_probs=False)
        forced = _engine_tensors(gpu, eng, exact, img, names)
        eng.close()
        assert np.array_equal(forced["input"], exact.input_canvas(img)), "%s: the input canvas" % label
        layers = exact.evaluate(arch, Wt, img, forced)
        forced["logits"] = logit
        reps = {n: exact.check(forced[n], l.s, l.bound, n) for n, l in layers.items() if n in forced}
        text = "%s-%d-%dx%d-in%d%s %s: max error / bound per layer: " % (arch, C, shape[0], shape[1], in_ch, "-bn" if bn else "", label) + \
               " ".join("%s %.3f" % (n, r.ratio) for n, r in reps.items())
        print(text)
        ratios.append(text)
        for n, r in reps.items():
            if r.count:
                failures.append("%s, %s: %d of %d elements over the bound; worst (layer, y, x, channel, error, bound): %r"
                                % (label, n, r.count, layers[n].s.size, r.worst))
        absent = [n for n in layers if n not in forced]
        if label != "default":
            # every op's output is there and was checked on forced inputs alone
            assert not absent and len(reps) == len(layers), "%s: not stored: %r" % (label, absent)
            assert all(l.all_forced for l in layers.values()), label
        else:
            # every absent tensor lies inside a group whose outputs are checked: it has readers, and they are checked or inside too
            readers = {n: [m for m, l in layers.items() if n in l.inputs] for n in absent}
            assert all(readers[n] for n in absent), readers
            assert "logits" in reps
        # labels: from the exact forced logits, their margin and their bound -- nothing from the engine's own error
        lg = layers["logits"]
        assert np.array_equal(pred, np.argmax(logit, -1)), label
        wrong, excused = exact.check_labels(pred, lg.s, lg.bound)
        print("%s: labels wrong %d, excused share %.5f" % (label, wrong, excused))
        if wrong:
            failures.append("%s: %d labels differ from argmax of the exact logits outside the excused band" % (label, wrong))
        if label != "default":
            assert excused <= EXCUSED_CAP, "%s: %.4f of the page inside the margin band" % (label, excused)
    assert not failures, "\n".join(failures + ratios)
