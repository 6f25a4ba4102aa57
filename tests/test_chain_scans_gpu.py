"""pseg_prepare_scans / pseg_predict_chain_scans_png / Engine.predict_chain_scans / Predictor.write_masks_scans: gray scans straight
into the page chain, binarisation and line-height normalisation on the device.

References, all on the same engine: the front end against engine.prepare_images(scan, where(scan > 127, 255, 0), scale) (and the NumPy
oracle); the chain against predict_chain_pages(mixed=True) fed with prepare_images' outputs; the Predictor against
DatasetLoader.load_images + write_masks_dataset.  Every comparison is for equal bytes."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("color", "overlay", "inverted", "fg_color")
LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)


def _text_scan(k, H, W):
    from pseg_amd import synth
    return (255 - synth.synth_page(k, H, W, 3)[0]).astype(np.uint8)        # ink dark, as a scan comes off disk


def _bin255(scan):
    return np.where(scan > 127, 255, 0).astype(np.uint8)


# ---- the front end alone ---------------------------------------------------------------------------------------------------------
# (name, scan, target_line_height, line_height_px): scale = target / line height, the same double in the binding and in the oracle
def _front_cases():
    rng = np.random.default_rng(31)
    noise = lambda H, W: rng.integers(0, 256, (H, W), dtype=np.uint8)
    two = np.where(rng.random((61, 70)) < 0.3, 30, 200).astype(np.uint8)
    return [
        ("both passes, radius 2, tiles cut by both edges", noise(97, 131), 1, 2),
        ("radii 3, no multiple of a tile, a text page", _text_scan(3, 200, 333), 37, 100),
        ("radius 8: the fused cap", noise(130, 90), 1, 5),
        ("radius 23: one pass per launch", noise(300, 260), 2, 25),
        ("no filter launch", noise(64, 48), 1, 1),
        ("upscale", noise(37, 19), 8, 5),
        ("two values: no anti-aliasing", two, 1, 2),
        ("two values under large radii: the copy behind the passes", two, 1, 10),
        ("constant: min = max", np.full((40, 50), 180, np.uint8), 1, 2),
        ("no pixel above 127: all ink", rng.integers(0, 128, (50, 60), dtype=np.uint8), 3, 5),
    ]


def test_front_end_cases_take_every_branch(gpu):
    """The radii the table above promises (host arithmetic of the binding; `gpu`: the library loads behind the fixture's set-up)."""
    from pseg_amd import engine as E
    radii = [(E.scan_plan(c[1].shape, c[2] / c[3])[2][1], E.scan_plan(c[1].shape, c[2] / c[3])[3][1]) for c in _front_cases()]
    assert radii[0] == (2, 2) and radii[2] == (8, 8) and radii[3] == (23, 23) and radii[4] == (0, 0) and radii[5] == (0, 0)
    assert all(3 <= r <= 4 for r in radii[1]) and max(radii[7]) > 8
    assert E.scan_plan((37, 19), 8 / 5)[:2] == (59, 30)


@pytest.fixture(scope="module")
def front_reference(gpu):
    from pseg_amd import engine as E
    return [E.prepare_images(scan, _bin255(scan), t / lh) for _, scan, t, lh in _front_cases()]


def test_prepare_scans_equals_prepare_images(gpu, front_reference):
    from pseg_amd import engine as E
    cases = _front_cases()
    scans, scales = [c[1] for c in cases], [c[2] / c[3] for c in cases]
    # one call holds all scans: per-scan records and weights cannot be swapped unnoticed; twice: no state survives a call
    for run in range(2):
        got = E.prepare_scans(scans, scales)
        assert len(got) == len(cases)
        for (name, scan, _, _), g, w in zip(cases, got, front_reference):
            for part, a, b in zip(("img", "bin", "orig"), g, w):
                assert a.dtype == np.uint8 and a.shape == b.shape, (name, part, run)
                assert np.array_equal(a, b), (name, part, run, int((a != b).sum()))
            assert np.array_equal(g[2], (scan <= 127).astype(np.uint8)), name
    # the scans one by one, and in another order
    for k in (3, 1, 7):
        g = E.prepare_scans([scans[k]], [scales[k]])[0]
        assert all(np.array_equal(a, b) for a, b in zip(g, front_reference[k])), cases[k][0]
    assert E.prepare_scans([], []) == []


def test_prepare_scans_equals_the_oracle(gpu):
    from oracle import resize as oresize
    from pseg_amd import engine as E
    cases = _front_cases()
    got = E.prepare_scans([c[1] for c in cases], [c[2] / c[3] for c in cases])
    for (name, scan, t, lh), g in zip(cases, got):
        want = oresize.prepare_images(scan, _bin255(scan), t, lh)[:3]
        assert all(np.array_equal(a, b) for a, b in zip(g, want)), name


def test_prepare_scans_argument_errors(gpu):
    from pseg_amd import engine as E
    L = gpu.lib()
    scan = _front_cases()[0][1]
    table, keep, plans = E.scan_table([scan], [0.5])
    out = [np.empty(plans[0][:2], np.uint8) for _ in range(2)]
    P = ctypes.c_void_p * 1
    table[0].ry += 1
    assert L.pseg_prepare_scans(0, 1, table, P(out[0].ctypes.data), P(out[1].ctypes.data), None) == -1 and b"radius" in L.pseg_last_error()
    table[0].ry -= 1
    table[0].H = 0
    assert L.pseg_prepare_scans(0, 1, table, P(out[0].ctypes.data), P(out[1].ctypes.data), None) == -1 and b"scan 0" in L.pseg_last_error()
    table[0].H = plans[0][0]
    assert L.pseg_prepare_scans(0, 1, table, P(out[0].ctypes.data), P(None), None) == -1
    assert L.pseg_prepare_scans(0, 1, table, P(out[0].ctypes.data), P(out[1].ctypes.data), None) == 0       # out_orig may be NULL
    want = E.prepare_images(scan, _bin255(scan), 0.5)
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])


# ---- the chain -------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(150, 110), (180, 150), (260, 200), (240, 130), (200, 160), (220, 170)]
SCALES = [0.9, 0.5, 0.5, 0.4, 0.7, 0.4]


def _canvas(s):
    return (-(-s[0] // 32) * 32, -(-s[1] // 32) * 32)


def _page_shapes():
    from pseg_amd import engine as E
    return [E.rescale_shape(s, sc) for s, sc in zip(SCAN_SHAPES, SCALES)]


def test_the_scans_form_units_that_mix_page_shapes(gpu):
    from pseg_amd import engine as E
    pages = _page_shapes()
    assert len(set(SCALES)) == 4 and all(0.4 <= s <= 0.9 for s in SCALES)
    assert all(150 <= s[0] <= 260 and 110 <= s[1] <= 200 for s in SCAN_SHAPES)
    assert len({_canvas(p) for p in pages}) >= 2
    # this is what keeps the byte comparisons below from passing on single-page units
    for cap in (2, 4):                          # (unit_cap 0 is at most 2 for a list of six)
        order, units = E.chain_units_mixed(pages, cap=cap)
        assert any(c >= 2 and len({pages[order[f + k]] for k in range(c)}) >= 2 for f, c in units), (cap, units)
    assert E.chain_units_mixed(pages, cap=4)[0] != list(range(len(pages)))          # the planner's order is not the list's


def _engine(gpu, mode, **kw):
    from pseg_amd import synth
    eng = gpu.Engine("fcn_skip", 3, mode=mode, **kw)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return eng


@pytest.fixture(scope="module")
def engines(gpu):
    engs = {"f32": _engine(gpu, gpu.MODE_F32_EXACT), "bf16": _engine(gpu, gpu.MODE_BF16)}
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def scans(gpu):
    """The scans and, computed once, what prepare_images makes of them: (scan, img, bin, orig) per scan."""
    from pseg_amd import engine as E
    out = []
    for k, (s, sc) in enumerate(zip(SCAN_SHAPES, SCALES)):
        scan = _text_scan(40 + k, s[0], s[1])
        out.append((scan,) + tuple(E.prepare_images(scan, _bin255(scan), sc)))
    return out


def _reference(eng, scans, high_res, **kw):
    return eng.predict_chain_pages([p[1] for p in scans], binaries=[p[3] if high_res else p[2] for p in scans],
                                   out_shapes=[p[0].shape for p in scans] if high_res else None, lut=LUT, mixed=True, **kw)


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_bytes_equal_the_page_chain_fed_with_prepare_images(gpu, engines, scans, mode_name, level):
    eng = engines[mode_name]
    raw = [p[0] for p in scans]
    for posts in ([], ["cc_vote"], ["cc_vote", "bbox"]):
        for high_res in (False, True):
            want = _reference(eng, scans, high_res, post_ops=posts, labels=True, png_level=level, unit_cap=4)
            for cap in (0, 2, 4):
                got = eng.predict_chain_scans(raw, SCALES, high_res=high_res, post_ops=posts, lut=LUT, labels=True, png_level=level, unit_cap=cap)
                assert len(got) == len(scans)
                for k, (g, w) in enumerate(zip(got, want)):
                    at = (k, posts, high_res, cap)
                    assert g["labels"].dtype == np.uint8 and g["labels"].shape == (raw[k].shape if high_res else scans[k][1].shape), at
                    assert g["labels"].tobytes() == w["labels"].tobytes(), at
                    assert sorted(g["masks"]) == ["color", "inverted", "overlay"], at
                    for name in g["masks"]:
                        assert g["masks"][name] == w["masks"][name], at + (name,)
    # mask subsets (the k-th requested mask is not mask k), and labels alone: neither table nor ink map
    for which in (("overlay",), NAMES, ("fg_color", "color")):
        want = _reference(eng, scans, False, post_ops=["cc_vote"], which=which, png_level=level, unit_cap=4)
        got = eng.predict_chain_scans(raw, SCALES, post_ops=["cc_vote"], lut=LUT, which=which, png_level=level, unit_cap=4)
        for g, w in zip(got, want):
            assert g["labels"] is None and sorted(g["masks"]) == sorted(which) and g["masks"] == w["masks"], which
    for high_res in (False, True):
        got = eng.predict_chain_scans(raw, SCALES, high_res=high_res, which=(), labels=True, unit_cap=4)
        bare = eng.predict_chain_pages([p[1] for p in scans], out_shapes=[p[0].shape for p in scans] if high_res else None, which=(), labels=True,
                                       unit_cap=4, mixed=True)
        assert all(g["masks"] == {} and np.array_equal(g["labels"], b["labels"]) for g, b in zip(got, bare))


def test_sink_contract(gpu, engines, scans):
    from pseg_amd import engine as E
    eng = engines["bf16"]
    raw = [p[0] for p in scans]
    n = len(raw)
    kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=4)
    full = eng.predict_chain_scans(raw, SCALES, **kw)
    calls = []
    assert eng.predict_chain_scans(raw, SCALES, sink=lambda page, name, data: calls.append((page, name, data)), **kw) is None
    order, _ = E.chain_units_mixed(_page_shapes(), cap=4)
    names = ["color", "overlay", "inverted", "labels"]
    assert [(c[0], c[1]) for c in calls] == [(p, nm) for p in order for nm in names]          # the planner's order; each output once
    for page, name, data in calls:
        if name == "labels":
            assert np.array_equal(data, full[page]["labels"])
        else:
            assert isinstance(data, bytes) and data == full[page]["masks"][name]

    class Stop(Exception):
        pass

    seen = []

    def raising(page, name, data):
        seen.append((page, name))
        if page == order[3]:
            raise Stop("fourth scan")

    with pytest.raises(Stop, match="fourth scan"):
        eng.predict_chain_scans(raw, SCALES, post_ops=["cc_vote"], lut=LUT, unit_cap=4, sink=raising)
    assert seen == [(p, nm) for p in order[:3] for nm in names[:3]] + [(order[3], "color")]    # nothing behind the call that raised
    again = eng.predict_chain_scans(raw, SCALES, **kw)
    assert all(a["masks"] == f["masks"] and np.array_equal(a["labels"], f["labels"]) for a, f in zip(again, full))
    assert eng.predict_chain_scans([], [], lut=LUT) == []


def test_argument_errors_leave_the_engine_usable(gpu, engines, scans):
    from pseg_amd import engine as E
    L = gpu.lib()
    eng = engines["bf16"]
    raw = [p[0] for p in scans]
    n = len(raw)
    kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=4)
    full = eng.predict_chain_scans(raw, SCALES, **kw)
    table, keep, plans = E.scan_table(raw, SCALES)
    delivered = []
    sink = E.CHAIN_SINK(lambda user, page, which, data, nb: delivered.append(page) or 0)
    ops = (ctypes.c_int * 1)(1)

    def call(h, table, sink):
        return L.pseg_predict_chain_scans_png(h, n, table, ops, 1, 0, LUT.ctypes.data, 3, 0, 7, 4, sink, None)

    # a radius that does not match sigma, in the last scan: refused before the first one is touched
    table[n - 1].rx += 1
    assert call(eng._h, table, sink) == -1 and b"radius" in L.pseg_last_error() and b"scan %d" % (n - 1) in L.pseg_last_error()
    table[n - 1].rx -= 1
    assert call(eng._h, table, ctypes.cast(None, E.CHAIN_SINK)) == -1 and b"sink" in L.pseg_last_error()
    assert call(eng._h, None, sink) == -1
    rgb = _engine(gpu, gpu.MODE_BF16, in_channels=3)
    assert call(rgb._h, table, sink) == -5 and b"one input channel" in L.pseg_last_error()
    with pytest.raises(gpu.PsegError, match="one input channel"):
        rgb.predict_chain_scans(raw, SCALES, lut=LUT)
    rgb.close()
    assert delivered == []
    assert call(eng._h, table, sink) == 0 and sorted(delivered) == sorted(list(range(n)) * 3)
    again = eng.predict_chain_scans(raw, SCALES, **kw)
    assert all(a["masks"] == f["masks"] and np.array_equal(a["labels"], f["labels"]) for a, f in zip(again, full))
    # weights left to the library (NULL: pseg_gaussian_kernel) still run; the radii are then not read
    for k in range(n):
        table[k].wy = table[k].wx = None
        table[k].ry = table[k].rx = 0
    delivered.clear()
    assert call(eng._h, table, sink) == 0 and len(delivered) == 3 * n


# ---- the Predictor ---------------------------------------------------------------------------------------------------------------
TARGET_LINE_HEIGHT = 6


def _line_heights():
    # target / line height gives the scales above: 6 / (6 / scale) with integral line heights where they exist, else the fraction
    return [TARGET_LINE_HEIGHT / s for s in SCALES]


def _predictor(gpu, posts, high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor(p) for p in posts], high_res_output=high_res)
    return Predictor(settings, net), cm


def _entries(tmp_path, scans):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    os.makedirs(str(tmp_path / "scans"), exist_ok=True)
    out = []
    for k, (p, lh) in enumerate(zip(scans, _line_heights())):
        path = str(tmp_path / "scans" / ("scan%d.png" % k))
        Image.fromarray(p[0]).save(path)
        out.append(SingleData(image_path=path, line_height_px=lh))
    return out


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


def _rel(paths_per_page, root):
    return [[os.path.relpath(p, str(root)) for p in paths] for paths in paths_per_page]


def _parent_route(pred, loader, entries, out, level):
    from ocr4all_pixel_classifier.lib.dataset import Dataset
    ds = Dataset([loader.load_images(dataclasses.replace(e)) for e in entries], loader.color_map)
    return list(pred.write_masks_dataset(ds, str(out), level=level))


@pytest.mark.parametrize("high_res", [False, True])
@pytest.mark.parametrize("level", [0, 1])
def test_write_masks_scans(gpu, tmp_path, scans, level, high_res):
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    pred, cm = _predictor(gpu, ["cc_majority"], high_res)
    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)
    entries = _entries(tmp_path, scans)
    want_paths = _parent_route(pred, loader, entries, tmp_path / "parent", level)
    want = _files(want_paths)
    for name, kw in (("whole", {}), ("chunks", {"chunk_pages": 4, "decode_threads": 1})):
        before = [dataclasses.replace(e) for e in entries]
        got_paths = list(pred.write_masks_scans(entries, loader, str(tmp_path / name), level=level, **kw))
        assert _rel(got_paths, tmp_path / name) == _rel(want_paths, tmp_path / "parent"), name
        assert _files(got_paths) == want, name
        assert entries == before, name                                       # not modified on the device path


def test_write_masks_scans_sends_the_right_entries_through_the_fallback(gpu, tmp_path, scans, monkeypatch):
    from ocr4all_pixel_classifier.lib import output
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    pred, cm = _predictor(gpu, ["cc_majority"], False)
    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)
    entries = _entries(tmp_path, scans)[:5]
    entries[1] = dataclasses.replace(entries[1], image=scans[1][0])           # pre-loaded: the reference's binarisation quirk
    entries[3] = dataclasses.replace(entries[3], output_path="third.jpg")     # not a PNG target
    taken = []
    real = pred.network.model.predict_chain_scans
    monkeypatch.setattr(pred.network.model, "predict_chain_scans", lambda s, sc, **kw: taken.append([a.shape for a in s]) or real(s, sc, **kw))
    want_paths = _parent_route(pred, loader, entries, tmp_path / "parent", 0)
    mine = [dataclasses.replace(e) for e in entries]
    got_paths = list(pred.write_masks_scans(mine, loader, str(tmp_path / "scans_out"), level=0))
    assert _rel(got_paths, tmp_path / "scans_out") == _rel(want_paths, tmp_path / "parent")
    assert got_paths[3][0].endswith("third.jpg") and _files(got_paths) == _files(want_paths)
    assert taken == [[SCAN_SHAPES[0], SCAN_SHAPES[2], SCAN_SHAPES[4]]]
    assert mine[0] == entries[0] and mine[1].binary is not None and mine[3].binary is not None        # fallback entries are loaded in place
    # DEVICE_PNG off: every entry falls back
    taken.clear()
    monkeypatch.setattr(output, "DEVICE_PNG", False)
    mine = [dataclasses.replace(e) for e in entries[:2]]
    off_paths = list(pred.write_masks_scans(mine, loader, str(tmp_path / "pil"), level=0))
    assert taken == [] and _rel(off_paths, tmp_path / "pil") == _rel(want_paths[:2], tmp_path / "parent")
    monkeypatch.setattr(output, "DEVICE_PNG", True)
    # a max_width that brings the second stage for the wide pages only: those fall back, the others stay on the device
    pages_w = [p[1].shape[1] for p in scans]
    narrow = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, max_width=sorted(pages_w)[2])
    plain = _entries(tmp_path, scans)
    want_paths = _parent_route(pred, narrow, plain, tmp_path / "parent_narrow", 0)
    got_paths = list(pred.write_masks_scans(plain, narrow, str(tmp_path / "narrow"), level=0))
    assert _rel(got_paths, tmp_path / "narrow") == _rel(want_paths, tmp_path / "parent_narrow") and _files(got_paths) == _files(want_paths)
    assert taken == [[s for s, w in zip(SCAN_SHAPES, pages_w) if w <= sorted(pages_w)[2]]]
    assert [e.binary is not None for e in plain] == [w > sorted(pages_w)[2] for w in pages_w]
