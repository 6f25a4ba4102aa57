"""pseg_binarize_scans / pseg_prepare_scans_bin / pseg_predict_chain_scans_bin_png / Predictor.write_masks_scans(binarize=...) on the
device.  The list entry against the host entry and the NumPy restatement of tests/binarize_cases.py, ink maps and float64
thresholds bit for bit; the front end against engine.prepare_images(scan, where(ink, 0, 255)); the chain against
predict_chain_pages(mixed=True) fed with those arrays; the Predictor against DatasetLoader(binarize=...) + load_images +
write_masks_dataset.  Every comparison is for equal bytes."""
import os

import numpy as np
import pytest

import binarize_cases as C

pytestmark = pytest.mark.gpu

LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)


def _how(gpu, cases):
    return [None if c[2] == 0 else gpu.Sauvola(c[2], c[3], c[4]) for c in cases]


def _edge_cases(gpu):
    """Shapes one below, at and one above every constant of the kernels: the columns a row workgroup owns at a window (segment -
    (window - 1)), the band of rows and the tile of columns of the column kernel, the 16-byte vector; widths that are no multiple
    of 16, so that rows start at every misalignment; radii larger than the image on either axis."""
    from pseg_amd import engine as E
    seg, band, tile, vec = E.binarize_geometry()
    rng = np.random.default_rng(77)
    out = []

    def add(shape, w, k=0.2):
        out.append(("edge %dx%d w=%d" % (shape[0], shape[1], w), C.random_scan(rng, shape, 0.3), w, k, 128.0))

    for w in (3, 15, 255):
        own = seg - (w - 1)
        for W in (own - 1, own, own + 1):
            add((3, W), w)                                     # one segment, exactly one, one and a pixel
        add((2, 2 * own + 1), w)                               # three segments, the last of one column
    for H in (band - 1, band, band + 1, 2 * band, 2 * band + 1):
        add((H, 21), 15)
        add((H, 5), 255)
    for W in (tile - 1, tile, tile + 1, 2 * tile + 1, vec - 1, vec, vec + 1, 3 * vec + 5):
        add((7, W), 15)
        add((band + 3, W), 37)
    add((3, 300), 255)                                         # radius above the height
    add((300, 3), 255)                                         # radius above the width
    add((200, 1), 37)
    add((1, 200), 37)
    return out


@pytest.fixture(scope="module")
def cases(gpu):
    """The cases and, computed once: the restatement, the host entry, the device entry (one list call over all of them)."""
    cs = C.grid_cases() + C.special_cases() + _edge_cases(gpu)
    scans, how = [c[1] for c in cs], _how(gpu, cs)
    want = C.restated(cs)
    host = gpu.binarize_scans(scans, how, host=True, thresholds=True)
    dev = gpu.binarize_scans(scans, how, thresholds=True)
    return cs, want, host, dev


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_device_equals_host_equals_restatement(gpu, cases):
    cs, want, host, dev = cases
    assert len(cs) > 360 and len(dev) == len(cs)
    for c, w, h, d in zip(cs, want, host, dev):
        assert d[0].dtype == np.uint8 and d[1].dtype == np.float64 and d[0].shape == d[1].shape == c[1].shape, c[0]
        assert np.array_equal(h[0], w[0]) and np.array_equal(h[1], w[1]), ("host", c[0])
        assert np.array_equal(d[0], w[0]), ("ink", c[0], int((d[0] != w[0]).sum()))
        assert np.array_equal(d[1], w[1]), ("threshold", c[0], int((d[1] != w[1]).sum()), float(np.abs(d[1] - w[1]).max()))


def test_lists_and_groups(gpu, cases):
    cs, want, _, _ = cases
    rng = np.random.default_rng(5)
    # 70 scans: two groups; mixed windows, fixed and adaptive entries in one list
    pick = [int(k) for k in rng.permutation(len(cs))[:70]]
    sub = [cs[k] if j % 5 else (cs[k][0], cs[k][1], 0, 0.0, 0.0) for j, k in enumerate(pick)]
    ref = [want[k] if j % 5 else C.fixed(cs[k][1]) for j, k in enumerate(pick)]
    assert len({c[2] for c in sub}) >= 4 and 0 in {c[2] for c in sub}
    scans, how = [c[1] for c in sub], _how(gpu, sub)
    for run in range(2):                                       # twice: the workspace is reused
        got = gpu.binarize_scans(scans, how, thresholds=True)
        assert all(_same(g, r) for g, r in zip(got, ref)), run
    assert gpu.lib().pseg_release_workspace(0) == 0             # the workspace goes and comes back
    # without thresholds; in another order; each scan alone
    assert all(np.array_equal(g, r[0]) for g, r in zip(gpu.binarize_scans(scans, how), ref))
    order = [int(k) for k in rng.permutation(70)]
    got = gpu.binarize_scans([scans[k] for k in order], [how[k] for k in order], thresholds=True)
    assert all(_same(g, ref[k]) for g, k in zip(got, order))
    for k in range(70):
        assert _same(gpu.binarize_scans([scans[k]], [how[k]], thresholds=True)[0], ref[k]), sub[k][0]
    # thresholds for some scans only (the C entry takes NULL entries): covered with the refusals
    C.refusals(gpu.lib(), False)
    assert gpu.binarize_scans([], gpu.Sauvola(15)) == []


def test_the_unevenly_lit_page(gpu):
    gray, glyph, line_height = C.uneven_page()
    how = gpu.Sauvola().resolved(line_height)
    ink, T = gpu.binarize_scans([gray], how, thresholds=True)[0]
    rink, rT = C.sauvola(gray, how.window)
    assert np.array_equal(ink, rink) and np.array_equal(T, rT)
    assert (ink != glyph).mean() <= 0.005


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def _front_cases():
    """(name, scan, target_line_height, line_height_px, window): as tests/test_chain_scans_gpu.py's table, unevenly lit."""
    rng = np.random.default_rng(31)
    noise = lambda H, W: rng.integers(0, 256, (H, W), dtype=np.uint8)
    return [
        ("both passes, radius 2, tiles cut by both edges", noise(97, 131), 1, 2, 15),
        ("radii 3, a lit text page", C.lit_text_scan(3, 200, 333), 37, 100, 33),
        ("radius 8: the fused cap", noise(130, 90), 1, 5, 255),
        ("radius 23: one pass per launch", C.lit_text_scan(4, 300, 260), 2, 25, 61),
        ("no filter launch", C.lit_text_scan(5, 64, 48), 1, 1, 21),
        ("upscale", noise(37, 19), 8, 5, 37),
        ("fixed entry in the list", noise(61, 70), 1, 2, 0),
    ]


def test_prepare_scans_equals_prepare_images_of_the_adaptive_map(gpu):
    from pseg_amd import engine as E
    cases = _front_cases()
    radii = [max(E.scan_plan(c[1].shape, c[2] / c[3])[2][1], E.scan_plan(c[1].shape, c[2] / c[3])[3][1]) for c in cases]
    assert radii[0] == 2 and radii[2] == 8 and radii[3] == 23 and radii[4] == 0 and radii[5] == 0      # every path of the front end
    scans, scales = [c[1] for c in cases], [c[2] / c[3] for c in cases]
    how = [gpu.Sauvola(c[4]) if c[4] else None for c in cases]
    inks = [C.sauvola(c[1], c[4])[0] if c[4] else C.fixed(c[1])[0] for c in cases]
    assert any((i != (s <= 127)).mean() > 0.05 for i, s in zip(inks, scans))          # the adaptive map is another map
    want = [E.prepare_images(s, np.where(i != 0, 0, 255).astype(np.uint8), sc) for s, i, sc in zip(scans, inks, scales)]
    for run in range(2):
        got = E.prepare_scans(scans, scales, binarize=how)
        for c, g, w, i in zip(cases, got, want, inks):
            for part, a, b in zip(("img", "bin", "orig"), g, w):
                assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (c[0], part, run, int((a != b).sum()))
            assert np.array_equal(g[2], i), c[0]
    for k in (3, 1):                                           # alone
        g = E.prepare_scans([scans[k]], [scales[k]], binarize=how[k])[0]
        assert all(np.array_equal(a, b) for a, b in zip(g, want[k])), cases[k][0]
    # binarize=None, and entries of window 0, are today's call
    today = E.prepare_scans(scans, scales)
    for other in (E.prepare_scans(scans, scales, binarize=None), E.prepare_scans(scans, scales, binarize=[None] * len(scans))):
        assert all(np.array_equal(a, b) for g, t in zip(other, today) for a, b in zip(g, t))


# ---- the chain -------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(150, 110), (180, 150), (256, 200), (240, 130), (200, 160), (220, 170)]
SCALES = [0.9, 0.5, 0.5, 0.4, 0.7, 0.4]
WINDOWS = [15, 33, 0, 61, 255, 21]                             # scan 2 keeps the fixed threshold


def _engine(gpu, mode):
    from pseg_amd import synth
    eng = gpu.Engine("fcn_skip", 3, mode=mode)
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
    """The scans and, computed once, what prepare_images makes of them and their adaptive maps: (scan, img, bin, orig) per scan."""
    from pseg_amd import engine as E
    out = []
    for k, (s, sc, w) in enumerate(zip(SCAN_SHAPES, SCALES, WINDOWS)):
        scan = C.lit_text_scan(40 + k, s[0], s[1])
        ink = C.sauvola(scan, w)[0] if w else C.fixed(scan)[0]
        out.append((scan,) + tuple(E.prepare_images(scan, np.where(ink != 0, 0, 255).astype(np.uint8), sc)))
    return out


def _chain_how(gpu):
    return [gpu.Sauvola(w) if w else None for w in WINDOWS]


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_chain_bytes_equal_the_page_chain_fed_with_the_adaptive_maps(gpu, engines, scans, mode_name, level):
    eng = engines[mode_name]
    raw = [p[0] for p in scans]
    how = _chain_how(gpu)
    for posts in (["cc_vote"], ["cc_vote", "bbox"]):
        for high_res in (False, True):
            want = eng.predict_chain_pages([p[1] for p in scans], binaries=[p[3] if high_res else p[2] for p in scans],
                                           out_shapes=[p[0].shape for p in scans] if high_res else None, lut=LUT, mixed=True, post_ops=posts,
                                           labels=True, png_level=level, unit_cap=2)
            for cap in (0, 2):
                got = eng.predict_chain_scans(raw, SCALES, high_res=high_res, post_ops=posts, lut=LUT, labels=True, png_level=level, unit_cap=cap,
                                              binarize=how)
                assert len(got) == len(scans)
                for k, (g, w) in enumerate(zip(got, want)):
                    at = (k, posts, high_res, cap)
                    assert g["labels"].tobytes() == w["labels"].tobytes(), at
                    assert sorted(g["masks"]) == ["color", "inverted", "overlay"], at
                    for name in g["masks"]:
                        assert g["masks"][name] == w["masks"][name], at + (name,)
    if mode_name == "bf16" and level == 0:
        # the adaptive map changes the output (the comparison above has teeth); None and window 0 are today's call
        kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2)
        today = eng.predict_chain_scans(raw, SCALES, **kw)
        adaptive = eng.predict_chain_scans(raw, SCALES, binarize=how, **kw)
        assert any(a["masks"]["inverted"] != t["masks"]["inverted"] for a, t in zip(adaptive, today))
        assert adaptive[2]["masks"] == today[2]["masks"]        # the fixed entry
        for other in (eng.predict_chain_scans(raw, SCALES, binarize=None, **kw), eng.predict_chain_scans(raw, SCALES, binarize=[None] * len(raw), **kw)):
            assert all(o["masks"] == t["masks"] and np.array_equal(o["labels"], t["labels"]) for o, t in zip(other, today))
        # labels alone: no ink map is needed, none is made
        bare = eng.predict_chain_scans(raw, SCALES, which=(), labels=True, unit_cap=2)
        got = eng.predict_chain_scans(raw, SCALES, which=(), labels=True, unit_cap=2, binarize=how)
        assert all(np.array_equal(g["labels"], b["labels"]) for g, b in zip(got, bare))
        with pytest.raises(gpu.PsegError, match="scan 1"):
            eng.predict_chain_scans(raw, SCALES, lut=LUT, binarize=[how[0], _even(), *how[2:]])
        again = eng.predict_chain_scans(raw, SCALES, binarize=how, **kw)
        assert all(a["masks"] == f["masks"] for a, f in zip(again, adaptive))


def _even():
    """A Sauvola the constructor would refuse: the library's own check has to catch it."""
    import pseg_amd
    s = pseg_amd.Sauvola(15)
    s.window = 14
    return s


# ---- the Predictor ---------------------------------------------------------------------------------------------------------------
TARGET_LINE_HEIGHT = 6
FILE_SHAPES = [(256, 200), (240, 230), (250, 250), (200, 256)]


def _predictor(gpu, high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=high_res)
    return Predictor(settings, net), cm


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


def _rel(paths_per_page, root):
    return [[os.path.relpath(p, str(root)) for p in paths] for paths in paths_per_page]


@pytest.mark.parametrize("high_res", [False, True])
def test_write_masks_scans_with_a_binarisation(gpu, tmp_path, high_res):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import Dataset, DatasetLoader, SingleData
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    files = []
    for k, s in enumerate(FILE_SHAPES):
        files.append(str(tmp_path / ("scan%d.png" % k)))
        Image.fromarray(C.lit_text_scan(60 + k, s[0], s[1])).save(files[-1])
    heights = [compute_char_height(f, False) for f in files]
    assert all(isinstance(h, int) for h in heights)
    pred, cm = _predictor(gpu, high_res)
    how = gpu.Sauvola()                                        # the window comes from each entry's line height

    def entries(measured):
        # entry 1 has no line height (measured in the call), entry 2 is no PNG target (the fallback route)
        return [SingleData(image_path=f, line_height_px=(h if measured or k != 1 else None), output_path=("third.jpg" if k == 2 else None))
                for k, (f, h) in enumerate(zip(files, heights))]

    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, binarize=how)
    loaded = [loader.load_images(e) for e in entries(True)]
    for e, f, h in zip(loaded, files, heights):                # the records carry the adaptive map
        gray = np.asarray(Image.open(f).convert("L"))
        assert np.array_equal(e.orig_binary, C.sauvola(gray, gpu.sauvola_window(h))[0])
    want_paths = list(pred.write_masks_dataset(Dataset(loaded, cm), str(tmp_path / "parent"), level=0))
    want = _files(want_paths)
    plain = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)      # the call's binarize, not the loader's, decides
    for name, kw in (("whole", {}), ("chunks", {"chunk_pages": 3, "decode_threads": 1})):
        mine = entries(False)
        got_paths = list(pred.write_masks_scans(mine, plain, str(tmp_path / name), level=0, binarize=how, **kw))
        assert _rel(got_paths, tmp_path / name) == _rel(want_paths, tmp_path / "parent"), name
        assert got_paths[2][0].endswith("third.jpg") and _files(got_paths) == want, name
        assert mine[1].line_height_px == heights[1] and mine[2].binary is not None and mine[0].binary is None, name
    # and it is another result than today's
    today = _files(list(pred.write_masks_scans(entries(True), plain, str(tmp_path / "today"), level=0)))
    assert today != want
