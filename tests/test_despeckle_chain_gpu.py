"""pseg_prepare_scans_clean / pseg_predict_chain_scans_clean_png / Predictor.write_masks_scans(despeckle=...) /
DatasetLoader(despeckle=...) on the device.  The front end against engine.prepare_images(scan, where(clean, 0, 255)) with clean =
despeckle_maps of the scan's ink map; the chain against predict_chain_pages(mixed=True) fed with those arrays; the Predictor against
DatasetLoader(despeckle=...) + load_images + write_masks_dataset; load_data_list against load_data; one page with planted specks.
Every comparison is for equal bytes."""
import ctypes
import os

import numpy as np
import pytest

import binarize_cases as B
import despeckle_cases as C

pytestmark = pytest.mark.gpu

LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)


def _scan(seed, H, W, salt=0.004):
    """A synthetic text scan (ink dark) with dust: its two textured rectangles break into specks under either threshold, and a share
    `salt` of its pixels is dark."""
    from pseg_amd import synth
    scan = (255 - synth.synth_page(seed, H, W, 3)[0]).astype(np.uint8)
    scan[np.random.default_rng(7000 + seed).random((H, W)) < salt] = 10
    return scan


def _ink(scan, window):
    return B.sauvola(scan, window)[0] if window else B.fixed(scan)[0]


def _clean(gpu, scan, window, d):
    """The despeckled ink map of a scan, from the list entry (tests/test_despeckle_gpu.py holds it to the restatement)."""
    ink = _ink(scan, window)
    return ink if d is None else gpu.despeckle_maps([ink], d)[0]


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def _front_cases(gpu):
    """(name, scan, target_line_height, line_height_px, window, despeckle): every path of the front end, both thresholds."""
    rng = np.random.default_rng(31)
    noise = lambda H, W: rng.integers(0, 256, (H, W), dtype=np.uint8)
    D = gpu.Despeckle
    return [
        ("both passes, radius 2, tiles cut by both edges", noise(97, 131), 1, 2, 0, D(3, 8)),
        ("radii 3, a text page", _scan(3, 200, 333), 37, 100, 33, D(9, 8)),
        ("radius 8: the fused cap", noise(130, 90), 1, 5, 0, D(2, 4)),
        ("radius 23: one pass per launch", _scan(4, 300, 260), 2, 25, 0, D(16, 8)),
        ("radius 23, adaptive", _scan(6, 290, 250), 2, 25, 61, D(16, 4)),
        ("no filter launch", noise(64, 48), 1, 1, 21, D(4, 8)),
        ("upscale", noise(37, 19), 8, 5, 0, D(5, 8)),
        ("two values", np.where(rng.random((90, 150)) < 0.3, 30, 200).astype(np.uint8), 1, 2, 0, D(6, 8)),
        ("two values, adaptive", np.where(rng.random((77, 140)) < 0.4, 30, 200).astype(np.uint8), 1, 3, 15, D(3, 4)),
        ("not despeckled, in the list", noise(61, 70), 1, 2, 0, None),
    ]


def test_prepare_scans_equals_prepare_images_of_the_despeckled_map(gpu):
    from pseg_amd import engine as E
    cases = _front_cases(gpu)
    radii = [max(E.scan_plan(c[1].shape, c[2] / c[3])[2][1], E.scan_plan(c[1].shape, c[2] / c[3])[3][1]) for c in cases]
    assert radii[0] == 2 and radii[2] == 8 and radii[3] == 23 and radii[5] == 0 and radii[6] == 0       # every path of the front end
    scans, scales = [c[1] for c in cases], [c[2] / c[3] for c in cases]
    how = [gpu.Sauvola(c[4]) if c[4] else None for c in cases]
    dsp = [c[5] for c in cases]
    cleans = [_clean(gpu, c[1], c[4], c[5]) for c in cases]
    for c, cl in zip(cases, cleans):                            # the yardstick is the restatement's map, and it is another map than the ink
        if c[5] is not None:
            assert np.array_equal(cl, C.restated(_ink(c[1], c[4]), c[5].max_area, c[5].connectivity)[0]), c[0]
            assert (cl != _ink(c[1], c[4])).sum() > 0, c[0]
    want = [E.prepare_images(s, np.where(cl != 0, 0, 255).astype(np.uint8), sc) for s, cl, sc in zip(scans, cleans, scales)]
    for run in range(2):
        got = E.prepare_scans(scans, scales, binarize=how, despeckle=dsp)
        for c, g, w, cl in zip(cases, got, want, cleans):
            for part, a, b in zip(("img", "bin", "orig"), g, w):
                assert a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (c[0], part, run, int((a != b).sum()))
            assert np.array_equal(g[2], cl), c[0]
    for k in (3, 1, 7):                                        # alone
        g = E.prepare_scans([scans[k]], [scales[k]], binarize=how[k], despeckle=dsp[k])[0]
        assert all(np.array_equal(a, b) for a, b in zip(g, want[k])), cases[k][0]
    # out_orig not asked for: the ink plane lives in the workspace; page and ink map are the same bytes
    n = len(cases)
    table, keep, plans = E.scan_table(scans, scales)
    out = [[np.full(p[:2], 0xA5, np.uint8) for p in plans] for _ in range(2)]
    P = ctypes.c_void_p * n
    for orig in (None, P(*([None] * n))):
        assert E.lib().pseg_prepare_scans_clean(0, n, table, E.binarize_table(how, n), E.despeckle_table(dsp, n), P(*[o.ctypes.data for o in out[0]]),
                                                P(*[o.ctypes.data for o in out[1]]), orig) == 0
        for k, w in enumerate(want):
            assert np.array_equal(out[0][k], w[0]) and np.array_equal(out[1][k], w[1]), cases[k][0]
    # despeckle=None, and entries that are None, are the call without the argument
    today = E.prepare_scans(scans, scales, binarize=how)
    for other in (E.prepare_scans(scans, scales, binarize=how, despeckle=None), E.prepare_scans(scans, scales, binarize=how, despeckle=[None] * n)):
        assert all(np.array_equal(a, b) for g, t in zip(other, today) for a, b in zip(g, t))
    assert any(not np.array_equal(g[1], t[1]) for g, t in zip(got, today))


# ---- the chain -------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(150, 110), (180, 150), (256, 200), (240, 130), (200, 160), (220, 170)]
SCALES = [0.9, 0.5, 0.5, 0.4, 0.7, 0.4]
WINDOWS = [0, 33, 0, 61, 0, 21]
AREAS = [(4, 8), (9, 8), None, (6, 4), (12, 4), (3, 8)]         # scan 2 is not despeckled


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


def _chain_how(gpu):
    return [gpu.Sauvola(w) if w else None for w in WINDOWS], [gpu.Despeckle(*a) if a else None for a in AREAS]


@pytest.fixture(scope="module")
def scans(gpu):
    """The scans and, computed once, what prepare_images makes of them and their despeckled maps: (scan, img, bin, orig) per scan."""
    from pseg_amd import engine as E
    dsp = _chain_how(gpu)[1]
    out = []
    for k, (s, sc, w) in enumerate(zip(SCAN_SHAPES, SCALES, WINDOWS)):
        scan = _scan(40 + k, s[0], s[1])
        clean = _clean(gpu, scan, w, dsp[k])
        out.append((scan,) + tuple(E.prepare_images(scan, np.where(clean != 0, 0, 255).astype(np.uint8), sc)))
    return out


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_chain_bytes_equal_the_page_chain_fed_with_the_despeckled_maps(gpu, engines, scans, mode_name, level):
    eng = engines[mode_name]
    raw = [p[0] for p in scans]
    how, dsp = _chain_how(gpu)
    for posts in (["cc_vote"], ["cc_vote", "bbox"]):
        for high_res in (False, True):
            want = eng.predict_chain_pages([p[1] for p in scans], binaries=[p[3] if high_res else p[2] for p in scans],
                                           out_shapes=[p[0].shape for p in scans] if high_res else None, lut=LUT, mixed=True, post_ops=posts,
                                           labels=True, png_level=level, unit_cap=2)
            for cap in (0, 2):
                got = eng.predict_chain_scans(raw, SCALES, high_res=high_res, post_ops=posts, lut=LUT, labels=True, png_level=level, unit_cap=cap,
                                              binarize=how, despeckle=dsp)
                assert len(got) == len(scans)
                for k, (g, w) in enumerate(zip(got, want)):
                    at = (k, posts, high_res, cap)
                    assert g["labels"].tobytes() == w["labels"].tobytes(), at
                    assert sorted(g["masks"]) == ["color", "inverted", "overlay"], at
                    for name in g["masks"]:
                        assert g["masks"][name] == w["masks"][name], at + (name,)
    if mode_name == "bf16" and level == 0:
        # the despeckling changes the output (the comparison above has teeth); None is the call without the argument
        kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2, binarize=how)
        today = eng.predict_chain_scans(raw, SCALES, **kw)
        clean = eng.predict_chain_scans(raw, SCALES, despeckle=dsp, **kw)
        assert sum(a["masks"]["inverted"] != t["masks"]["inverted"] for a, t in zip(clean, today)) >= 4
        assert clean[2]["masks"] == today[2]["masks"]           # the entry that is not despeckled
        for other in (eng.predict_chain_scans(raw, SCALES, despeckle=None, **kw), eng.predict_chain_scans(raw, SCALES, despeckle=[None] * len(raw), **kw)):
            assert all(o["masks"] == t["masks"] and np.array_equal(o["labels"], t["labels"]) for o, t in zip(other, today))
        # labels alone: no ink map is needed, none is made or cleaned
        bare = eng.predict_chain_scans(raw, SCALES, which=(), labels=True, unit_cap=2)
        got = eng.predict_chain_scans(raw, SCALES, which=(), labels=True, unit_cap=2, binarize=how, despeckle=dsp)
        assert all(np.array_equal(g["labels"], b["labels"]) for g, b in zip(got, bare))
        with pytest.raises(gpu.PsegError, match="scan 1"):
            eng.predict_chain_scans(raw, SCALES, lut=LUT, despeckle=[dsp[0], _conn3(), *dsp[2:]])
        again = eng.predict_chain_scans(raw, SCALES, despeckle=dsp, **kw)
        assert all(a["masks"] == f["masks"] for a, f in zip(again, clean))


def _conn3():
    """A Despeckle the constructor would refuse: the library's own check has to catch it."""
    import pseg_amd
    d = pseg_amd.Despeckle(4)
    d.connectivity = 3
    return d


# ---- the Predictor and the loaders ----------------------------------------------------------------------------------------------------
TARGET_LINE_HEIGHT = 6
FILE_SHAPES = [(256, 200), (240, 230), (250, 250), (200, 256)]


def _color_map():
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    return ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})


def _predictor(gpu, high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = _color_map()
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=high_res)
    return Predictor(settings, net), cm


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


def _rel(paths_per_page, root):
    return [[os.path.relpath(p, str(root)) for p in paths] for paths in paths_per_page]


@pytest.mark.parametrize("high_res", [False, True])
def test_write_masks_scans_with_a_despeckling(gpu, tmp_path, high_res):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import Dataset, DatasetLoader, SingleData
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    files = []
    for k, s in enumerate(FILE_SHAPES):
        files.append(str(tmp_path / ("scan%d.png" % k)))
        Image.fromarray(_scan(60 + k, s[0], s[1])).save(files[-1])
    heights = [compute_char_height(f, False) for f in files]
    assert all(isinstance(h, int) for h in heights)
    pred, cm = _predictor(gpu, high_res)
    d = gpu.Despeckle()                                        # max_area comes from each entry's line height
    assert all(gpu.despeckle_area(h) >= 1 for h in heights)

    def entries(measured):
        # entry 1 has no line height (measured in the call), entry 2 is no PNG target (the fallback route)
        return [SingleData(image_path=f, line_height_px=(h if measured or k != 1 else None), output_path=("third.jpg" if k == 2 else None))
                for k, (f, h) in enumerate(zip(files, heights))]

    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, despeckle=d)
    loaded = [loader.load_images(e) for e in entries(True)]
    for e, f, h in zip(loaded, files, heights):                # the records carry the despeckled map
        gray = np.asarray(Image.open(f).convert("L"))
        assert np.array_equal(e.orig_binary, C.restated(gray <= 127, gpu.despeckle_area(h), 8)[0])
    want_paths = list(pred.write_masks_dataset(Dataset(loaded, cm), str(tmp_path / "parent"), level=0))
    want = _files(want_paths)
    plain = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)      # the call's despeckle, not the loader's, decides
    for name, kw in (("whole", {}), ("chunks", {"chunk_pages": 3, "decode_threads": 1})):
        mine = entries(False)
        got_paths = list(pred.write_masks_scans(mine, plain, str(tmp_path / name), level=0, despeckle=d, **kw))
        assert _rel(got_paths, tmp_path / name) == _rel(want_paths, tmp_path / "parent"), name
        assert got_paths[2][0].endswith("third.jpg") and _files(got_paths) == want, name
        assert mine[1].line_height_px == heights[1] and mine[2].binary is not None and mine[0].binary is None, name
    # and it is another result than today's; despeckle=None is today's call
    today = _files(list(pred.write_masks_scans(entries(True), plain, str(tmp_path / "today"), level=0)))
    assert today != want
    assert _files(list(pred.write_masks_scans(entries(True), plain, str(tmp_path / "none"), level=0, despeckle=None))) == today
    # with a binarisation as well
    s = gpu.Sauvola()
    both = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, binarize=s, despeckle=d)
    want2 = _files(list(pred.write_masks_dataset(Dataset([both.load_images(e) for e in entries(True)], cm), str(tmp_path / "parent2"), level=0)))
    assert _files(list(pred.write_masks_scans(entries(False), plain, str(tmp_path / "both"), level=0, binarize=s, despeckle=d))) == want2


FIELDS = ("image", "binary", "orig_binary", "mask")


def test_load_data_list_equals_load_data_with_a_despeckling(gpu, tmp_path):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    from pseg_amd import synth
    spec = [((150, 101), 9, "list"), ((120, 90), 10, "preloaded"), ((80, 219), 3, "max_width"), ((260, 200), None, "unmeasured"), ((201, 160), 13, "list")]
    made = []
    for k, (shape, lh, kind) in enumerate(spec):
        img, _, ids = synth.synth_page(60 if kind == "unmeasured" else 20 + k, shape[0], shape[1], 3)
        scan_path, mask_path = str(tmp_path / ("scan%d.png" % k)), str(tmp_path / ("mask%d.png" % k))
        Image.fromarray((255 - img).astype(np.uint8)).save(scan_path)
        Image.fromarray(LUT[ids]).save(mask_path)
        made.append((kind, scan_path, mask_path, lh, (255 - img).astype(np.uint8), ids.astype(np.uint8)))
    measured = compute_char_height(made[3][1], False)
    assert isinstance(measured, int)

    def make(measure):
        out = []
        for kind, scan_path, mask_path, lh, scan, ids in made:
            e = SingleData(image_path=scan_path, mask_path=mask_path, line_height_px=lh if lh is not None or not measure else measured)
            if kind == "preloaded":
                e.image, e.mask = scan.copy(), ids.copy()
            out.append(e)
        return out

    for binarize in (None, gpu.Sauvola()):
        loader = lambda d: DatasetLoader(TARGET_LINE_HEIGHT, _color_map(), max_width=400, binarize=binarize, despeckle=d)
        d = gpu.Despeckle(connectivity=4)
        want = loader(d).load_data(make(True))
        report = []
        got = loader(d).load_data_list(make(False), chunk=3, report=report)
        assert [r is None for r in report] == [False, True, True, False, False]      # the pre-loaded image and the wide scan took load_images' route
        for k, (g, w) in enumerate(zip(got.data, want.data)):
            for f in FIELDS:
                a, b = getattr(g, f), getattr(w, f)
                assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, f)
            assert tuple(g.original_shape) == tuple(w.original_shape) and g.line_height_px == w.line_height_px, k
        # the despeckling reached the records of both routes that derive the ink map from the file
        plain = loader(None).load_data(make(True))
        assert [not np.array_equal(a.orig_binary, b.orig_binary) for a, b in zip(want.data, plain.data)] == [True, False, True, True, True]


# ---- a page with planted specks ----------------------------------------------------------------------------------------------------
def speck_page(seed=12, H=300, W=260):
    """-> (scan uint8, ink map, glyphs, specks, speck pixels): blocks of glyph boxes on paper, and one- to four-pixel specks planted
    at least three pixels from every glyph and from each other."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    glyph = np.zeros((H, W), bool)
    n_glyphs = 0
    for top, left, rows, cols in ((20, 16, 5, 14), (150, 40, 6, 11)):
        for r in range(rows):
            for c in range(cols):
                y, x = top + r * 20, left + c * 15
                glyph[y:y + 12, x:x + int(rng.integers(6, 11))] = True
                n_glyphs += 1
    shapes = [[(0, 0)], [(0, 0), (0, 1)], [(0, 0), (1, 0), (1, 1)], [(0, 0), (0, 1), (1, 0), (1, 1)], [(0, 0), (0, 1), (0, 2), (0, 3)]]
    taken = ndimage.binary_dilation(glyph, np.ones((7, 7), bool))
    speck = np.zeros((H, W), bool)
    n_specks = 0
    for _ in range(400):
        shape = shapes[int(rng.integers(0, len(shapes)))]
        y, x = int(rng.integers(4, H - 8)), int(rng.integers(4, W - 8))
        if any(taken[y + dy, x + dx] for dy, dx in shape):
            continue
        one = np.zeros((H, W), bool)
        for dy, dx in shape:
            one[y + dy, x + dx] = True
        speck |= one
        taken |= ndimage.binary_dilation(one, np.ones((7, 7), bool))
        n_specks += 1
    ink = (glyph | speck).astype(np.uint8)
    return np.where(ink != 0, 20, 230).astype(np.uint8), ink, n_glyphs, n_specks, int(speck.sum())


def test_planted_specks_are_what_is_erased(gpu):
    from pseg_amd import engine as E
    scan, ink, n_glyphs, n_specks, speck_px = speck_page()
    assert n_specks > 60 and n_glyphs == 136
    d = gpu.Despeckle(4, 8)
    # the page is what it claims to be, on the CPU: no speck touches a glyph
    for conn in (4, 8):
        want, wc = C.restated(ink, 4, conn)
        assert list(wc) == [n_specks, speck_px, n_glyphs]
        (host,), hc = gpu.despeckle_maps([ink], gpu.Despeckle(4, conn), host=True, counts=True)
        assert np.array_equal(host, want) and list(hc[0]) == list(wc)
    (clean,), cnt = gpu.despeckle_maps([ink], d, counts=True)
    assert list(cnt[0]) == [n_specks, speck_px, n_glyphs] and np.array_equal(clean, C.restated(ink, 4, 8)[0])
    # through the front end at scale 1: without the despeckling every speck is an ink component of the map the vote works on
    plain = E.prepare_scans([scan], [1.0])[0]
    cleaned = E.prepare_scans([scan], [1.0], despeckle=d)[0]
    assert np.array_equal(plain[1], ink) and np.array_equal(cleaned[1], clean) and np.array_equal(cleaned[2], clean)
    zero = np.zeros(ink.shape, np.uint8)
    comps = gpu.eval_pages([zero, zero], [zero, zero], binaries=[plain[1], cleaned[1]], n_classes=3, connectivity=8)["components"]
    assert int(comps[0]) == n_glyphs + n_specks and int(comps[1]) == n_glyphs and int(comps[0] - comps[1]) == int(cnt[0][0])
