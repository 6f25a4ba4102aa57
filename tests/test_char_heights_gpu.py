"""pseg_char_heights / pseg_amd.char_heights / image_ops.compute_char_heights / Predictor.write_masks_scans(line_height_px=None):
the line heights of a list of scans in one device-resident call.

References: per scan the single-image entry (otsu_char_height, the parent's code path) and the NumPy oracle
(compute_char_height_from_gray, otsu_threshold); for the Predictor the same call with the heights filled in by compute_char_height.
Every comparison is for equality."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _text_scan(k, H, W, noise=0):
    """A synthetic text scan (ink dark); noise: a band of uniform gray noise so that the threshold is not trivial."""
    from pseg_amd import synth
    scan = (255 - synth.synth_page(k, H, W, 3)[0]).astype(np.uint8)
    if noise:
        rng = np.random.default_rng(900 + k)
        scan[-noise:, :] = rng.integers(0, 256, (noise, W), dtype=np.uint8)
    return scan


def _list_cases():
    rng = np.random.default_rng(17)
    noise = lambda H, W: rng.integers(0, 256, (H, W), dtype=np.uint8)
    boxed = noise(70, 50) // 4 + 180
    boxed[10:40, 12:32] = 20                                              # one glyph on noisy paper
    return [
        ("one row", noise(1, 37)),
        ("one column", noise(33, 1)),
        ("a glyph on noise, one tile and a bit", boxed),
        ("text, odd shape, byte loads", _text_scan(5, 203, 311, noise=20)),
        ("text, rows dword-aligned", _text_scan(6, 260, 420, noise=30)),
        ("flat", np.full((40, 50), 180, np.uint8)),
        ("two values", np.where(rng.random((61, 70)) < 0.3, 30, 200).astype(np.uint8)),
        ("text, several tiles both ways", _text_scan(7, 130, 257)),
        ("noise alone: runs everywhere", noise(97, 131)),
    ]


def _oracle(oracle_mod, scan, inverse):
    return oracle_mod.compute_char_height_from_gray(scan, inverse=inverse), int(oracle_mod.otsu_threshold(scan))


@pytest.mark.parametrize("inverse", [False, True])
def test_list_equals_single_equals_oracle(gpu, oracle_mod, inverse):
    cases = _list_cases()
    scans = [c[1] for c in cases]
    for run in range(2):                                                  # twice: no state survives a call
        heights, thresholds = gpu.char_heights(scans, inverse=inverse)
        assert len(heights) == len(thresholds) == len(scans)
        for (name, scan), h, t in zip(cases, heights, thresholds):
            single, want = gpu.otsu_char_height(scan, inverse=inverse), _oracle(oracle_mod, scan, inverse)
            print(name, inverse, (h, t), single, want)
            assert (h, t) == single, (name, run)
            assert (h, t) == want, (name, run)
    if not inverse:
        assert sum(h is not None for h in heights) >= 4                   # the text scans and the boxed glyph do measure


def _draw(scan, y, x, h, w, hollow):
    scan[y:y + h, x:x + w] = 0
    if hollow and h > 2 and w > 2:
        scan[y + 1:y + h - 1, x + 1:x + w - 1] = 255


def _edge_scans(geom):
    """One 0/255 scan of 300x420 per (shape, position): the shape under test and a ballast chosen so that the median says whether
    the shape was counted -- a shape lower than 30 rows beside glyphs of 30 and 45 rows (counted: 30, not counted: 45), a higher one
    beside one glyph of 30 rows (counted: its own height, not counted: 30)."""
    th, tw, above, below, left, right = geom
    shapes = [(h, w) for h in (10, 11, 59, 60) for w in (5, 6, 49, 50)] + [(20, 10), (20, 11), (20, 39), (20, 40), (12, 24), (24, 12)]
    out = []
    for k, (h, w) in enumerate(shapes):
        # first pixel and extents on every side of the tile and window borders: the shape starts on the last row / column of a tile, on
        # the first of the next, ends on a tile's last row / column, reaches the window's last row / column and one past it
        ys = [0, th - 1, th, 2 * th - h, th + th - 1 + below - (h - 1), th + th - 1 + below - (h - 1) + 1, 3 * th + 1]
        xs = [0, tw - 1, tw, 2 * tw - w, tw + tw - 1 + right - (w - 1), tw + tw - 1 + right - (w - 1) + 1, 2 * tw + 1]
        for j, (y, x) in enumerate(zip(ys, xs[k % 7:] + xs[:k % 7])):
            y, x = max(0, y), max(0, x)
            assert y + h <= 180 and x + w <= 260, (h, w, y, x)
            scan = np.full((300, 420), 255, np.uint8)
            _draw(scan, y, x, h, w, hollow=(j + k) % 2 == 1)
            _draw(scan, 200, 270, 30, 30, hollow=False)
            if h < 30:
                _draw(scan, 200, 320, 45, 30, hollow=True)
            out.append(((h, w, y, x), scan))
    return out


def test_filter_edges(gpu, oracle_mod):
    from pseg_amd import engine as E
    cases = _edge_scans(E.char_height_window())
    heights, thresholds = gpu.char_heights([c[1] for c in cases])
    seen = set()
    for (at, scan), h, t in zip(cases, heights, thresholds):
        want = _oracle(oracle_mod, scan, False)
        assert (h, t) == want, (at, (h, t), want)
        counted = (h == 30) if at[0] < 30 else (h == at[0])
        assert counted == (10 < at[0] < 60 and 5 < at[1] < 50 and 0.5 < at[1] / at[0] < 2), at     # the median does tell
        seen.add((at[:2], counted))
    assert len(seen) == 22 and sorted(k for k, c in seen if c) == [(11, 6), (20, 11), (20, 39), (59, 49)]
    assert ((12, 24), False) in seen and ((24, 12), False) in seen        # w / h = 2 and 0.5 exactly: out


def _spiral(h, w):
    """A one-pixel line that winds inwards with one-pixel gaps: a single component whose runs join only through many rows."""
    a = np.zeros((h, w), bool)
    y0, y1, x0, x1 = 0, h - 1, 0, w - 1
    first = True
    while y1 - y0 >= 2 and x1 - x0 >= 2:
        a[y0, (x0 if first else x0 - 1):x1 + 1] = True
        a[y0:y1 + 1, x1] = True
        a[y1, x0:x1 + 1] = True
        a[y0 + 2:y1 + 1, x0] = True
        first = False
        y0, y1, x0, x1 = y0 + 2, y1 - 2, x0 + 2, x1 - 2
        if y1 - y0 >= 2 and x1 - x0 >= 2:
            a[y0, x0 - 1] = True
    return a


def _fragment_scans():
    H, W = 300, 420
    blank = lambda: np.full((H, W), 255, np.uint8)
    out = []
    # a U whose arms look like glyphs to a window and join 200 rows lower; a rule across the page; a spiral; one plain glyph
    a = blank()
    a[20:240, 70:80] = 0
    a[20:240, 95:105] = 0
    a[230:240, 70:105] = 0
    a[270, :] = 0
    sp = _spiral(40, 30)
    from scipy import ndimage
    assert ndimage.label(sp)[1] == 1 and sp[0].all() and sp[:, -1].all()
    a[30:70, 200:230][sp] = 0
    _draw(a, 100, 300, 25, 20, hollow=False)
    out.append(("U, rule, spiral", a, 40))                                # heights [25, 40] -> 40: the spiral counts, the U does not
    # a frame around the page (touches every scan edge) with glyphs inside
    b = blank()
    b[0, :] = b[-1, :] = 0
    b[:, 0] = b[:, -1] = 0
    _draw(b, 2, 2, 20, 15, hollow=True)
    _draw(b, 150, 200, 31, 21, hollow=False)
    out.append(("page frame", b, 31))
    # a cross that touches every scan edge, glyphs in its quadrants
    c = blank()
    c[150, :] = 0
    c[:, 210] = 0
    _draw(c, 10, 10, 12, 12, hollow=False)
    _draw(c, 152, 212, 14, 14, hollow=False)
    _draw(c, 250, 30, 16, 16, hollow=True)
    out.append(("cross", c, 14))
    # glyphs flush against the four scan edges and in the corners: the scan edge is not a window side, they count
    d = blank()
    for y, x, h, w in ((0, 100, 21, 15), (H - 23, 200, 23, 15), (100, 0, 25, 15), (150, W - 15, 27, 15),
                       (0, 0, 29, 20), (H - 31, W - 20, 31, 20), (0, W - 20, 33, 20)):
        _draw(d, y, x, h, w, hollow=(h % 4 == 1))
    out.append(("flush glyphs", d, 27))                                   # [21 23 25 27 29 31 33] -> 27
    return out


def test_fragments_that_must_not_count(gpu, oracle_mod):
    cases = _fragment_scans()
    heights, thresholds = gpu.char_heights([c[1] for c in cases])
    for (name, scan, expect), h, t in zip(cases, heights, thresholds):
        want = _oracle(oracle_mod, scan, False)
        assert want[0] == expect, (name, want)                            # the scans are what their comments say
        assert (h, t) == want, (name, (h, t), want)


def _group_scans():
    rng = np.random.default_rng(23)
    out = []
    for k in range(70):                                                   # more than the 64 scans one group holds
        H, W = int(rng.integers(30, 80)), int(rng.integers(30, 100))
        scan = rng.integers(150, 256, (H, W), dtype=np.uint8)
        if k % 5 == 0:                                                    # every fifth has no glyph: two values, specks of ink
            scan = np.where(rng.random((H, W)) < 0.02, 40, 220).astype(np.uint8)
        else:
            h = int(rng.integers(11, min(H, 60) - 1))
            w = int(rng.integers(h // 2 + 1, min(2 * h, W - 1, 50)))
            scan[1:1 + h, 1:1 + w] = rng.integers(0, 60, (h, w), dtype=np.uint8)
        out.append(scan)
    return out


def test_groups(gpu, oracle_mod):
    scans = _group_scans()
    want = [_oracle(oracle_mod, s, False) for s in scans]
    assert len({w[0] for w in want}) > 10 and any(w[0] is None for w in want)
    heights, thresholds = gpu.char_heights(scans)
    assert list(zip(heights, thresholds)) == want
    perm = np.random.default_rng(3).permutation(len(scans))
    heights, thresholds = gpu.char_heights([scans[k] for k in perm])
    assert list(zip(heights, thresholds)) == [want[k] for k in perm]      # neither order nor grouping plays a part
    for k in (0, 5, 69):
        assert gpu.char_heights([scans[k]]) == ([want[k][0]], [want[k][1]])
    assert gpu.char_heights([]) == ([], [])
    assert gpu.char_heights(scans[:3], inverse=True)[1] == [w[1] for w in want[:3]]
    L = gpu.lib()
    assert L.pseg_release_workspace(0) == 0                               # the workspace goes and comes back
    assert gpu.char_heights(scans[60:]) == ([w[0] for w in want[60:]], [w[1] for w in want[60:]])


def test_refusals_name_the_scan(gpu):
    L = gpu.lib()
    scans = [np.full((20, 30), 200, np.uint8) for _ in range(4)]
    n = len(scans)

    def call(ptrs, Hs, Ws, heights):
        return L.pseg_char_heights(0, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*Hs), (ctypes.c_int * n)(*Ws), 0, heights, None)

    ptrs, Hs, Ws = [s.ctypes.data for s in scans], [20] * n, [30] * n
    heights = (ctypes.c_int * n)(*([-77] * n))
    assert call(ptrs[:2] + [None] + ptrs[3:], Hs, Ws, heights) == -1 and b"scan 2" in L.pseg_last_error()
    assert call(ptrs, Hs[:3] + [0], Ws, heights) == -1 and b"scan 3" in L.pseg_last_error() and b"empty" in L.pseg_last_error()
    assert call(ptrs, Hs, [-1] + Ws[1:], heights) == -1 and b"scan 0" in L.pseg_last_error()
    assert call(ptrs, Hs[:1] + [65536] + Hs[2:], Ws[:1] + [32768] + Ws[2:], heights) == -5 and b"scan 1" in L.pseg_last_error()
    assert L.pseg_char_heights(0, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*Hs), (ctypes.c_int * n)(*Ws), 0, None, None) == -1
    assert L.pseg_char_heights(0, -1, None, None, None, 0, heights, None) == -1
    assert L.pseg_char_heights(99, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*Hs), (ctypes.c_int * n)(*Ws), 0, heights, None) == -1
    assert list(heights) == [-77] * n                                     # nothing was written
    assert call(ptrs, Hs, Ws, heights) == 0 and list(heights) == [-1] * n   # otsu may be NULL; the library works on


def test_compute_char_heights_over_files(gpu, tmp_path):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height, compute_char_heights
    files = []
    for k, (name, scan) in enumerate(_list_cases()):
        files.append(str(tmp_path / ("scan%d.png" % k)))
        Image.fromarray(scan).save(files[-1])
    for inverse in (False, True):
        want = [compute_char_height(f, inverse) for f in files]
        assert compute_char_heights(files, inverse) == want
        assert compute_char_heights(files, inverse, decode_threads=1, chunk_files=4) == want
        assert compute_char_heights(iter(files[:1]), inverse) == want[:1]
    assert any(h is None for h in want) and any(h is not None for h in want)
    assert compute_char_heights([], False) == []
    with pytest.raises(Exception, match="File does not exist at"):
        compute_char_heights(files[:2] + [str(tmp_path / "missing.png")], False)


# ---- the Predictor ---------------------------------------------------------------------------------------------------------------
TARGET_LINE_HEIGHT = 6
SCAN_SHAPES = [(260, 200), (240, 230), (300, 260), (280, 210), (250, 250)]


def _predictor(gpu, high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)                    # a bf16 engine
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=high_res)
    return Predictor(settings, net), cm


@pytest.fixture(scope="module")
def scan_files(gpu, tmp_path_factory):
    """The scan files and, measured once, compute_char_height of each."""
    from PIL import Image
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    root = tmp_path_factory.mktemp("line_height_scans")
    files = []
    for k, s in enumerate(SCAN_SHAPES):
        files.append(str(root / ("scan%d.png" % k)))
        Image.fromarray(_text_scan(60 + k, s[0], s[1])).save(files[-1])
    blank = str(root / "blank.png")
    Image.fromarray(np.full((120, 90), 230, np.uint8)).save(blank)
    heights = [compute_char_height(f, False) for f in files]
    assert all(isinstance(h, int) for h in heights) and compute_char_height(blank, False) is None
    return files, heights, blank


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


def _rel(paths_per_page, root):
    return [[os.path.relpath(p, str(root)) for p in paths] for paths in paths_per_page]


@pytest.mark.parametrize("high_res", [False, True])
def test_write_masks_scans_measures_missing_line_heights(gpu, tmp_path, scan_files, high_res):
    from ocr4all_pixel_classifier.lib.dataset import Dataset, DatasetLoader, SingleData
    files, heights, blank = scan_files
    pred, cm = _predictor(gpu, high_res)
    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)
    filled = [SingleData(image_path=f, line_height_px=h) for f, h in zip(files, heights)]
    # entries that carry a line height: what the parent's pair of calls produces
    ds = Dataset([loader.load_images(dataclasses.replace(e)) for e in filled], loader.color_map)
    parent_paths = list(pred.write_masks_dataset(ds, str(tmp_path / "parent"), level=0))
    want_paths = list(pred.write_masks_scans([dataclasses.replace(e) for e in filled], loader, str(tmp_path / "filled"), level=0))
    want = _files(want_paths)
    assert want == _files(parent_paths) and _rel(want_paths, tmp_path / "filled") == _rel(parent_paths, tmp_path / "parent")
    # none given; a chunk that mixes given and missing ones; chunks smaller than the list
    for name, given, kw in (("none", (), {}), ("mixed", (1, 3), {}), ("chunks", (2,), {"chunk_pages": 2, "decode_threads": 1})):
        entries = [SingleData(image_path=f, line_height_px=(h if k in given else None)) for k, (f, h) in enumerate(zip(files, heights))]
        got_paths = list(pred.write_masks_scans(entries, loader, str(tmp_path / name), level=0, **kw))
        assert _rel(got_paths, tmp_path / name) == _rel(want_paths, tmp_path / "filled"), name
        assert _files(got_paths) == want, name
        assert [e.line_height_px for e in entries] == heights, name      # stored into the entries
        assert all(e.image is None and e.binary is None for e in entries), name     # otherwise untouched: the scan chain took them
    # the fallback route (not a PNG target) takes the measured height too
    entries = [SingleData(image_path=files[0], line_height_px=None, output_path="first.jpg"), SingleData(image_path=files[1], line_height_px=None)]
    ref = [SingleData(image_path=files[0], line_height_px=heights[0], output_path="first.jpg"), SingleData(image_path=files[1], line_height_px=heights[1])]
    got_paths = list(pred.write_masks_scans(entries, loader, str(tmp_path / "fallback"), level=0))
    ref_paths = list(pred.write_masks_scans(ref, loader, str(tmp_path / "fallback_ref"), level=0))
    assert got_paths[0][0].endswith("first.jpg") and _files(got_paths) == _files(ref_paths)
    assert [e.line_height_px for e in entries] == heights[:2] and entries[0].binary is not None
    # a scan without a measurable height raises at its entry, after the paths in front of it
    entries = [SingleData(image_path=files[0], line_height_px=None), SingleData(image_path=files[1], line_height_px=heights[1]),
               SingleData(image_path=blank, line_height_px=None), SingleData(image_path=files[2], line_height_px=None)]
    it = pred.write_masks_scans(entries, loader, str(tmp_path / "blank"), level=0)
    seen = []
    with pytest.raises(Exception, match="blank.png"):
        for paths in it:
            seen.append(paths)
    assert len(seen) == 2 and _files(seen) == want[:2]
    pred.network.model.close()
