"""DatasetLoader(deskew=...) and Predictor.write_masks_scans(deskew=...) on the device, on a small bf16 fcn_skip with PNG scans in a
tmp dir: the loader against a manual deskew_scans followed by today's loader on the pre-rotated arrays; load_data_list against
load_data; the Predictor's files against DatasetLoader(deskew=...) + load_images + write_masks_dataset, with an unmeasured entry, a
fallback entry and a planted 2 degree page among them; deskew=None against a call without the argument.  Every comparison is for
equal bytes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
TARGET_LINE_HEIGHT = 6
FIELDS = ("image", "binary", "orig_binary", "mask")
# (shape, planted index over 1024): 36 / 1024 is a slope of 2 degrees
PAGES = [((300, 250), -23), ((280, 300), 36), ((260, 420), 5), ((300, 200), 0)]


def _color_map():
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    return ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})


def _make_files(gpu, tmp_path):
    """[(scan file, mask file, scan, mask ids, planted index)]: synthetic pages, scan and mask skewed by the same planted index."""
    from PIL import Image
    from pseg_amd import synth
    made = []
    for k, (shape, a0) in enumerate(PAGES):
        img, _, ids = synth.synth_page(30 + k, shape[0], shape[1], 3)
        scan = gpu.rotate_maps([(255 - img).astype(np.uint8)], -a0, order=1, fill=255, host=True)[0]
        ids = gpu.rotate_maps([ids.astype(np.uint8)], -a0, order=0, fill=0, host=True)[0]
        scan_path, mask_path = str(tmp_path / ("scan%d.png" % k)), str(tmp_path / ("mask%d.png" % k))
        Image.fromarray(scan).save(scan_path)
        Image.fromarray(LUT[ids]).save(mask_path)
        made.append((scan_path, mask_path, scan, ids, a0))
    return made


def _same_records(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            a, b = getattr(g, f), getattr(w, f)
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, f)
        assert tuple(g.original_shape) == tuple(w.original_shape) and g.line_height_px == w.line_height_px, k


def test_loader_deskews_scan_and_mask(gpu, tmp_path):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    made = _make_files(gpu, tmp_path)
    how = gpu.Skew()
    heights = [9, 10, 8, 11]

    def entries():
        out = [SingleData(image_path=m[0], mask_path=m[1], line_height_px=h) for m, h in zip(made, heights)]
        out.append(SingleData(image=made[0][2].copy(), mask=made[0][3].copy(), line_height_px=9))     # pre-loaded: left as it is
        return out

    calls = []
    loader = DatasetLoader(TARGET_LINE_HEIGHT, _color_map(), deskew=how, on_skew=lambda e, i, d: calls.append((e.image_path, i, d)))
    got = loader.load_data(entries()).data
    # the estimate is skew_maps' on scan <= 127; the planted skews are found, to within the strip method's reach on these pages
    want_idx = gpu.skew_maps([m[2] <= 127 for m in made], how)
    assert calls == [(m[0], int(i), 1024) for m, i in zip(made, want_idx)]
    print("planted -> found:", [(m[4], int(i)) for m, i in zip(made, want_idx)])
    assert [int(np.sign(i)) for i in want_idx] == [int(np.sign(m[4])) for m in made]
    # by hand: deskew_scans, the mask rotated with the same index, then today's loader on the pre-rotated arrays
    turned, idx = gpu.deskew_scans([m[2] for m in made], how)
    assert np.array_equal(idx, want_idx)
    turned_files, turned_masks = [], []
    for k, (m, t, a) in enumerate(zip(made, turned, idx)):
        turned_files.append(str(tmp_path / ("turned%d.png" % k)))
        Image.fromarray(t).save(turned_files[-1])
        turned_masks.append(gpu.rotate_maps([m[3]], int(a), order=0, fill=0)[0])

    def by_hand():
        return [SingleData(image_path=p, mask=m.copy(), line_height_px=h) for p, m, h in zip(turned_files, turned_masks, heights)]

    plain = DatasetLoader(TARGET_LINE_HEIGHT, _color_map())
    want = plain.load_data(by_hand() + entries()[4:]).data
    _same_records(got, want)
    assert not np.array_equal(got[1].mask, plain.load_data(entries()[1:2]).data[0].mask)   # the mask did turn
    # load_data_list: every entry through load_images, in place and in order
    calls.clear()
    report = []
    listed = loader.load_data_list(entries(), chunk=2, report=report).data
    _same_records(listed, got)
    assert report == [None] * 5 and [c[1] for c in calls] == [int(i) for i in want_idx]
    # with a binarisation and a despeckling: derived from the deskewed scan
    both = DatasetLoader(TARGET_LINE_HEIGHT, _color_map(), binarize=gpu.Sauvola(), despeckle=gpu.Despeckle(), deskew=how)
    want2 = DatasetLoader(TARGET_LINE_HEIGHT, _color_map(), binarize=gpu.Sauvola(), despeckle=gpu.Despeckle()).load_data(
        by_hand()).data
    _same_records(both.load_data(entries()[:4]).data, want2)


def _predictor(gpu):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = _color_map()
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=False)
    return Predictor(settings, net), cm


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


def _rel(paths_per_page, root):
    return [[os.path.relpath(p, str(root)) for p in paths] for paths in paths_per_page]


def test_write_masks_scans_with_a_deskew(gpu, tmp_path):
    from ocr4all_pixel_classifier.lib.dataset import Dataset, DatasetLoader, SingleData
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    made = _make_files(gpu, tmp_path)
    files = [m[0] for m in made]
    heights = [compute_char_height(f, False) for f in files]
    assert all(isinstance(h, int) for h in heights)
    # a max_width between the widest page (entry 2: the fallback route) and the others
    widths = [gpu.engine.rescale_shape(m[2].shape, TARGET_LINE_HEIGHT / h)[1] for m, h in zip(made, heights)]
    assert widths[2] == max(widths) and sorted(widths)[-2] < widths[2] - 1
    max_width = (sorted(widths)[-2] + widths[2]) // 2
    pred, cm = _predictor(gpu)
    how = gpu.Skew()

    def entries(measured):
        # entry 1 (the 2 degree page) has no line height: measured in the call
        return [SingleData(image_path=f, line_height_px=(h if measured or k != 1 else None)) for k, (f, h) in enumerate(zip(files, heights))]

    loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, max_width=max_width, deskew=how)
    loaded = [loader.load_images(e) for e in entries(True)]
    want_paths = list(pred.write_masks_dataset(Dataset(loaded, cm), str(tmp_path / "parent"), level=0))
    want = _files(want_paths)
    want_idx = [int(i) for i in gpu.skew_maps([m[2] <= 127 for m in made], how)]
    plain = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True, max_width=max_width)      # the call's deskew, not the loader's, decides
    for name, kw in (("whole", {}), ("chunks", {"chunk_pages": 3, "decode_threads": 1})):
        mine, calls = entries(False), []
        got_paths = list(pred.write_masks_scans(mine, plain, str(tmp_path / name), level=0, deskew=how,
                                                on_skew=lambda k, i, d: calls.append((k, i, d)), **kw))
        assert _rel(got_paths, tmp_path / name) == _rel(want_paths, tmp_path / "parent"), name
        assert _files(got_paths) == want, name
        assert calls == [(k, i, 1024) for k, i in enumerate(want_idx)], name
        # the unmeasured entry was measured on the scan as decoded; only the fallback entry was loaded in place
        assert mine[1].line_height_px == heights[1] and mine[2].binary is not None and mine[0].binary is None, name
    # deskew=None is today's call, byte for byte, and the deskewed files are another result
    today = _files(list(pred.write_masks_scans(entries(True), plain, str(tmp_path / "today"), level=0)))
    assert _files(list(pred.write_masks_scans(entries(True), plain, str(tmp_path / "none"), level=0, deskew=None))) == today
    assert today != want
    for k, a in enumerate(want_idx):                                   # only a page that was turned changed
        assert (today[k] == want[k]) == (a == 0), k
