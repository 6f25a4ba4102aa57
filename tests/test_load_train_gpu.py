"""DatasetLoader.load_data_list against DatasetLoader.load_data -- the parent's code, unchanged -- on PNG files: every field and dtype
of every record, under both binarisations, for prediction, for several chunk sizes and pool sizes, through load_data_from_json; the
report and the warning about unknown colours; an undecodable file in the middle; one training epoch over both datasets."""
import copy
import json
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGET_LINE_HEIGHT = 6
MAX_WIDTH = 210
LUT = np.array([(255, 255, 255), (255, 0, 0), (0, 255, 0)], np.uint8)
FIELDS = ("image", "binary", "orig_binary", "mask")


def _color_map():
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    return ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})


def _page(seed, shape):
    """-> (scan uint8, ink dark; label ids uint8) of a synthetic page."""
    from pseg_amd import synth
    img, _, ids = synth.synth_page(seed, shape[0], shape[1], 3)
    return (255 - img).astype(np.uint8), ids.astype(np.uint8)


def _soft_edges(rgb, ids):
    """Anti-aliased region edges, as hand-made ground truth has them: colours the map does not know."""
    edge = np.zeros(ids.shape, bool)
    edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    rgb = rgb.copy()
    rgb[edge] = (rgb[edge].astype(np.int32) + 255) // 2                 # (white stays white)
    return rgb, int((edge & (ids != 0)).sum())


@pytest.fixture(scope="module")
def corpus(gpu, tmp_path_factory):
    """Nine entries of distinct shapes and line heights as PNG files: masks saved as RGB, palette and RGBA files; a mask of another
    shape than its scan; a pre-loaded image and mask; a pre-loaded mask only; a scan so wide that max_width brings the second stage;
    an entry without a line height; a mask with soft edges.  -> make(): fresh entries, and what the test knows about them."""
    from PIL import Image
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    root = tmp_path_factory.mktemp("train_files")
    spec = [((60, 45), 8, "RGB"), ((97, 131), 11, "P"), ((150, 101), 9, "RGBA"), ((300, 220), 12, "other shape"), ((120, 90), 10, "preloaded both"),
            ((133, 77), 7, "preloaded mask"), ((80, 219), 3, "max_width"), ((260, 200), None, "unmeasured"), ((201, 160), 13, "soft edges")]
    made, soft = [], 0
    for k, (shape, lh, kind) in enumerate(spec):
        scan, ids = _page(60 if kind == "unmeasured" else 20 + k, shape)
        scan_path, mask_path = str(root / ("scan%d.png" % k)), str(root / ("mask%d.png" % k))
        Image.fromarray(scan).save(scan_path)
        if kind == "other shape":
            ids = _page(40, (150, 110))[1]
        rgb = LUT[ids]
        if kind == "soft edges":
            rgb, soft = _soft_edges(rgb, ids)
        if kind == "P":
            im = Image.frombytes("P", (ids.shape[1], ids.shape[0]), ids.tobytes())
            im.putpalette([int(v) for v in LUT.reshape(-1)])
            im.save(mask_path)
        elif kind == "RGBA":
            Image.fromarray(np.dstack([rgb, np.full(ids.shape, 255, np.uint8)])).save(mask_path)
        else:
            Image.fromarray(rgb).save(mask_path)
        made.append((kind, scan_path, mask_path, lh, scan, ids))
    assert soft > 0
    assert [Image.open(m[2]).mode for m in made[:3]] == ["RGB", "P", "RGBA"]
    measured = compute_char_height(made[7][1], False)
    assert isinstance(measured, int)

    def make(measure=False):
        out = []
        for kind, scan_path, mask_path, lh, scan, ids in made:
            e = SingleData(image_path=scan_path, mask_path=mask_path, line_height_px=lh if lh is not None or not measure else measured)
            if kind == "preloaded both":
                e.image, e.mask = scan.copy(), ids.copy()
            elif kind == "preloaded mask":
                e.mask, e.mask_path = ids.copy(), None
            out.append(e)
        return out
    return make, made, measured, soft


def _loader(binarize=None, prediction=False):
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader
    return DatasetLoader(TARGET_LINE_HEIGHT, _color_map(), prediction=prediction, max_width=MAX_WIDTH, binarize=binarize)


@pytest.fixture(scope="module")
def reference(gpu, corpus):
    """load_data per loader configuration, once: compute_char_height fills the missing line height first."""
    make = corpus[0]
    memo = {}

    def get(name):
        if name not in memo:
            loader = _loader(gpu.Sauvola() if name == "sauvola" else None, name == "prediction")
            memo[name] = loader.load_data(make(measure=True))
        return memo[name]
    return get


def _same_records(got, want):
    assert len(got) == len(want) == 9
    for k, (g, w) in enumerate(zip(got.data, want.data)):
        for f in FIELDS:
            a, b = getattr(g, f), getattr(w, f)
            if b is None:
                assert a is None, (k, f)
                continue
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (k, f, getattr(a, "dtype", None), b.dtype)
            assert np.array_equal(a, b), (k, f, int((a != b).sum()))
        assert tuple(g.original_shape) == tuple(w.original_shape) and g.line_height_px == w.line_height_px, k
        assert (g.image_path, g.mask_path, g.binary_path) == (w.image_path, w.mask_path, w.binary_path)
    assert got.color_map is not None


def _loader_of(gpu, name):
    return _loader(gpu.Sauvola() if name == "sauvola" else None, name == "prediction")


@pytest.mark.parametrize("name", ["plain", "sauvola", "prediction"])
def test_list_route_gives_the_records_of_load_data(gpu, corpus, reference, name):
    make, made, measured, _ = corpus
    want = reference(name)
    assert want.data[0].mask.dtype == np.uint8 if name != "prediction" else want.data[0].mask is None
    entries = make()
    report = []
    got = _loader_of(gpu, name).load_data_list(entries, report=report)
    assert got.data == entries and all(a is b for a, b in zip(got.data, entries))       # in place, in order
    _same_records(got, want)
    assert entries[7].line_height_px == measured
    # the two fallbacks took load_images' route (no report), the others the list's
    if name == "prediction":
        assert report == [None] * 9
    else:
        assert [r is None for r in report] == [k in (4, 6) for k in range(9)]
    if name == "sauvola":
        assert any(not np.array_equal(a.orig_binary, b.orig_binary) for a, b in zip(want.data, reference("plain").data))
    # the wide scan really brought the second stage
    assert want.data[6].image.shape[1] <= MAX_WIDTH < gpu.engine.rescale_shape(made[6][4].shape, TARGET_LINE_HEIGHT / 3)[1]
    assert want.data[3].mask.shape == want.data[3].image.shape if name != "prediction" else True


@pytest.mark.parametrize("chunk,threads", [(1, 1), (4, 3), (64, 1), (4, 2)])
def test_chunks_and_pool_sizes(gpu, corpus, reference, chunk, threads):
    got = _loader_of(gpu, "plain").load_data_list(corpus[0](), chunk=chunk, decode_threads=threads)
    _same_records(got, reference("plain"))


def test_report_and_warning(gpu, corpus, reference, caplog):
    make, made, _, soft = corpus
    report = []
    with caplog.at_level(logging.WARNING):
        got = _loader_of(gpu, "plain").load_data_list(make(), chunk=4, report=report)
    assert len(report) == 9
    for k, (r, d) in enumerate(zip(report, got.data)):
        if r is None:
            continue
        assert set(r) == {"label_counts", "unknown"} and r["label_counts"].dtype == np.int64 and r["label_counts"].shape == (256,)
        assert np.array_equal(r["label_counts"], np.bincount(d.mask.reshape(-1), minlength=256)), k
        assert isinstance(r["unknown"], int) and (r["unknown"] > 0) == (k == 8), k
    # the count is what the reference route lost silently: the page's pixels whose source colour the map does not hold
    from oracle import resize as oresize
    from PIL import Image
    rgb = np.asarray(Image.open(made[8][2]).convert("RGB"))
    known = np.zeros(rgb.shape[:2], bool)
    for c in LUT:
        known |= (rgb == c).all(-1)
    assert int((~known).sum()) == soft
    assert report[8]["unknown"] == int(oresize.resize_nearest((~known).astype(np.uint8), got.data[8].image.shape).sum())
    warned = [r for r in caplog.records if r.levelno == logging.WARNING and "colour map does not know" in r.getMessage()]
    assert len(warned) == 1 and made[8][2] in warned[0].getMessage() and str(report[8]["unknown"]) in warned[0].getMessage()


def test_load_data_from_json(gpu, corpus, tmp_path):
    make, made, measured, _ = corpus
    rows = [dict(image_path=m[1], mask_path=m[2], line_height_px=m[3] if m[3] is not None else measured) for m in made]
    path = str(tmp_path / "dataset.json")
    with open(path, "w") as f:
        json.dump({"train": rows[:5], "test": rows[5:7], "eval": rows[7:]}, f)
    loader = _loader_of(gpu, "plain")
    for kind in ("train", "all"):
        want = loader.load_data_from_json([path], kind)
        got = loader.load_data_from_json([path], kind, as_list=True)
        assert len(got) == len(want) == (5 if kind == "train" else 9)
        for g, w in zip(got.data, want.data):
            for f in FIELDS:
                a, b = getattr(g, f), getattr(w, f)
                assert a.dtype == b.dtype and np.array_equal(a, b)
            assert tuple(g.original_shape) == tuple(w.original_shape)


@pytest.mark.parametrize("what", ["scan", "mask"])
def test_an_undecodable_file_in_the_middle(gpu, corpus, reference, tmp_path, what):
    import PIL
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    made = corpus[1]
    broken = str(tmp_path / "broken.png")
    with open(broken, "wb") as f:
        f.write(b"this is no image")
    rows = [made[k] for k in (0, 1, 2, 3, 8, 0, 1)]
    for chunk in (3, 64):
        entries = [SingleData(image_path=m[1], mask_path=m[2], line_height_px=m[3]) for m in rows]
        if what == "scan":
            entries[4].image_path = broken
        else:
            entries[4].mask_path = broken
        with pytest.raises(PIL.UnidentifiedImageError):
            _loader_of(gpu, "plain").load_data_list(entries, chunk=chunk)
        want = reference("plain").data
        for e, k in zip(entries[:4], (0, 1, 2, 3)):                     # the entries in front of it are loaded
            assert all(np.array_equal(getattr(e, f), getattr(want[k], f)) for f in FIELDS)
        assert all(e.image is None and e.binary is None and e.mask is None and e.original_shape is None for e in entries[4:])
    # a scan without a measurable height raises naming the file
    from PIL import Image
    blank = str(tmp_path / "blank.png")
    Image.fromarray(np.full((120, 90), 230, np.uint8)).save(blank)
    entries = [SingleData(image_path=rows[0][1], mask_path=rows[0][2], line_height_px=8), SingleData(image_path=blank, mask_path=rows[0][2], line_height_px=None)]
    with pytest.raises(Exception, match="blank.png"):
        _loader_of(gpu, "plain").load_data_list(entries)
    assert entries[0].image is not None and entries[1].image is None


def test_one_training_epoch_over_both_datasets(gpu, corpus, reference, tmp_path):
    """Network.train_dataset on a tiny fcn_skip: the records are equal, so the histories are."""
    from ocr4all_pixel_classifier.lib.trainer import Trainer, TrainSettings
    from ocr4all_pixel_classifier.lib.dataset import Dataset
    from ocr4all_pixel_classifier.lib.metrics import Monitor
    listed = _loader_of(gpu, "plain").load_data_list(corpus[0]())
    hists = []
    for tag, ds in (("load_data", reference("plain")), ("load_data_list", listed)):
        data = copy.deepcopy(ds.data)
        np.random.seed(0)
        settings = TrainSettings(n_epoch=1, n_classes=3, l_rate=2e-3, train_data=Dataset(data[:6], ds.color_map), validation_data=Dataset(data[6:], ds.color_map),
                                 display=1, output_dir=str(tmp_path / tag), threads=1, monitor=Monitor.VAL_LOSS)
        t = Trainer(settings)
        hists.append(t.train())
        t.train_net.model.close()
    assert set(hists[0]) == set(hists[1]) and len(hists[0]["loss"]) == 1 and np.isfinite(hists[0]["loss"]).all()
    for k in hists[0]:
        assert hists[0][k] == hists[1][k], (k, hists[0][k], hists[1][k])
