"""pseg_predict_chain_pages_mixed_png / Engine.predict_chain_pages(mixed=True) / Predictor.write_masks_dataset(mixed=): a list of
pages of DIFFERENT shapes through the device chain, units formed by canvas.  The reference for every byte is the page-by-page chain
(Engine.predict_chain with masks="png", Predictor.write_masks) on the same engine.

The list has four canvases, interleaved: 96x64 (pages 0 2 4 6: 2, 1, 1, 1 bands at level 0), 160x224 (pages 1 5 7: 7, 5, 6 bands),
64x32 (page 3) and 32x64 (page 8); odd widths and a width of 1 meet the edges of the pad and crop kernels.  The planner keeps
pseg_chain_units' ramps, so the first page of the list travels alone and, without out-shapes, the 96x64 unit of two pages holds one
band per page: there the 160x224 unit alone mixes band counts.  The per-page out-shapes give both units pages of different band
counts (3 and 1; 12, 1 and 2), one of them a page that is not resized among pages that are."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(96, 64), (160, 224), (70, 50), (33, 1), (65, 47), (129, 193), (90, 33), (150, 200), (1, 37)]
OUT = [(167, 105), (231, 265), (141, 91), (40, 3), None, (40, 60), None, (100, 100), (3, 50)]
NAMES = ("color", "overlay", "inverted", "fg_color")
LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)


def _canvas(s):
    return (-(-s[0] // 32) * 32, -(-s[1] // 32) * 32)


def _bands(shape, level):
    """png_rows restated: rows per band from the filtered row's bytes, then the band count."""
    H, W = shape
    L = 3 * W + 1
    R = min(H, max(1, (65536 if level else 16384) // L))
    return -(-H // R)


def _pages(shapes=SHAPES, out=OUT, channels=1):
    """Per page: image, binarisation at the page's shape, out-shape or None, binarisation at the final shape."""
    from pseg_amd import synth
    pages = []
    for k, s in enumerate(shapes):
        rng = np.random.default_rng(100 + k)
        if min(s) >= 48 and channels == 1:
            img, binary, _ = synth.synth_page(4 + k, s[0], s[1], 3)
        else:                                   # (synth_page draws text lines: not on a page of one row or one column)
            img = rng.integers(0, 256, s if channels == 1 else s + (channels,), dtype=np.uint8)
            binary = (rng.random(s) < 0.3).astype(np.uint8)
        fs = out[k] if out[k] is not None else s
        pages.append((img, binary, out[k], (rng.random(fs) < 0.2).astype(np.uint8) if out[k] is not None else binary))
    return pages


def _engine(gpu, arch, mode, **kw):
    from pseg_amd import synth
    eng = gpu.Engine(arch, 3, mode=mode, **kw)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return eng


@pytest.fixture(scope="module")
def engines(gpu):
    engs = {"f32": _engine(gpu, "fcn_skip", gpu.MODE_F32_EXACT), "bf16": _engine(gpu, "fcn_skip", gpu.MODE_BF16)}
    yield engs
    for e in engs.values():
        e.close()


def _single(eng, page, posts, resized, level):
    img, binary, osh, big = page
    r = eng.predict_chain(img, binary=big if resized else binary, out_shape=osh if resized else None, post_ops=posts, labels="u8", lut=LUT,
                          masks="png", png_level=level)
    return np.array(r["labels"]), dict(zip(NAMES, r["masks"]))


def _mixing_units(cap, resized, level):
    """The planner's units that hold two or more pages with different (H, W) and different band counts of their final maps."""
    from pseg_amd import engine as E
    order, units = E.chain_units_mixed(SHAPES, cap=cap)
    final = [OUT[k] if resized and OUT[k] is not None else SHAPES[k] for k in range(len(SHAPES))]
    hit = []
    for first, count in units:
        pages = [order[first + k] for k in range(count)]
        assert len({_canvas(SHAPES[p]) for p in pages}) == 1
        if count >= 2 and len({SHAPES[p] for p in pages}) >= 2 and len({_bands(final[p], level) for p in pages}) >= 2:
            hit.append(pages)
    return hit


def test_the_list_forms_units_that_mix_shapes_and_band_counts(gpu):
    assert len({_canvas(s) for s in SHAPES}) == 4
    assert [_bands(SHAPES[p], 0) for p in (1, 5, 7)] == [7, 5, 6] and [_bands(SHAPES[p], 0) for p in (0, 2, 4, 6)] == [2, 1, 1, 1]
    # this is what keeps the byte comparisons below from passing on single-page units
    for cap in (2, 4):                          # (unit_cap 0 is 2 for a list of nine pages)
        assert len(_mixing_units(cap, True, 0)) >= 2, cap
        assert len(_mixing_units(cap, False, 0)) >= 1, cap
    assert sorted(_bands(OUT[p], 0) for p in (1, 5, 7)) == [1, 2, 12] and [1, 5, 7] in _mixing_units(4, True, 0)


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_bytes_equal_the_page_by_page_chain(gpu, engines, mode_name, level):
    eng = engines[mode_name]
    pages = _pages()
    imgs = [p[0] for p in pages]
    for posts in ([], ["cc_vote"], ["cc_vote", "bbox"]):
        for resized in (False, True):
            want = [_single(eng, p, posts, resized and p[2] is not None, level) for p in pages]
            for cap in (0, 2, 4):
                got = eng.predict_chain_pages(imgs, binaries=[p[3] if resized else p[1] for p in pages],
                                              out_shapes=[p[2] for p in pages] if resized else None, post_ops=posts, lut=LUT,
                                              labels=True, png_level=level, unit_cap=cap, mixed=True)
                assert len(got) == len(pages)
                for k, (g, (lab, masks)) in enumerate(zip(got, want)):
                    at = (k, posts, resized, cap)
                    assert g["labels"].dtype == np.uint8 and g["labels"].shape == lab.shape, at
                    assert g["labels"].tobytes() == lab.tobytes(), at
                    assert sorted(g["masks"]) == ["color", "inverted", "overlay"], at
                    for name in g["masks"]:
                        assert g["masks"][name] == masks[name], at + (name,)
    # mask subsets (the k-th requested mask is not mask k), and labels alone: neither table nor binarisation
    want = [_single(eng, p, ["cc_vote"], False, level) for p in pages]
    for which in (("overlay",), NAMES, ("fg_color", "color")):
        got = eng.predict_chain_pages(imgs, binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=LUT, which=which, png_level=level,
                                      unit_cap=4, mixed=True)
        for g, (_, masks) in zip(got, want):
            assert g["labels"] is None and g["masks"] == {n: masks[n] for n in which}, which
    got = eng.predict_chain_pages(imgs, which=(), labels=True, unit_cap=4, mixed=True)
    bare = [np.array(eng.predict_chain(p[0], labels="u8")["labels"]) for p in pages]
    assert all(g["masks"] == {} and np.array_equal(g["labels"], b) for g, b in zip(got, bare))


@pytest.mark.parametrize("arch", ["unet", "res_unet"])
def test_other_graphs_on_one_canvas(gpu, arch):
    from pseg_amd import engine as E
    eng = _engine(gpu, arch, gpu.MODE_BF16)
    # three pages of one canvas; a page of another canvas on either side keeps the list's ramps (1, 2, ...) off them: one unit of three
    shapes = [(33, 40), (70, 50), (96, 64), (65, 47), (40, 100)]
    assert E.chain_units_mixed(shapes, cap=4) == ([0, 1, 2, 3, 4], [(0, 1), (1, 3), (4, 1)])
    pages = _pages(shapes, [None] * 5)
    want = [_single(eng, p, ["cc_vote"], False, 0) for p in pages]
    got = eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=LUT, labels=True,
                                  unit_cap=4, mixed=True)
    for g, (lab, masks) in zip(got, want):
        assert np.array_equal(g["labels"], lab) and g["masks"] == {n: masks[n] for n in NAMES[:3]}
    eng.close()


def test_three_channel_pages(gpu):
    eng = _engine(gpu, "fcn_skip", gpu.MODE_BF16, in_channels=3)
    from pseg_amd import engine as E
    shapes = [(70, 50), (129, 193), (160, 224), (65, 47), (150, 200), (33, 40)]
    assert E.chain_units_mixed(shapes, cap=4) == ([0, 3, 1, 2, 4, 5], [(0, 1), (1, 1), (2, 3), (5, 1)])
    pages = _pages(shapes, [None] * 6, channels=3)
    want = [_single(eng, p, ["cc_vote"], False, 1) for p in pages]
    got = eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=LUT, labels=True,
                                  png_level=1, unit_cap=4, mixed=True)
    for g, (lab, masks) in zip(got, want):
        assert np.array_equal(g["labels"], lab) and g["masks"] == {n: masks[n] for n in NAMES[:3]}
    eng.close()


def test_sink_contract(gpu, engines):
    from pseg_amd import engine as E
    eng = engines["bf16"]
    pages = _pages()
    imgs, bins = [p[0] for p in pages], [p[1] for p in pages]
    n = len(pages)
    full = eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=4, mixed=True)
    calls = []
    assert eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=4, mixed=True,
                                   sink=lambda page, name, data: calls.append((page, name, data))) is None
    order, _ = E.chain_units_mixed(SHAPES, cap=4)
    names = ["color", "overlay", "inverted", "labels"]
    assert order != list(range(n))
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
            raise Stop("fourth page")

    with pytest.raises(Stop, match="fourth page"):
        eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, unit_cap=4, mixed=True, sink=raising)
    assert seen == [(p, nm) for p in order[:3] for nm in names[:3]] + [(order[3], "color")]    # nothing behind the call that raised
    # the raw return code of a sink that says stop, then the engine again: the full, correct result
    L = gpu.lib()
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    stop = E.CHAIN_SINK(lambda user, page, which, data, nb: 1 if page == order[1] else 0)
    rc = L.pseg_predict_chain_pages_mixed_png(eng._h, n, P(*[a.ctypes.data for a in imgs]), I(*[s[0] for s in SHAPES]), I(*[s[1] for s in SHAPES]),
                                              None, None, P(*[b.ctypes.data for b in bins]), (ctypes.c_int * 1)(1), 1, 0, LUT.ctypes.data, 3, 0, 7, 4,
                                              stop, None)
    assert rc == -6 and b"sink" in L.pseg_last_error()
    again = eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=4, mixed=True)
    assert all(a["masks"] == f["masks"] and np.array_equal(a["labels"], f["labels"]) for a, f in zip(again, full))
    assert eng.predict_chain_pages([], lut=LUT, mixed=True) == []
    # the same-shape entry still sees the list in page order
    plain = []
    eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, unit_cap=4, sink=lambda page, name, data: plain.append(page))
    assert plain == [p for p in range(n) for _ in range(3)]


def _predictor_and_dataset(gpu, posts, high_res):
    import dataclasses
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    data = []
    for k, s in enumerate([(96, 64), (160, 224), (70, 50), (65, 47), (129, 193), (90, 33), (150, 200)]):
        img, binary, _ = synth.synth_page(20 + k, s[0], s[1], 3)
        d = SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page%d.png" % k)
        if high_res:
            orig = (s[0] + 71 - 9 * k, s[1] + 41 + 5 * k)
            d = dataclasses.replace(d, original_shape=orig, orig_binary=(np.random.default_rng(k).random(orig) < 0.2).astype(np.uint8))
        data.append(d)
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor(p) for p in posts], high_res_output=high_res)
    return Predictor(settings, net), Dataset(data, cm)


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


@pytest.mark.parametrize("posts,high_res,level", [(["cc_majority"], False, 0), (["cc_majority", "bounding_boxes"], True, 1)])
def test_write_masks_dataset(gpu, tmp_path, posts, high_res, level):
    pred, ds = _predictor_and_dataset(gpu, posts, high_res)
    want_paths = [pred.write_masks(d, str(tmp_path / "single"), level=level) for d in ds.data]
    want = _files(want_paths)
    for name, kw in (("mixed", {"mixed": True}), ("default", {}), ("plain", {"mixed": False}), ("chunks", {"mixed": True, "chunk_pages": 4})):
        got_paths = list(pred.write_masks_dataset(ds, str(tmp_path / name), level=level, **kw))
        assert [[os.path.relpath(p, str(tmp_path / name)) for p in paths] for paths in got_paths] == \
               [[os.path.relpath(p, str(tmp_path / "single")) for p in paths] for paths in want_paths], name
        assert _files(got_paths) == want, name
