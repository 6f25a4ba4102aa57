"""pseg_predict_chain_pages_png / Engine.predict_chain_pages / Predictor.write_masks_dataset: a page list through the device chain
to PNG streams.  The reference for every byte is the page-by-page chain (Engine.predict_chain with masks="png", Predictor.write_masks)
on the same engine: the list entry pipelines and batches, it must not change a single byte.  Tiny pages: 96x64 (A), 70x50 (B: no
multiple of 32, H*W no multiple of 256) and 160x224 (C: 7 bands at level 0, 2 at level 1)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, B, C = (96, 64), (70, 50), (160, 224)
SHAPES = [A, A, A, B, A, A, C]
NAMES = ("color", "overlay", "inverted", "fg_color")
LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)


def _pages(shapes=SHAPES):
    """Per page: image, binarisation at the page's shape, out-shape (+71, +41), binarisation at the out-shape."""
    from pseg_amd import synth
    out = []
    for k, s in enumerate(shapes):
        img, binary, _ = synth.synth_page(4 + k, s[0], s[1], 3)
        osh = (s[0] + 71, s[1] + 41)
        out.append((img, binary, osh, (np.random.default_rng(k).random(osh) < 0.2).astype(np.uint8)))
    return out


@pytest.fixture(scope="module")
def engines(gpu, oracle_mod):
    Wt = oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05)
    engs = {}
    for mode in (gpu.MODE_F32_EXACT, gpu.MODE_BF16):
        engs[mode] = gpu.Engine("fcn_skip", 3, mode=mode)
        engs[mode].set_weights(Wt)
    yield engs
    for e in engs.values():
        e.close()


def _single(eng, page, posts, resized, level):
    img, binary, osh, big = page
    r = eng.predict_chain(img, binary=big if resized else binary, out_shape=osh if resized else None, post_ops=posts, labels="u8", lut=LUT,
                          masks="png", png_level=level)
    return np.array(r["labels"]), dict(zip(NAMES, r["masks"]))


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_bytes_equal_the_page_by_page_chain(gpu, engines, mode_name, level):
    eng = engines[gpu.MODE_F32_EXACT if mode_name == "f32" else gpu.MODE_BF16]
    pages = _pages()
    from pseg_amd import engine as E
    units = E.chain_units(SHAPES, cap=2)
    assert len(units) >= 4 and max(c for _, c in units) == 2        # both staging sets are used again; units of A hold two pages
    for posts in ([], ["cc_vote"], ["cc_vote", "bbox"]):
        for resized in (False, True):
            want = [_single(eng, p, posts, resized, level) for p in pages]
            got = eng.predict_chain_pages([p[0] for p in pages], binaries=[p[3] if resized else p[1] for p in pages],
                                          out_shapes=[p[2] for p in pages] if resized else None, post_ops=posts, lut=LUT,
                                          labels=True, png_level=level, unit_cap=2)
            assert len(got) == len(pages)
            for k, (g, (lab, masks)) in enumerate(zip(got, want)):
                assert g["labels"].dtype == np.uint8 and g["labels"].shape == lab.shape, (k, posts, resized)
                assert g["labels"].tobytes() == lab.tobytes(), (k, posts, resized)
                assert sorted(g["masks"]) == ["color", "inverted", "overlay"]
                for name in g["masks"]:
                    assert g["masks"][name] == masks[name], (k, name, posts, resized)
    # other output sets: the k-th requested mask is not mask k
    want = [_single(eng, p, ["cc_vote"], False, level) for p in pages]
    for which in (("overlay",), NAMES, ("fg_color", "color")):
        got = eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=LUT, which=which,
                                      png_level=level, unit_cap=2)
        for g, (_, masks) in zip(got, want):
            assert g["labels"] is None and g["masks"] == {n: masks[n] for n in which}, which
    # the default unit size and one unit for all same-shape pages give the same bytes; labels alone need neither table nor binarisation
    for cap in (0, 8):
        got = eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=LUT, png_level=level,
                                      unit_cap=cap)
        assert [g["masks"] for g in got] == [{n: m[n] for n in NAMES[:3]} for _, m in want]
    got = eng.predict_chain_pages([p[0] for p in pages], which=(), labels=True, unit_cap=2)
    bare = [np.array(eng.predict_chain(p[0], labels="u8")["labels"]) for p in pages]
    assert all(g["masks"] == {} and np.array_equal(g["labels"], b) for g, b in zip(got, bare))


def test_sink_contract(gpu, engines):
    eng = engines[gpu.MODE_BF16]
    pages = _pages()
    imgs, bins = [p[0] for p in pages], [p[1] for p in pages]
    full = eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2)
    calls = []
    assert eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2,
                                   sink=lambda page, name, data: calls.append((page, name, data))) is None
    order = ["color", "overlay", "inverted", "labels"]
    assert [(c[0], c[1]) for c in calls] == [(k, n) for k in range(len(pages)) for n in order]
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
        if page == 3:
            raise Stop("page 3")

    with pytest.raises(Stop, match="page 3"):
        eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, unit_cap=2, sink=raising)
    assert seen == [(k, n) for k in range(3) for n in order[:3]] + [(3, "color")]       # nothing behind the call that raised
    # the raw return code of a sink that says stop, then the engine again: the full, correct result
    from pseg_amd import engine as E
    L = gpu.lib()
    P, I = ctypes.c_void_p * 7, ctypes.c_int * 7
    stop = E.CHAIN_SINK(lambda user, page, which, data, n: 1 if page == 1 else 0)
    rc = L.pseg_predict_chain_pages_png(eng._h, 7, P(*[a.ctypes.data for a in imgs]), I(*[s[0] for s in SHAPES]), I(*[s[1] for s in SHAPES]), None, None,
                                        P(*[b.ctypes.data for b in bins]), (ctypes.c_int * 1)(1), 1, 0, LUT.ctypes.data, 3, 0, 7, 2, stop, None)
    assert rc == -6 and b"sink" in L.pseg_last_error()
    again = eng.predict_chain_pages(imgs, binaries=bins, post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2)
    assert all(a["masks"] == f["masks"] and np.array_equal(a["labels"], f["labels"]) for a, f in zip(again, full))
    assert eng.predict_chain_pages([], lut=LUT) == []
    never = E.CHAIN_SINK(lambda *a: pytest.fail("sink called for an empty list"))
    assert L.pseg_predict_chain_pages_png(eng._h, 0, None, None, None, None, None, None, None, 0, 0, LUT.ctypes.data, 3, 0, 7, 0, never, None) == 0


def test_argument_errors(gpu, engines):
    from pseg_amd import engine as E
    eng = engines[gpu.MODE_F32_EXACT]
    L = gpu.lib()
    pages = _pages([A, B, A])
    imgs, bins = [p[0] for p in pages], [p[1] for p in pages]
    P, I = ctypes.c_void_p * 3, ctypes.c_int * 3
    ip, bp = P(*[a.ctypes.data for a in imgs]), P(*[b.ctypes.data for b in bins])
    hs, ws = I(A[0], B[0], A[0]), I(A[1], B[1], A[1])
    called = []
    sink = E.CHAIN_SINK(lambda *a: called.append(a) or 0)
    vote = (ctypes.c_int * 1)(1)

    def run(binaries=bp, ops=vote, n_post=1, level=0, want=7, cb=sink):
        return L.pseg_predict_chain_pages_png(eng._h, 3, ip, hs, ws, None, None, binaries, ops, n_post, 0, LUT.ctypes.data, 3, level, want, 2, cb, None)

    assert run(binaries=P(bins[0].ctypes.data, None, bins[2].ctypes.data)) == -1
    msg = L.pseg_last_error()
    assert b"page 1" in msg and b"binarisation" in msg
    assert run(binaries=None, want=16) == -1 and b"page 0" in L.pseg_last_error()          # the vote alone needs it too
    assert run(level=2) == -1 and b"level" in L.pseg_last_error()
    assert run(ops=(ctypes.c_int * 1)(9)) == -1 and b"post-processor" in L.pseg_last_error()
    assert run(want=0) == -1 and b"want" in L.pseg_last_error()
    assert run(want=32) == -1 and b"want" in L.pseg_last_error()
    assert run(cb=ctypes.cast(None, E.CHAIN_SINK)) == -1 and b"sink" in L.pseg_last_error()
    assert called == []
    assert run() == 0 and len(called) == 9                                                  # the same arguments, all valid


def _predictor_and_dataset(gpu, oracle_mod, posts, high_res):
    import dataclasses
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=True)
    net.model.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    data = []
    for k, s in enumerate([A, A, B, A, B]):
        img, binary, _ = synth.synth_page(20 + k, s[0], s[1], 3)
        d = SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page%d.png" % k)
        if high_res:
            orig = (s[0] + 71, s[1] + 41)
            d = dataclasses.replace(d, original_shape=orig, orig_binary=(np.random.default_rng(k).random(orig) < 0.2).astype(np.uint8))
        data.append(d)
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor(p) for p in posts], high_res_output=high_res)
    return Predictor(settings, net), Dataset(data, cm)


def _files(paths_per_page):
    return [[open(p, "rb").read() for p in paths] for paths in paths_per_page]


@pytest.mark.parametrize("posts,high_res", [(["cc_majority"], False), (["cc_majority", "bounding_boxes"], True)])
@pytest.mark.parametrize("level", [0, 1])
def test_write_masks_dataset(gpu, oracle_mod, tmp_path, posts, high_res, level):
    from ocr4all_pixel_classifier.lib import output
    pred, ds = _predictor_and_dataset(gpu, oracle_mod, posts, high_res)
    want_paths = [pred.write_masks(d, str(tmp_path / "single"), level=level) for d in ds.data]
    want = _files(want_paths)
    got_paths = list(pred.write_masks_dataset(ds, str(tmp_path / "list"), level=level))
    assert [[os.path.relpath(p, str(tmp_path / "list")) for p in paths] for paths in got_paths] == \
           [[os.path.relpath(p, str(tmp_path / "single")) for p in paths] for paths in want_paths]
    assert _files(got_paths) == want
    assert _files(pred.write_masks_dataset(ds, str(tmp_path / "chunks"), level=level, chunk_pages=2)) == want
    # where the device list path does not apply, write_masks' files again
    try:
        output.DEVICE_PNG = False
        pil = [pred.write_masks(d, str(tmp_path / "pil_single"), level=level) for d in ds.data]
        assert _files(pred.write_masks_dataset(ds, str(tmp_path / "pil_list"), level=level)) == _files(pil)
    finally:
        output.DEVICE_PNG = True
    pred.settings.post_process = list(pred.settings.post_process) + [lambda lab, d: lab]
    assert pred._chain_ops() is None
    host = [pred.write_masks(d, str(tmp_path / "host_single"), level=level) for d in ds.data]
    assert _files(pred.write_masks_dataset(ds, str(tmp_path / "host_list"), level=level)) == _files(host)
