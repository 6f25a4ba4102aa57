"""The tile plan of tiled prediction (pseg_tile_plan): its invariants over random shapes, its argument errors, and the
plan against the CPU oracle -- float32 logits stitched from the plan's tiles equal the whole page's, bit for bit.  No GPU."""
import ctypes

import numpy as np
import pytest

HALO = {"fcn_skip": 96, "fcn": 96, "unet": 160, "res_unet": 160}


def _up32(v):
    return (v + 31) // 32 * 32


def _check_plan(arch, H, W, tile):
    """The four invariants, on an ownership count array painted from the plan's rectangles."""
    from pseg_amd import engine as E
    halo = HALO[arch]
    (th, tw), org, own = E.tile_plan(arch, (H, W), tile)
    Hp, Wp = _up32(H), _up32(W)
    T = tile or 2048
    assert (th, tw) == (min(T, Hp), min(T, Wp)), (arch, H, W, tile)
    o, r = np.asarray(org, np.int64).reshape(-1, 2), np.asarray(own, np.int64).reshape(-1, 4)
    assert len(o) == len(r) >= 1
    assert (o % 32 == 0).all(), "origins on the 32-pixel grid"
    assert (o >= 0).all() and (o[:, 0] + th <= Hp).all() and (o[:, 1] + tw <= Wp).all(), "tiles inside the canvas"
    assert (r[:, 0] < r[:, 1]).all() and (r[:, 2] < r[:, 3]).all()
    # an owned rectangle lies inside its tile, at least halo from every tile edge that is not a canvas edge
    for lo, hi, y, t, Np in ((r[:, 0], r[:, 1], o[:, 0], th, Hp), (r[:, 2], r[:, 3], o[:, 1], tw, Wp)):
        assert (np.where(y == 0, lo == 0, lo - y >= halo)).all(), (arch, H, W, tile)
        assert (np.where(y + t == Np, hi == Np, y + t - hi >= halo)).all(), (arch, H, W, tile)
    # every canvas pixel has exactly one owner: +1 / -1 at the rectangles' corners, summed up along both axes
    cnt = np.zeros((Hp + 1, Wp + 1), np.int32)
    np.add.at(cnt, (r[:, 0], r[:, 2]), 1)
    np.add.at(cnt, (r[:, 1], r[:, 3]), 1)
    np.add.at(cnt, (r[:, 0], r[:, 3]), -1)
    np.add.at(cnt, (r[:, 1], r[:, 2]), -1)
    cnt = cnt.cumsum(0).cumsum(1)[:Hp, :Wp]
    assert cnt.min() == 1 and cnt.max() == 1, (arch, H, W, tile)
    return len(o)


def test_tile_plan_invariants_over_random_shapes():
    rng = np.random.RandomState(7)
    cases = [("fcn_skip", 1, 1, 224), ("unet", 1, 1, 352), ("fcn", 5000, 5000, 224), ("res_unet", 5000, 5000, 352), ("fcn_skip", 5000, 1, 0),
             ("unet", 33, 4999, 2048), ("fcn_skip", 300, 260, 256), ("fcn_skip", 200, 700, 256), ("unet", 500, 420, 384)]
    while len(cases) < 200:
        arch = ("fcn_skip", "fcn", "unet", "res_unet")[rng.randint(4)]
        lo = 2 * HALO[arch] + 32
        H, W = (int(np.exp(rng.uniform(0, np.log(5000.999)))) for _ in range(2))
        tile = 32 * int(rng.randint(lo // 32, 2048 // 32 + 1)) if rng.randint(8) else 0
        cases.append((arch, H, W, tile))
    counts = [_check_plan(*c) for c in cases]
    assert counts[0] == 1 and counts[2] == 151 * 151 and max(counts) > 1000
    # the shapes of the issue's table
    assert counts[6] == 4 and counts[7] == 8 and counts[8] == 6


def test_tile_plan_argument_errors():
    import pseg_amd
    from pseg_amd import engine as E
    L = pseg_amd.lib()
    assert "pseg_tile_plan" in E.EXPORTED_SYMBOLS and "pseg_predict_tiled_device" in E.EXPORTED_SYMBOLS and "pseg_engine_set_tiling" in E.EXPORTED_SYMBOLS
    for arch, tile in (("fcn_skip", 250), ("fcn_skip", 192), ("unet", 320), ("unet", 353), ("fcn", -32)):
        with pytest.raises(E.PsegError, match="tile"):
            E.tile_plan(arch, (300, 300), tile)
    assert E.tile_plan("fcn_skip", (300, 300), 224)[0] == (224, 224) and E.tile_plan("unet", (300, 300), 352)[0] == (320, 320)
    for shape in ((0, 10), (10, -1)):
        with pytest.raises(E.PsegError, match="shape"):
            E.tile_plan("fcn", shape)
    with pytest.raises(E.PsegError, match="architecture"):
        E.tile_plan(9, (64, 64))
    # the count alone needs no arrays; arrays need room
    th, tw = ctypes.c_int(), ctypes.c_int()
    assert L.pseg_tile_plan(0, 420, 300, 256, ctypes.byref(th), ctypes.byref(tw), None, None, None, 0) == 8
    oy = np.zeros(8, np.int32)
    assert L.pseg_tile_plan(0, 420, 300, 256, None, None, oy.ctypes.data_as(ctypes.c_void_p), None, None, 7) == -1
    assert L.pseg_tile_plan(0, 420, 300, 256, None, None, oy.ctypes.data_as(ctypes.c_void_p), None, None, 8) == 8
    assert list(oy) == [0, 0, 64, 64, 128, 128, 192, 192]
    # no engine: the argument checks of the engine entries come first
    assert L.pseg_engine_set_tiling(None, 1, 0) == -1 and L.pseg_engine_page_fits(None, 10, 10) == -1
    assert L.pseg_predict_tiled_device(None, None, 10, 10, 0, None, None, None) == -1


def _stitched_logits(oracle_mod, arch, Wt, img, tile):
    from pseg_amd import engine as E
    H, W = img.shape
    (th, tw), org, own = E.tile_plan(arch, (H, W), tile)
    out = None
    for (y, x), (y0, y1, x0, x1) in zip(org, own):
        t = np.zeros((th, tw), np.uint8)
        part = img[y:y + th, x:x + tw]
        t[:part.shape[0], :part.shape[1]] = part
        z = oracle_mod.forward(arch, Wt, t)
        if out is None:
            out = np.full((H, W, z.shape[2]), np.nan, np.float32)
        y1, x1 = min(y1, H), min(x1, W)
        out[y0:y1, x0:x1] = z[y0 - y:y1 - y, x0 - x:x1 - x]
    return out, len(org)


@pytest.mark.parametrize("arch,shape,tile,tiles", [("fcn_skip", (300, 260), 256, 4), ("fcn_skip", (420, 300), 256, 8), ("fcn_skip", (200, 700), 256, 8),
                                                   ("unet", (500, 420), 384, 6)])
def test_stitched_oracle_logits_equal_the_whole_page(oracle_mod, arch, shape, tile, tiles):
    from pseg_amd import synth
    img, _, _ = synth.synth_page(3, shape[0], shape[1])
    Wt = oracle_mod.init_weights(arch, 3, seed=42, gain=1.5, bias_scale=0.05)
    whole = oracle_mod.forward(arch, Wt, img)
    got, n = _stitched_logits(oracle_mod, arch, Wt, img, tile)
    assert n == tiles
    assert np.array_equal(got, whole)


# ---- Predictor: a page the whole-page path refuses leaves the list entries for write_masks, in place --------------------------------
class _StubEngine:
    def __init__(self, log, refused):
        self.log, self.refused = log, refused

    def page_fits(self, H, W):
        return (H, W) not in self.refused

    def predict_chain_pages(self, images, binaries=None, out_shapes=None, post_ops=(), exact_labels=False, lut=None, which=(), labels=False,
                            png_level=0, unit_cap=0, sink=None, mixed=False):
        self.log.append(("pages", [im.shape for im in images]))
        for page in range(len(images)):
            for name in which:
                sink(page, name, b"x")

    def predict_chain_scans(self, scans, scales, high_res=False, post_ops=(), exact_labels=False, lut=None, which=(), labels=False, png_level=0,
                            unit_cap=0, sink=None):
        self.log.append(("scans", [int(s[0, 0]) for s in scans]))
        for page in range(len(scans)):
            for name in which:
                sink(page, name, b"x")


class _StubNetwork:
    n_classes = 3
    _rgb = False
    exact = False

    def __init__(self, log, refused):
        self.model = _StubEngine(log, refused)


class _StubLoader:
    target_line_height = 6
    max_width = None

    def load_images(self, entry):
        return entry


def test_predictor_sends_refused_pages_through_write_masks(tmp_path, monkeypatch):
    import os
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    from ocr4all_pixel_classifier.lib import dataset, output
    log = []
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    pred = Predictor(PredictSettings(n_classes=3, color_map=cm, post_process=[]), _StubNetwork(log, {(64, 48), (16, 12)}))
    monkeypatch.setattr(pred, "write_masks", lambda data, output_dir=None, level=None: log.append(("write_masks", os.path.basename(data.image_path))))
    shapes = [(32, 40), (64, 48), (32, 40)]
    data = [SingleData(image=np.zeros(s, np.uint8), binary=np.ones(s, np.uint8), original_shape=s, image_path="/in/p%d.png" % k) for k, s in enumerate(shapes)]
    got = list(pred.write_masks_dataset(Dataset(data, cm), str(tmp_path)))
    assert got == [output.output_paths(str(tmp_path), d) for d in data]
    assert log == [("pages", [(32, 40), (32, 40)]), ("write_masks", "p1.png")]
    # the scan route: scan k is a (40, 30) plane of k, line height 12 + k; scan 3 becomes a (16, 12) page
    del log[:]
    monkeypatch.setattr(dataset, "_imread_gray", lambda path: np.full((40, 30), int(os.path.basename(path)[4:-4]), np.uint8))
    entries = [SingleData(image_path="/in/scan%d.png" % k, line_height_px=12 + k) for k in range(5)]
    got = list(pred.write_masks_scans(entries, _StubLoader(), str(tmp_path)))
    assert got == [output.output_paths(str(tmp_path), e) for e in entries]
    assert log == [("scans", [0, 1, 2, 4]), ("write_masks", "scan3.png")]
    # a model object without page_fits refuses nothing
    del pred.network.model.__class__.page_fits
    assert pred._list_takes((64, 48))
