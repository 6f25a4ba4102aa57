"""Tiled prediction on the GPU (pseg_predict_tiled_device, pseg_engine_set_tiling): the label map stitched from the
plan's tiles is array_equal to the whole page's on both engines -- no tolerance --, through the page-slot units and tile by tile, in
the chain, and for a page the bf16 engine refuses whole.  Small pages: 256-pixel tiles with the 96-pixel halo of fcn / fcn_skip give
1 to 8 tiles at 33x1 ... 420x300 (8 tiles: a page-slot unit), 384-pixel tiles with unet's 160 give 6 at 500x420."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
FCN_SHAPES = [(300, 260), (420, 300), (200, 700), (33, 1), (256, 256)]
FCN_TILES = [4, 8, 8, 1, 1]


def _engine(gpu, oracle_mod, arch, n_classes, mode, in_ch=1, plan=None):
    e = gpu.Engine(arch, n_classes, in_channels=in_ch, mode=mode, plan=plan)
    e.set_weights(oracle_mod.init_weights(arch, n_classes, seed=42, in_ch=in_ch, gain=1.5, bias_scale=0.05))
    return e


def _page(seed, H, W, n_classes=3):
    """A synthetic page; shapes too small for a layout are noise."""
    from pseg_amd import synth
    if min(H, W) < 32:
        return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    return synth.synth_page(seed, H, W, n_classes)[0]


def _whole(eng, img):
    return eng.predict(img, want_logits=False, want_probs=False)[2]


def _check_tiled(eng, img, tile):
    want = _whole(eng, img)
    got64 = eng.predict_tiled(img, tile)
    got8 = eng.predict_tiled(img, tile, dtype=np.uint8)
    assert got64.dtype == np.int64 and got8.dtype == np.uint8 and got64.shape == got8.shape == want.shape
    assert np.array_equal(got64, want)
    assert np.array_equal(got8, want)


@pytest.mark.parametrize("n_classes", [3, 6])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["fcn_skip", "fcn"])
def test_tiled_equals_whole_fcn(gpu, oracle_mod, arch, mode, n_classes):
    from pseg_amd import synth
    from pseg_amd import engine as E
    eng = _engine(gpu, oracle_mod, arch, n_classes, gpu.MODE_BF16 if mode == "bf16" else gpu.MODE_F32_EXACT)
    for k, (shape, tiles) in enumerate(zip(FCN_SHAPES, FCN_TILES)):
        assert len(E.tile_plan(arch, shape, 256)[1]) == tiles
        img = _page(10 + k, shape[0], shape[1], n_classes)
        _check_tiled(eng, img, 256)
    eng.close()


@pytest.mark.parametrize("n_classes", [3, 6])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["unet", "res_unet"])
def test_tiled_equals_whole_unet(gpu, oracle_mod, arch, mode, n_classes):
    from pseg_amd import synth
    from pseg_amd import engine as E
    eng = _engine(gpu, oracle_mod, arch, n_classes, gpu.MODE_BF16 if mode == "bf16" else gpu.MODE_F32_EXACT)
    assert len(E.tile_plan(arch, (500, 420), 384)[1]) == 6
    img, _, _ = synth.synth_page(20, 500, 420, n_classes)
    _check_tiled(eng, img, 384)
    eng.close()


def test_tiled_equals_whole_three_input_channels(gpu, oracle_mod):
    from pseg_amd import synth
    eng = _engine(gpu, oracle_mod, "fcn_skip", 3, gpu.MODE_BF16, in_ch=3)
    for k, shape in enumerate([(420, 300), (200, 701)]):       # (a row of 701 * 3 bytes: the cut kernel's byte-wise reads)
        g, _, _ = synth.synth_page(30 + k, shape[0], shape[1], 3)
        img = np.ascontiguousarray(np.stack([g, 255 - g, g // 2 + 17], -1))
        _check_tiled(eng, img, 256)
    eng.close()


def test_tile_units_and_the_tile_by_tile_route(gpu, oracle_mod):
    """32 tiles: two page-slot units of 16 on a bf16 engine; PSEG_NO_PAGE_BATCH runs the same tiles one by one."""
    from pseg_amd import synth
    from pseg_amd import engine as E
    assert len(E.tile_plan("fcn_skip", (700, 420), 256)[1]) == 32
    img, _, _ = synth.synth_page(40, 700, 420, 3)
    eng = _engine(gpu, oracle_mod, "fcn_skip", 3, gpu.MODE_BF16)
    want = _whole(eng, img)
    assert np.array_equal(eng.predict_tiled(img, 256), want)
    one = _engine(gpu, oracle_mod, "fcn_skip", 3, gpu.MODE_BF16, plan="PSEG_NO_PAGE_BATCH=1")
    assert np.array_equal(one.predict_tiled(img, 256, dtype=np.uint8), want)
    one.close()
    eng.close()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_chain_with_tiling_always(gpu, oracle_mod, mode):
    """Resize, vote, boxes and the PNG masks behind a tiled network stage: the bytes and maps of the same calls with tiling off."""
    from pseg_amd import synth
    eng = _engine(gpu, oracle_mod, "fcn_skip", 3, gpu.MODE_BF16 if mode == "bf16" else gpu.MODE_F32_EXACT)
    img, _, _ = synth.synth_page(50, 300, 260, 3)
    osh = (371, 301)
    big = (np.random.default_rng(5).random(osh) < 0.2).astype(np.uint8)

    def calls():
        out = []
        for level in (0, 1):
            r = eng.predict_chain(img, binary=big, out_shape=osh, post_ops=("cc_vote", "bbox"), labels="u8", lut=LUT, masks="png", png_level=level)
            out.append((np.array(r["labels"]), r["masks"]))
        r = eng.predict_chain(img, binary=big, out_shape=osh, post_ops=("bbox", "cc_vote"), labels="i64", lut=LUT, masks=True)
        out.append((np.array(r["labels"]), tuple(np.array(m).tobytes() for m in r["masks"])))
        out.append((np.array(eng.predict_chain(img, labels="u8")["labels"]), ()))
        return out

    want = calls()
    eng.set_tiling("always", 256)
    got = calls()
    for (gl, gm), (wl, wm) in zip(got, want):
        assert gl.dtype == wl.dtype and np.array_equal(gl, wl)
        assert gm == wm
    # predict and predict_device read the mode too (labels alone); logits keep the whole-page path
    assert np.array_equal(_whole(eng, img), want[3][0])
    z_on = eng.predict(img, want_probs=False)
    eng.set_tiling("off")
    z_off = eng.predict(img, want_probs=False)
    assert np.array_equal(z_on[0], z_off[0]) and np.array_equal(z_on[2], z_off[2])
    with pytest.raises(gpu.PsegError, match="tile"):
        eng.set_tiling("auto", 100)
    with pytest.raises(gpu.PsegError, match="tiling mode"):
        eng.set_tiling("sometimes")
    eng.close()


# ---- a page the bf16 engine refuses whole: 8192 x 8200 (a 64 B/px plane of fcn_skip reaches 4 GiB at 8192 x 8192) -----------------
BIG = (8192, 8200)


@pytest.fixture(scope="module")
def big(gpu, oracle_mod):
    """The page, its binarisation, the engine and the page's uint8 map in AUTO mode: computed once, shared, left unchanged."""
    from pseg_amd import synth
    from pseg_amd import engine as E
    base, binary, _ = synth.synth_page(60, 1024, 1025, 3)
    img, binary = np.tile(base, (8, 8)), np.tile(binary, (8, 8))
    assert img.shape == BIG
    eng = _engine(gpu, oracle_mod, "fcn_skip", 3, gpu.MODE_BF16)
    assert not eng.page_fits(*BIG) and eng.page_fits(2560, 2568)
    with pytest.raises(gpu.PsegError, match="4 GiB"):
        _whole(eng, img)                                   # tiling off: today's refusal
    assert len(E.tile_plan("fcn_skip", BIG, 1024)[1]) == 100
    eng.set_tiling("auto", 1024)
    lab = np.array(eng.predict_chain(img, labels="u8")["labels"])
    assert lab.shape == BIG and lab.dtype == np.uint8
    yield img, binary, eng, lab
    eng.close()


def test_refused_page_comes_back_in_auto_mode(gpu, big):
    img, _, eng, lab = big
    eng.set_tiling("off")
    try:
        # an interior crop across several tile seams (tiles own 832-pixel ranges from 928 on): the window 96 px inside the crop
        y0, x0, n = 2560, 3072, 2560
        sub = _whole(eng, np.ascontiguousarray(img[y0:y0 + n, x0:x0 + n]))
        assert np.array_equal(lab[y0 + 96:y0 + n - 96, x0 + 96:x0 + n - 96], sub[96:n - 96, 96:n - 96])
        # the crop that holds the page's bottom-right corner, from 32-aligned origins: everything 96 px from its top and left edges
        y0, x0 = 8192 - 2560, 5632
        sub = _whole(eng, np.ascontiguousarray(img[y0:, x0:]))
        assert sub.shape == (2560, 2568)
        assert np.array_equal(lab[y0 + 96:, x0 + 96:], sub[96:, 96:])
    finally:
        eng.set_tiling("auto", 1024)
    assert len(np.unique(lab)) > 1


def test_write_masks_of_a_refused_page(gpu, oracle_mod, big, tmp_path):
    from PIL import Image
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    img, binary, _, lab = big
    net = Network("Predict", n_classes=3, exact=False)            # (Network.tiling: "auto")
    net.model.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    pred = Predictor(PredictSettings(n_classes=3, color_map=cm, post_process=[], output=str(tmp_path)), net)
    data = SingleData(image=img, binary=binary, original_shape=img.shape, image_path="big.png")
    paths = pred.write_masks(data, level=0)
    assert not pred._list_takes(BIG) and pred._list_takes((96, 80))
    color = np.asarray(Image.open(paths[0]))
    assert color.shape == BIG + (3,) and np.array_equal(color, cm.lut()[lab])
    for p in paths[1:]:
        with Image.open(p) as im:
            assert im.size == (BIG[1], BIG[0]) and im.mode == "RGB"
    net.model.close()


def test_refusals_that_stay_and_trim(gpu, big):
    img, _, eng, lab = big
    # logits of an oversized page: no tiles, today's refusal -- also in AUTO mode
    with pytest.raises(gpu.PsegError, match="4 GiB"):
        eng.predict(img, want_probs=False, want_labels=False)
    with pytest.raises(gpu.PsegError, match="4 GiB"):
        eng.predict_chain(img, exact_labels=True, labels="u8")
    # after trim() a tiled call allocates its staging and the tile canvas again
    small = np.ascontiguousarray(img[:420, :300])
    want = eng.predict_tiled(small, 256, dtype=np.uint8)
    eng.trim()
    assert np.array_equal(eng.predict_tiled(small, 256, dtype=np.uint8), want)
    eng.set_tiling("off")
    assert np.array_equal(_whole(eng, small), want)
    eng.set_tiling("auto", 1024)
