"""Device-resident augmentation (pseg_train_forward_backward_aug / pseg_train_augment_sample): one call takes the uint8 page,
the uint8 mask and one set of transform parameters and builds the training sample of lib/network.py:149-161 on the device.  The
sample must equal, bit for bit, what the host-array path builds (ImageDataGeneratorCustom.apply_transform: one
pseg_affine_warp_fill per channel, NumPy flips, pseg_brightness_shift; the mask generator followed by astype(uint8)) -- that path
is itself pinned against the installed scipy and Pillow by tests/test_augment_gpu.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the transforms of tests/test_augment_gpu.py (theta, tx, ty, zx, zy), then the identity (no warp: flips only / no-op)
TRANSFORMS = [(2.5, 1.6, -2.4, 0.95, 1.05), (-1.3, 0.0, 0.0, 1.0, 1.0), (0.0, 3.0, 2.0, 1.0, 1.0), (40.0, 5.0, -7.0, 0.7, 1.4),
              (-170.0, 90.5, -140.25, 2.5, 0.4), (0.0, 0.0, 0.0, 1.0, 1.0)]
FILLS = [("nearest", 0), ("constant", 0), ("constant", 3), ("constant", 255), ("reflect", 0), ("wrap", 0)]
FLIPS = [(False, False), (True, False), (False, True), (True, True)]
# (1,9): the one-sample line scipy leaves alone; (7,5), (33,50), (200,31): lines under 28 samples (closed forms); (64,96): exactly one
# 64-sample chunk; (65,129): one chunk plus one, two chunks plus one; (257,131), (300,520): line counts that are no multiple of 64,
# several chunks on both axes (with 'nearest' the plane is padded by 12 on every side: (64,96) -> 88 x 120, (40,..) would be 64)
SHAPES = [(1, 9), (7, 5), (33, 50), (64, 96), (65, 129), (200, 31), (257, 131), (300, 520)]


def _params(theta, tx, ty, zx, zy, fh=False, fv=False, brightness=None):
    return {'theta': theta, 'tx': tx, 'ty': ty, 'shear': 0.0, 'zx': zx, 'zy': zy, 'flip_horizontal': fh, 'flip_vertical': fv,
            'brightness': brightness}


def _generators(fill, cval, mask_fill=None, mask_cval=None):
    from ocr4all_pixel_classifier.lib.data_generator import ImageDataGeneratorCustom as G
    from ocr4all_pixel_classifier.lib.trainer import AugmentationSettings
    s = AugmentationSettings(image_fill_mode=fill, image_cval=cval, mask_fill_mode=mask_fill or fill,
                             mask_cval=cval if mask_cval is None else mask_cval)
    return G(**s.to_image_params(), data_format='channels_last'), G(**s.to_mask_params(), data_format='channels_last')


def _host_sample(gi, gm, img, mask, p):
    """The host-array path of Network.train_dataset for one sample and given parameters."""
    x = gi.apply_transform(img if img.ndim == 3 else img[..., None], p)
    m = gm.apply_transform(mask[..., None], dict(p, brightness=None))[..., 0].astype(np.uint8)
    return (x[..., 0] if img.ndim == 2 else x), m


def _device_sample(eng, gi, gm, img, mask, p):
    from ocr4all_pixel_classifier.lib.data_generator import device_transform_args
    matrix, offset, flips = device_transform_args(p, img.shape[0], img.shape[1])
    return eng.augment_sample(img, mask, matrix, offset, flips, gi.fill_mode, gi.cval, gm.fill_mode, gm.cval, p['brightness'])


@pytest.fixture(scope="module")
def engines(gpu):
    """One float32 train engine per channel count (the sample builder needs pseg_train_init, no weights, no canvas)."""
    out = {}
    for ch in (1, 3):
        e = gpu.Engine("fcn_skip", 3, in_channels=ch, mode=gpu.MODE_F32_EXACT)
        e.train_init()
        out[ch] = e
    yield out
    for e in out.values():
        e.close()


def _page(shape, channels, seed):
    rng = np.random.default_rng(seed)
    img = (rng.random(shape + ((3,) if channels == 3 else ())) * 256).astype(np.uint8)
    mask = rng.integers(0, 6, shape).astype(np.uint8)
    return img, mask


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_equals_the_host_array_path(engines, shape, channels):
    """All four fill modes ('constant' with cval 0, 3, 255) x the warp tests' transforms, flips only and the no-op x the four
    flip combinations: image and mask equal the host-array path's bit for bit."""
    img, mask = _page(shape, channels, shape[0] * 7 + channels)
    eng = engines[channels]
    for fill, cval in FILLS:
        gi, gm = _generators(fill, cval)
        for t in TRANSFORMS:
            for fh, fv in FLIPS:
                p = _params(*t, fh=fh, fv=fv)
                want_i, want_m = _host_sample(gi, gm, img, mask, p)
                got_i, got_m = _device_sample(eng, gi, gm, img, mask, p)
                assert got_i.dtype == np.float32 and got_m.dtype == np.uint8
                assert got_i.shape == want_i.shape and got_m.shape == want_m.shape
                assert np.array_equal(got_i, want_i), (fill, cval, t, fh, fv, float(np.abs(got_i - want_i).max()))
                assert np.array_equal(got_m, want_m), (fill, cval, t, fh, fv, int((got_m != want_m).sum()))


def test_image_and_mask_fill_modes_are_independent(engines):
    """lib/trainer.py:23-28 names the image's and the mask's fill mode / value separately."""
    img, mask = _page((65, 129), 3, 5)
    for (ifill, icval), (mfill, mcval) in [(("nearest", 0), ("constant", 7)), (("constant", 200), ("reflect", 0)),
                                           (("reflect", 0), ("wrap", 0)), (("wrap", 0), ("nearest", 0))]:
        gi, gm = _generators(ifill, icval, mfill, mcval)
        p = _params(40.0, 5.0, -7.0, 0.7, 1.4, fh=True)
        want_i, want_m = _host_sample(gi, gm, img, mask, p)
        got_i, got_m = _device_sample(engines[3], gi, gm, img, mask, p)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_m, want_m), (ifill, mfill)


@pytest.mark.parametrize("channels,shape", [(1, (65, 129)), (3, (33, 50))])
def test_brightness_stretch_branch(engines, channels, shape):
    """A 0/255 checkerboard under rotation: the cubic overshoot leaves [0, 255], so apply_brightness_shift stretches the sample to
    8 bit and maps it back (min / max over all channels, reduced per wave in the fused warp)."""
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    board = (((yy // 3 + xx // 3) % 2) * 255).astype(np.uint8)
    img = board if channels == 1 else np.stack([board, 255 - board, board[::-1]], -1)
    mask = (board // 255).astype(np.uint8)
    for fill in ("nearest", "reflect"):
        gi, gm = _generators(fill, 0)
        for fh, fv in FLIPS[::3]:
            plain, _ = _host_sample(gi, gm, img, mask, _params(7.0, 1.5, -2.0, 1.1, 0.9, fh=fh, fv=fv))
            assert plain.min() < 0.0 or plain.max() > 255.0
            for b in (0.6, 1.4):
                p = _params(7.0, 1.5, -2.0, 1.1, 0.9, fh=fh, fv=fv, brightness=b)
                want_i, want_m = _host_sample(gi, gm, img, mask, p)
                got_i, got_m = _device_sample(engines[channels], gi, gm, img, mask, p)
                assert not np.array_equal(want_i, plain)
                assert np.array_equal(got_i, want_i), (fill, fh, fv, b, float(np.abs(got_i - want_i).max()))
                assert np.array_equal(got_m, want_m)
    # in-range samples take the other branch: no warp, the exact uint8 values
    gi, gm = _generators("nearest", 0)
    p = _params(0.0, 0.0, 0.0, 1.0, 1.0, fv=True, brightness=1.4)
    want_i, want_m = _host_sample(gi, gm, img, mask, p)
    got_i, got_m = _device_sample(engines[channels], gi, gm, img, mask, p)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_m, want_m)


@pytest.mark.parametrize("channels", [1, 3])
def test_step_equals_the_float_entry(gpu, oracle_mod, channels):
    """train_forward_backward_augmented against train_forward_backward_float(host sample, host mask) on fresh engines with the
    same weights: the bars of test_float_page_training_entry_and_augmented_training for the same comparison."""
    from pseg_amd import synth
    gray, _, mask = synth.synth_page(2, 96, 112, 3)
    img = gray if channels == 1 else np.stack([gray, 255 - gray, gray[::-1]], -1)
    Wt = oracle_mod.init_weights("fcn_skip", 3, seed=3, in_ch=channels, gain=1.0, bias_scale=0.02)
    gi, gm = _generators("nearest", 0)
    p = _params(2.5, 1.6, -2.4, 0.95, 1.05, fh=True, brightness=1.2)
    host_i, host_m = _host_sample(gi, gm, img, mask, p)
    from ocr4all_pixel_classifier.lib.data_generator import device_transform_args
    matrix, offset, flips = device_transform_args(p, 96, 112)
    res = []
    for device_path in (True, False):
        e = gpu.Engine("fcn_skip", 3, in_channels=channels, mode=gpu.MODE_F32_EXACT)
        e.set_weights(Wt)
        e.train_init()
        if device_path:
            row = e.train_forward_backward_augmented(img, mask, matrix, offset, flips, "nearest", 0, "nearest", 0, p['brightness'])
        else:
            row = e.train_forward_backward_float(host_i, host_m)
        res.append((row, e.gradients()))
        e.close()
    (a, ga), (b, gb) = res
    assert np.isfinite(a).all() and np.allclose(a, b, rtol=1e-6, atol=0)
    assert all(np.allclose(ga[k], gb[k], rtol=1e-4, atol=1e-6 * np.abs(gb[k]).max()) for k in gb)


def _train(tmp_path, tag, device_augmentation, epochs=2, **aug):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.trainer import Trainer, TrainSettings, AugmentationSettings
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    from ocr4all_pixel_classifier.lib.metrics import Monitor

    def ds(seeds):
        out = []
        for s in seeds:
            i, bi, m = synth.synth_page(s, 96, 96, 3)
            out.append(SingleData(image=i, binary=bi, mask=m, original_shape=i.shape))
        return Dataset(out, ColorMap({}))
    np.random.seed(0)                    # the untrained network's weights, every epoch's shuffle
    settings = TrainSettings(n_epoch=epochs, n_classes=3, l_rate=2e-3, train_data=ds([0, 1, 2, 3]), validation_data=ds([4]),
                             display=1, output_dir=str(tmp_path / tag), threads=1, monitor=Monitor.VAL_LOSS, data_augmentation=True,
                             data_augmentation_settings=AugmentationSettings(horizontal_flip=True, vertical_flip=True,
                                                                             brightness_range=[0.6, 1.4], **aug))
    t = Trainer(settings)
    t.train_net.device_augmentation = device_augmentation
    calls = {"device": 0, "host": 0}
    eng = t.train_net.model
    dev, flt = eng.train_forward_backward_augmented, eng.train_forward_backward_float

    def spy_dev(*a, **k):
        calls["device"] += 1
        return dev(*a, **k)

    def spy_flt(*a, **k):
        calls["host"] += 1
        return flt(*a, **k)
    eng.train_forward_backward_augmented, eng.train_forward_backward_float = spy_dev, spy_flt
    hist = t.train()
    state = np.random.get_state()
    eng.close()
    return hist, state, calls


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _spread(h1, h2):
    return max(float(np.abs(np.asarray(h1[k]) - np.asarray(h2[k])).max()) for k in ("loss", "val_loss"))


@pytest.fixture(scope="module")
def host_runs(gpu, tmp_path_factory):
    """The host-array path twice: its history, and its own run-to-run spread."""
    tmp = tmp_path_factory.mktemp("aug_host")
    return _train(tmp, "h1", False), _train(tmp, "h2", False)


def test_train_dataset_keeps_its_trajectory(gpu, host_runs, tmp_path):
    """Two epochs over four 96x96 pages with flips and a brightness range, device_augmentation True against False from the same
    seed: the NumPy random state afterwards is the same, and the loss histories differ by at most 4 s, where s is the host
    path's own run-to-run spread (equal histories when s == 0).
    Measured on the MI355X: s = 0.0 (the step is bit-reproducible per device configuration), device against host 0.0."""
    (h1, st1, c1), (h2, st2, c2) = host_runs
    assert c1 == {"device": 0, "host": 8} and _same_state(st1, st2)
    s = _spread(h1, h2)
    hd, std, cd = _train(tmp_path, "dev", True)
    d = _spread(hd, h1)
    print("host run-to-run spread s = %r; device vs host = %r" % (s, d))
    assert cd == {"device": 8, "host": 0}
    assert _same_state(std, st1)
    assert np.isfinite(hd["loss"]).all()
    if s == 0:
        assert d == 0
    else:
        assert d <= 4 * s


def test_fallbacks(gpu, host_runs, tmp_path):
    """A mask fill value no uint8 holds, and device_augmentation = False, take the host-array path; the C entry refuses the value."""
    hd, std, cd = _train(tmp_path, "cval_dev", True, mask_fill_mode="constant", mask_cval=300)
    hh, sth, ch = _train(tmp_path, "cval_host", False, mask_fill_mode="constant", mask_cval=300)
    assert cd == ch == {"device": 0, "host": 8}
    assert _same_state(std, sth)
    (h1, _, _), (h2, _, _) = host_runs
    s = _spread(h1, h2)
    assert _spread(hd, hh) == 0 if s == 0 else _spread(hd, hh) <= 4 * s
    from pseg_amd import engine as E
    e = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_F32_EXACT)
    e.train_init()
    img, mask = _page((33, 50), 1, 1)
    out = (ctypes.c_float * 4)()
    for bad in (300.0, -1.0, 2.5):
        rc = E.lib().pseg_train_forward_backward_aug(e._h, E._ptr(img), E._ptr(mask), 33, 50, None, None, 0, 0, 0.0, 1, bad, 0, 0.0, out)
        assert rc == -1                                            # PSEG_EINVAL
    with pytest.raises(E.PsegError):
        e.augment_sample(img, mask, None, None, 0, "nearest", 0, "constant", 300)
    with pytest.raises(E.PsegError):
        e.augment_sample(img, mask, np.eye(2), None, 0, "nearest", 0, "nearest", 0)
    e.close()
