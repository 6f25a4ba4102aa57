"""Host side of the device-resident augmentation (Network.train_dataset -> Engine.train_forward_backward_augmented): the NumPy
random stream of the draw helper against the two flow() calls it replaces, and the packing of the transform parameters into the
entry's (matrix, offset, flips) arguments.  No GPU: apply_transform (the pixel work) is patched out."""
import numpy as np
import pytest

from ocr4all_pixel_classifier.lib import data_generator as DG
from ocr4all_pixel_classifier.lib.data_generator import ImageDataGeneratorCustom as G
from ocr4all_pixel_classifier.lib.trainer import AugmentationSettings


def _states_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("brightness_range", [None, [0.6, 1.4]])
@pytest.mark.parametrize("seed", [1, 7, 12345])
def test_draw_helper_leaves_the_random_stream_of_the_two_flows(monkeypatch, brightness_range, seed):
    s = AugmentationSettings(horizontal_flip=True, vertical_flip=True, brightness_range=brightness_range)
    gi, gm = G(**s.to_image_params(), data_format='channels_last'), G(**s.to_mask_params(), data_format='channels_last')
    seen = []

    def identity(self, x, params):
        seen.append(dict(params))
        return np.asarray(x, dtype=np.float32)
    monkeypatch.setattr(G, "apply_transform", identity)
    img = np.zeros((1, 24, 40, 1), np.uint8)
    msk = np.zeros((1, 24, 40, 1), np.uint8)
    np.random.seed(99)                                   # whatever state training is in: both flows re-seed
    next(gi.flow(img, seed=seed, batch_size=1))
    next(gm.flow(msk, seed=seed, batch_size=1))
    want_state = np.random.get_state()
    want_after = np.random.random(3)                     # what the next epoch's shuffle would see
    np.random.seed(99)
    p_img, p_mask = DG.draw_sample_transforms(gi, gm, (24, 40, 1), (24, 40, 1), seed)
    assert _states_equal(np.random.get_state(), want_state)
    assert np.array_equal(np.random.random(3), want_after)
    assert [p_img, p_mask] == seen
    assert (p_img['brightness'] is None) == (brightness_range is None) and p_mask['brightness'] is None
    assert all(p_img[k] == p_mask[k] for k in p_mask if k != 'brightness')


def test_argument_packing():
    p = {'theta': 2.0, 'tx': 1.5, 'ty': -2.0, 'shear': 0.0, 'zx': 0.97, 'zy': 1.04, 'flip_horizontal': False, 'flip_vertical': False}
    m, off, flips = DG.device_transform_args(p, 48, 80)
    wm, woff = G.affine_matrix(p, 48, 80)
    assert m.dtype == np.float64 and m.shape == (4,) and m.flags.c_contiguous and np.array_equal(m, wm.reshape(4))
    assert off.dtype == np.float64 and off.shape == (2,) and np.array_equal(off, woff)
    assert flips == 0
    ident = {'theta': 0, 'tx': 0, 'ty': 0, 'shear': 0, 'zx': 1, 'zy': 1}
    for fh, fv, bits in [(False, False, 0), (True, False, 1), (False, True, 2), (True, True, 3), (np.True_, 0, 1), (0, np.True_, 2)]:
        m, off, flips = DG.device_transform_args(dict(ident, flip_horizontal=fh, flip_vertical=fv), 48, 80)
        assert m is None and off is None and flips == bits          # NULL / NULL: the generator skips the warp for the identity
    assert DG.device_transform_args(dict(p, flip_horizontal=True, flip_vertical=True), 48, 80)[2] == 3


def test_settings_the_device_path_does_not_cover():
    def gens(**kw):
        s = AugmentationSettings(**kw)
        return G(**s.to_image_params(), data_format='channels_last'), G(**s.to_mask_params(), data_format='channels_last')
    assert DG.device_path_covers(*gens())
    assert DG.device_path_covers(*gens(mask_fill_mode='constant', mask_cval=255, image_fill_mode='wrap', brightness_range=[0.5, 1.5]))
    assert not DG.device_path_covers(*gens(mask_fill_mode='constant', mask_cval=300))
    assert not DG.device_path_covers(*gens(mask_fill_mode='constant', mask_cval=-1))
    assert not DG.device_path_covers(*gens(mask_fill_mode='constant', mask_cval=2.5))
    gi, gm = gens()
    assert not DG.device_path_covers(G(**dict(AugmentationSettings().to_image_params(), rescale=1 / 255.), data_format='channels_last'), gm)
    assert not DG.device_path_covers(gi, G(**dict(AugmentationSettings().to_mask_params(), preprocessing_function=lambda x: x),
                                           data_format='channels_last'))
    assert not DG.device_path_covers(gi, G(**AugmentationSettings(rotation_range=9.0).to_mask_params(), data_format='channels_last'))
    assert not DG.device_path_covers(G(**dict(AugmentationSettings().to_image_params(), dtype='float64'), data_format='channels_last'), gm)
