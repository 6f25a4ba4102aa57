"""Augmented train step: what building the sample costs (lib/network.py:149-161 in Network.train_dataset).
Times, on one 3-class fcn_skip float32 engine and 2048x1536 synthetic pages (default AugmentationSettings plus a brightness range):
  (a) the host-array path: image_gen.flow / mask_gen.flow (one pseg_affine_warp_fill per plane, pseg_brightness_shift, NumPy
      in between) -> pseg_train_forward_backward_f32;
  (b) the device-resident entry: the draw helper -> pseg_train_forward_backward_aug;
  (c) the un-augmented pseg_train_forward_backward.
Wall time per sample after warm-up; every sample ends with the step's own synchronise (the metrics read).  (a) and (b) alternate
three times in one process.  Writes the table to --out."""
import argparse, os, sys, time
os.environ.setdefault("PSEG_PLAN_FROM_ENV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "page-segmentation_amd")]
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_device.txt"))
    a = ap.parse_args()
    try:
        import torch
        torch.cuda.is_available()           # torch's bundled HIP runtime initialises first (as bench.py)
    except ImportError:
        pass
    from pseg_amd import engine as E, synth
    from ocr4all_pixel_classifier.lib.data_generator import (ImageDataGeneratorCustom as G, device_path_covers, device_transform_args,
                                                              draw_sample_transforms)
    from ocr4all_pixel_classifier.lib.trainer import AugmentationSettings
    from ocr4all_pixel_classifier.lib.util import image_to_batch
    s = AugmentationSettings(brightness_range=[0.8, 1.2])
    gi, gm = G(**s.to_image_params(), data_format='channels_last'), G(**s.to_mask_params(), data_format='channels_last')
    assert device_path_covers(gi, gm)
    eng = E.Engine("fcn_skip", 3, in_channels=a.channels, mode=E.MODE_F32_EXACT)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42))
    eng.train_init(clipnorm=1.0)
    pages = []
    for i in range(2):
        img, _, mask = synth.synth_page(1000 + i, a.height, a.width, 3)
        pages.append((img if a.channels == 1 else np.stack([img, 255 - img, img[::-1]], -1), mask))

    def host(k):
        img, m = pages[k % 2]
        i_n = next(gi.flow(image_to_batch(img), seed=k + 1, batch_size=1))[0]
        m_n = next(gm.flow(image_to_batch(m), seed=k + 1, batch_size=1))[0, ..., 0]
        if i_n.shape[-1] == 1:
            i_n = i_n[..., 0]
        return eng.train_forward_backward_float(i_n, m_n.astype(np.uint8))

    def device(k):
        img, m = pages[k % 2]
        p, _ = draw_sample_transforms(gi, gm, img.shape[:2] + (1,), m.shape + (1,), k + 1)
        matrix, offset, flips = device_transform_args(p, img.shape[0], img.shape[1])
        return eng.train_forward_backward_augmented(img, m, matrix, offset, flips, gi.fill_mode, gi.cval, gm.fill_mode, gm.cval,
                                                    p['brightness'])

    def plain(k):
        return eng.train_forward_backward(*pages[k % 2])

    def timed(fn):
        for k in range(a.warmup):
            fn(k)
        t = []
        for k in range(a.steps):
            t0 = time.perf_counter()
            fn(a.warmup + k)
            t.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(t)), float(np.min(t)), float(np.max(t))

    assert np.allclose(host(0), device(0), rtol=1e-6, atol=0)          # the same sample either way
    rows = []
    for r in range(3):
        rows.append(("(a) host-array path, run %d" % (r + 1), timed(host)))
        rows.append(("(b) device-resident entry, run %d" % (r + 1), timed(device)))
    rows.append(("(c) un-augmented step", timed(plain)))
    c = rows[-1][1][0]
    lines = ["augmented train step, fcn_skip float32, %dx%d page, %d channel(s), default AugmentationSettings + brightness_range [0.8, 1.2]"
             % (a.height, a.width, a.channels),
             "wall ms per sample (median / min / max of %d after %d warm-up), each ended by the step's metrics read" % (a.steps, a.warmup),
             ""]
    lines += ["%-36s %9.2f %9.2f %9.2f" % ((name,) + t) for name, t in rows]
    lines += ["", "sample build = path - (c), medians:"]
    lines += ["%-36s %9.2f   (train step (c): %.2f)" % (name, t[0] - c, c) for name, t in rows[:-1]]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    eng.close()


if __name__ == "__main__":
    main()
