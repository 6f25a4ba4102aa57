"""Writing the output masks as PNG (lib/output.py:20-41): what the last stage of the Predictor costs.
On synthetic pages of 2048x1536 (3 classes) and 4096x3072 (6 classes) -- labels = synth_page's mask plus 0.2 % label noise --:
  (a) the parent path: engine.masks (the three RGB masks come down) + three PIL.Image.save(format="PNG") into BytesIO, at PIL's
      default compress_level 6 and at compress_level 1;
  (b) engine.masks_png: the band-parallel device encoder, only the three PNG streams come down;
  (d) pseg_masks_png_device_u8 alone with the label map already resident (torch tensors): encode kernels + framing + download,
      as GB/s over the raw bytes of the three masks;
  (c) the whole page, bf16 fcn_skip engine + cc_majority vote: Predictor.write_masks (one pseg_predict_chain_png call) against
      Predictor.predict_single + output_data (which builds the masks and saves them through PIL: output.DEVICE_PNG = False), both into --tmp (a tmpfs directory).
Wall ms per page after warm-up; (a) and (b), and the two sides of (c), alternate three times in one process.  The device legs
(b), (d) and (c) run at every level of --level (0: fixed Huffman codes, 1: a dynamic code per band), the levels alternating inside
each of the three rounds; --band-rows sets the band of (b) and (d) (0: the level's default).  The size table has a row per level
and, for level 1, one per band size of 16 / 64 / 256 KB of filtered bytes, each with leg (d)'s time.  Writes --out."""
import argparse, ctypes, io, os, shutil, sys, time
os.environ.setdefault("PSEG_PLAN_FROM_ENV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "page-segmentation_amd")]
import numpy as np

LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255]], np.uint8)
NAMES = ("color", "overlay", "inverted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="2048x1536x3,4096x3072x6")
    ap.add_argument("--skip-pil", action="store_true", help="device legs only (profiler runs)")
    ap.add_argument("--tmp", default="/dev/shm/pseg_bench_png")
    ap.add_argument("--level", default="0,1", help="levels of the device legs, comma-separated")
    ap.add_argument("--band-rows", type=int, default=0, help="rows per band of legs (b) and (d); 0: the level's default")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_dynamic.txt"))
    a = ap.parse_args()
    levels = [int(v) for v in a.level.split(",")]
    import torch
    torch.cuda.is_available()               # torch's bundled HIP runtime initialises first (as bench.py)
    from PIL import Image
    from pseg_amd import engine as E, synth
    from ocr4all_pixel_classifier.lib import output
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings

    def timed(fn, steps=None):
        for _ in range(a.warmup):
            fn()
        t = []
        for _ in range(steps or a.steps):
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(t)), float(np.min(t)), float(np.max(t))

    lines = []
    for size in a.sizes.split(","):
        H, W, C = (int(v) for v in size.split("x"))
        img, binary, mask = synth.synth_page(0, H, W, C)
        rng = np.random.default_rng(7)
        pred = mask.astype(np.int64)
        noise = rng.random((H, W)) < 0.002
        pred[noise] = rng.integers(0, C, int(noise.sum()))
        lut = LUT[:C]
        raw = H * W * 3
        sizes = {}

        def pil(level=None):
            kw = {} if level is None else {"compress_level": level}
            ms = E.masks(pred, binary, lut)[:3]
            out = []
            for m in ms:
                buf = io.BytesIO()
                Image.fromarray(m).save(buf, format="PNG", **kw)
                out.append(buf.tell())
            sizes["pil%s" % ("" if level is None else level)] = out

        def dev(level):
            got = E.masks_png(pred, binary, lut, band_rows=a.band_rows, level=level)
            sizes["level %d" % level] = [len(got[n]) for n in NAMES]

        # the streams decode to the parent path's arrays
        ref = E.masks(pred, binary, lut)
        for level in levels:
            got = E.masks_png(pred, binary, lut, band_rows=a.band_rows, level=level)
            for n, m in zip(NAMES, ref):
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(got[n]))), m), (n, level)
        # (d) resident inputs
        d_pred = torch.from_numpy(pred.astype(np.uint8)).cuda()
        d_bin = torch.from_numpy(binary).cuda()
        d_lut = torch.from_numpy(np.ascontiguousarray(lut)).cuda()
        cap = max(E.png_bound(H, W, 3, br, lv) for lv in (0, 1) for br in (0, 1, a.band_rows))
        bufs = [E.pinned_empty((cap,), np.uint8) for _ in range(3)]
        P = (ctypes.c_void_p * 4)(bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, None)
        caps = (ctypes.c_size_t * 4)(cap, cap, cap, 0)
        nb = (ctypes.c_size_t * 4)()
        torch.cuda.synchronize()

        def resident(level, band_rows=None):
            E._check(E.lib().pseg_masks_png_device_u8_lv(0, ctypes.c_void_p(d_pred.data_ptr()), ctypes.c_void_p(d_bin.data_ptr()),
                                                         ctypes.c_void_p(d_lut.data_ptr()), C, H, W, a.band_rows if band_rows is None else band_rows,
                                                         level, P, caps, nb, None))

        rows = []
        for r in range(3):
            if not a.skip_pil:
                rows.append(("(a) masks + 3 x PIL save, level 6, run %d" % (r + 1), timed(pil)))
                rows.append(("(a) masks + 3 x PIL save, level 1, run %d" % (r + 1), timed(lambda: pil(1))))
            for lv in levels:
                rows.append(("(b) masks_png, level %d, run %d" % (lv, r + 1), timed(lambda: dev(lv), 4 * a.steps)))
        res = {}
        for r in range(3):
            for lv in levels:
                res[lv] = timed(lambda: resident(lv), 8 * a.steps)
                rows.append(("(d) resident label map -> 3 streams, level %d, run %d" % (lv, r + 1), res[lv]))
        band = {}
        if 1 in levels:                         # level 1 at three band sizes: bytes and leg (d)
            for kb in (16, 64, 256):
                br = max(1, kb * 1024 // (3 * W + 1))
                got = E.masks_png(pred, binary, lut, band_rows=br, level=1)
                for n, m in zip(NAMES, ref):
                    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got[n]))), m), (n, kb)
                band[kb] = (br, [len(got[n]) for n in NAMES], timed(lambda: resident(1, br), 8 * a.steps))
        # (c) the whole page
        cm = ColorMap({str(tuple(int(v) for v in LUT[k])): [k, "c%d" % k] for k in range(C)})
        net = Network("Predict", n_classes=C, exact=False)
        net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
        data = SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page.png")
        shutil.rmtree(a.tmp, ignore_errors=True)
        pr = Predictor(PredictSettings(n_classes=C, color_map=cm, post_process=[find_postprocessor("cc_majority")], output=a.tmp), net)

        def parent_page():
            output.DEVICE_PNG = False
            try:
                p = pr.predict_single(data)
                output.output_data(a.tmp, np.asarray(p.labels), p.data, cm)
            finally:
                output.DEVICE_PNG = True

        for r in range(3):
            if not a.skip_pil:
                rows.append(("(c) predict_single + output_data (PIL), run %d" % (r + 1), timed(parent_page)))
            for lv in levels:
                rows.append(("(c) Predictor.write_masks, level %d, run %d" % (lv, r + 1), timed(lambda: pr.write_masks(data, level=lv), 4 * a.steps)))
        shutil.rmtree(a.tmp, ignore_errors=True)
        net.model.close()
        lines += ["%dx%d page, %d classes: raw RGB %.1f MB per mask, three masks %.1f MB" % (H, W, C, raw / 1e6, 3 * raw / 1e6),
                  "wall ms per page (median / min / max after %d warm-up)" % a.warmup, ""]
        lines += ["%-56s %9.2f %9.2f %9.2f" % ((name,) + t) for name, t in rows]
        lines += ["", "bytes per mask (color / overlay / inverted), band_rows %d:" % a.band_rows]
        lines += ["  %-10s %s" % (k, "  ".join("%9d" % v for v in sizes[k])) for k in ("pil", "pil1", "level 0", "level 1") if k in sizes]
        if band:
            lines += ["level 1 by band size (rows; bytes per mask; (d) median / min / max ms):"]
            lines += ["  %3d KB %4d rows  %s   %9.2f %9.2f %9.2f" % ((kb, band[kb][0], "  ".join("%9d" % v for v in band[kb][1])) + band[kb][2])
                      for kb in sorted(band)]
        lines += ["(d), level %d, over the raw bytes of the three masks: %.1f GB/s (median %.2f ms; includes framing, the size read-back and the download)"
                  % (lv, 3 * raw / res[lv][0] / 1e6, res[lv][0]) for lv in levels]
        lines += [""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
