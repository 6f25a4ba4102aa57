"""Which device operations the list entries issue: every list entry once on a 70-item list of tiny mixed shapes (two groups each), the
mask encoder at both levels, the vote on both of its paths and a chain call with a bounding-box post-op.  Run it under a trace, once per
library, and compare the two summaries; PSEG_LIB selects the library:
    PSEG_LIB=<libpseg.so> rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d <dir> -- python tools/list_trace.py
    python tools/list_trace.py --summary <dir>          # kernel names with launch counts, copies by direction"""
import csv, glob, os, struct, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(d):
    calls, copies = {}, {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            calls[row["Kernel_Name"]] = calls.get(row["Kernel_Name"], 0) + 1
    for fn in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            copies[row["Direction"]] = copies.get(row["Direction"], 0) + 1
    print("kernels: %d launches of %d names" % (sum(calls.values()), len(calls)))
    for name in sorted(calls):
        print("%7d  %s" % (calls[name], name))
    print("copies: " + ", ".join("%s %d" % (k, copies[k]) for k in sorted(copies)))


def png_gray(a):
    """An 8-bit gray PNG of `a`, filter 0 on every row."""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))
    H, W = a.shape
    raw = b"".join(b"\0" + a[y].tobytes() for y in range(H))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "page-segmentation_amd")]
    import numpy as np
    from pseg_amd import engine as E, synth
    rng = np.random.default_rng(7)
    n = 70
    shapes = [(int(rng.integers(8, 41)), int(rng.integers(8, 71))) for _ in range(n)]
    gray = [rng.integers(0, 256, s).astype(np.uint8) for s in shapes]
    ink = [(g < 110).astype(np.uint8) for g in gray]
    lab = [rng.integers(0, 3, s).astype(np.uint8) for s in shapes]

    h, t = E.char_heights(gray)
    print("char_heights: %d heights, thresholds sum %d" % (len(h), sum(t)), flush=True)
    dec = E.png_decode_gray([png_gray(g) for g in gray])
    print("png_decode_gray: %d of %d equal" % (sum(int(st == 0 and np.array_equal(a, g)) for (a, st), g in zip(dec, gray)), n), flush=True)
    ev = E.eval_pages(lab, [rng.integers(0, 3, s).astype(np.uint8) for s in shapes], ink, n_classes=3, connectivity=8,
                      rules=(E.eval_rule(0, 1, 0.5, 0.5, 0.5),))
    print("eval_pages: counts sum %d, components %d" % (int(ev["counts"].sum()), int(ev["components"].sum())), flush=True)
    bz = E.binarize_scans(gray, [E.Sauvola(5 + 2 * (i % 3)) if i % 4 else None for i in range(n)], thresholds=True)
    print("binarize_scans: ink %d" % sum(int(b.sum()) for b, _ in bz), flush=True)
    ds, cnt = E.despeckle_maps(ink, [E.Despeckle(3 + i % 5, 8 if i % 2 else 4) if i % 7 else None for i in range(n)], counts=True)
    print("despeckle_maps: ink %d, counts %s" % (sum(int(m.sum()) for m in ds), cnt.sum(0).tolist()), flush=True)
    colors = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    src = [colors[rng.integers(0, 3, (s[0] + 3, s[1] + 5))] if i % 2 else rng.integers(0, 3, (s[0] + 3, s[1] + 5)).astype(np.uint8)
           for i, s in enumerate(shapes)]
    lm = E.label_masks(src, shapes, colors, np.array([0, 1, 2], np.uint8), counts=True)
    print("label_masks: %d maps, counts sum %d" % (len(lm), sum(int(c.sum()) for _, c in lm)), flush=True)
    tr = E.text_regions(lab, E.TextRegions(1, kernels=(3, 2, 5)))
    print("text_regions: %d regions" % sum(len(r["boxes"]) for r in tr), flush=True)

    H, W = 33, 65
    pred = rng.integers(0, 3, (H, W)).astype(np.int64)
    binary = (rng.random((H, W)) < 0.45).astype(np.uint8)
    lut = rng.integers(0, 256, (3, 3)).astype(np.uint8)
    for level in (0, 1):
        out = E.masks_png(pred, binary, lut, level=level)
        print("masks_png level %d: %s" % (level, sorted((k, len(v)) for k, v in out.items())), flush=True)
    for C in (3, 13):
        p = rng.integers(0, C, (H, W)).astype(np.int64)
        print("cc_vote %d classes: %s" % (C, np.bincount(E.cc_vote(p, binary, C).ravel(), minlength=C).tolist()), flush=True)
    img, b, _ = synth.synth_page(0, 96, 80)
    eng = E.Engine("fcn_skip", 3, mode=E.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    r = eng.predict_chain(img, b, post_ops=("cc_vote", "bbox"))
    print("predict_chain with bbox: %s" % np.bincount(np.asarray(r["labels"]).ravel(), minlength=3).tolist(), flush=True)
    eng.close()
    assert E.lib().pseg_release_workspace(0) == 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        run()
