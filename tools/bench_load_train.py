#!/usr/bin/env python
"""Loading a training set, measured: DatasetLoader.load_data against DatasetLoader.load_data_list end to end (a), one
pseg_amd.label_masks call on decoded arrays against ColorMap.to_labels + preserving_resize in a loop (b), the kernel against the
copies (c), and the list route with 2 and 16 decode threads (d).

  python tools/bench_load_train.py                       (a), (b), (d); report to profiles/load_train.txt
  python tools/bench_load_train.py --child LEG DIR       one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_load_train.py --kernel-run          8 masks, 3 list calls, nothing timed: run it under
                                                         `rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv`
                                                         (a run of its own)
  python tools/bench_load_train.py --kernel-count DIR    (c): kernel and copy times per mask from that run's *_stats.csv files

Workload: tools/bench_chain_scans.py's 64 synthetic scans of 1700x1200 with its line heights, and per scan an RGB mask of the same
size in the colours of a five-entry colour map, as PNG files in tmpfs.  Three alternations, each leg a process of its own that warms
up before it measures.  Times are host wall clock, ms per entry."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import bench_chain_scans as S  # noqa: E402

COLORS = {"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"], "(0, 0, 255)": [3, "marginalia"], "(0, 0, 0)": [4, "rule"]}


def color_map():
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    return ColorMap(COLORS)


def synth_mask(k):
    """The RGB mask of scan k: its regions in the map's colours (the text regions of odd rows of blocks as marginalia, so that all
    five colours occur)."""
    from pseg_amd import synth
    ids = synth.synth_page(k, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], 3)[2].astype(np.uint8)
    ids[(ids == 1) & ((np.arange(ids.shape[0])[:, None] // 200) % 2 == 1)] = 3
    ids[::340, :] = 4
    return color_map().lut()[ids]


def write_masks(directory, n):
    from PIL import Image
    for k in range(n):
        Image.fromarray(synth_mask(k)).save(os.path.join(directory, "mask%03d.png" % k))


def child(leg, directory, n):
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    from ocr4all_pixel_classifier.lib.util import preserving_resize
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    scans = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:n]
    masks = sorted(glob.glob(os.path.join(directory, "mask*.png")))[:n]
    lh = S.line_heights(len(scans))
    cm = color_map()
    loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm)
    entries = lambda: [SingleData(image_path=s, mask_path=m, line_height_px=h) for s, m, h in zip(scans, masks, lh)]
    if leg == "load_data":
        run = lambda: loader.load_data(entries())
    elif leg.startswith("load_data_list"):
        threads = int(leg.split(":")[1]) if ":" in leg else 2
        run = lambda: loader.load_data_list(entries(), decode_threads=threads)
    else:
        from PIL import Image
        rgb = [np.asarray(Image.open(m).convert("RGB")) for m in masks]
        shapes = [pseg_amd.engine.rescale_shape(S.SCAN_SHAPE, S.TARGET_LINE_HEIGHT / h) for h in lh]
        colors, ids = cm.table()
        if leg == "labels-loop":
            run = lambda: [preserving_resize(cm.to_labels(a), s).astype(np.uint8) for a, s in zip(rgb, shapes)]
        else:
            run = lambda: pseg_amd.label_masks(rgb, shapes, colors, ids, counts=(leg == "labels-list-counts"))
    run()
    t0 = time.perf_counter()
    run()
    print(json.dumps({"leg": leg, "ms": (time.perf_counter() - t0) * 1e3 / len(scans), "entries": len(scans)}), flush=True)


def _rows(cmd):
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _line(tag, vals):
    return "%s: median %.3f, runs %s" % (tag, statistics.median(vals), " ".join("%.3f" % v for v in vals))


def drive(args):
    base = tempfile.mkdtemp(prefix="load_train_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    me = os.path.abspath(__file__)
    lines = ["# tools/bench_load_train.py: %d scans of %dx%d (pseg_amd.synth) and RGB masks of %d colours, PNG files in tmpfs, ms per entry, host wall "
             "clock, %d alternations, one process per leg" % (args.scans, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], len(COLORS), args.alternations)]
    try:
        S.write_scans(base, args.scans)
        write_masks(base, args.scans)

        def legs(title, names):
            t = {leg: [] for leg in names}
            for alt in range(args.alternations):
                for leg in names:
                    print("%s alternation %d, %s" % (title[:3], alt, leg), file=sys.stderr, flush=True)
                    t[leg] += [r["ms"] for r in _rows([sys.executable, me, "--child", leg, base, "--scans", str(args.scans)])]
            lines.append(title)
            for leg in names:
                lines.append(_line("%-20s" % leg, t[leg]))
            return t
        t = legs("## (a) files to records: DatasetLoader.load_data against load_data_list (chunk 64, 2 decode threads)", ("load_data", "load_data_list"))
        a, b = t["load_data"], t["load_data_list"]
        spread = max(a) - min(a)
        below = all(x - y > spread for x, y in zip(a, b))
        lines.append("load_data_list / load_data = %.3f (medians); spread of load_data's own repeats %.3f ms; load_data - load_data_list per "
                     "alternation %s ms: %s" % (statistics.median(b) / statistics.median(a), spread, " ".join("%+.3f" % (x - y) for x, y in zip(a, b)),
                                                "below load_data by more than that spread in every alternation" if below else
                                                "**NOT below load_data by more than that spread in every alternation**"))
        t = legs("## (b) decoded arrays to label maps: to_labels + preserving_resize in a loop (labels-loop) against one label_masks call",
                 ("labels-loop", "labels-list", "labels-list-counts"))
        lines.append("labels-list / labels-loop = %.4f, with counts %.4f (medians)"
                     % (statistics.median(t["labels-list"]) / statistics.median(t["labels-loop"]),
                        statistics.median(t["labels-list-counts"]) / statistics.median(t["labels-loop"])))
        legs("## (d) load_data_list with 2 and 16 decode threads", ("load_data_list:2", "load_data_list:16"))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run():
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    rgb = [synth_mask(k) for k in range(8)]
    shapes = [pseg_amd.engine.rescale_shape(S.SCAN_SHAPE, S.TARGET_LINE_HEIGHT / h) for h in S.line_heights(8)]
    colors, ids = color_map().table()
    for _ in range(3):
        pseg_amd.label_masks(rgb, shapes, colors, ids, counts=True)
    print("kernel-run: 8 masks x 3 calls")


def kernel_count(args):
    lines = ["## (c) rocprofv3 --kernel-trace --memory-copy-trace --stats over `--kernel-run` (8 masks of %dx%d per call, 3 calls): per mask"
             % S.SCAN_SHAPE]
    for path in sorted(glob.glob(os.path.join(args.kernel_count, "**", "*_stats.csv"), recursive=True)):
        if not (path.endswith("kernel_stats.csv") or path.endswith("memory_copy_stats.csv")):
            continue
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "lm_list_kernel" in r["Name"] or "MEMORY_COPY" in r["Name"].upper():
                    lines.append("  %-44s calls %4d  total %10.1f us  %8.1f us per mask"
                                 % (r["Name"].split("(")[0].split("::")[-1][:44], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3,
                                    float(r["TotalDurationNs"]) / 1e3 / 24.0))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", nargs=2, metavar=("LEG", "DIR"))
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/load_train.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.scans)
    if args.kernel_run:
        return kernel_run()
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "load_train.txt")
    return drive(args)


if __name__ == "__main__":
    main()
