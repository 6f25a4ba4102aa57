#!/usr/bin/env python
"""A book through the Predictor to mask PNG files: page by page (leg A, a loop of Predictor.write_masks) against the page list
(leg B, Predictor.write_masks_dataset -> pseg_predict_chain_pages_png).

  python tools/bench_chain_pages.py                     both legs, alternated; report to profiles/chain_pages.txt
  python tools/bench_chain_pages.py --leg A             leg A alone (uses only API that older checkouts have: the baseline run)
  python tools/bench_chain_pages.py --kernel-run        the list entry at unit sizes 1, 2, 4, 8 and both levels, nothing timed: run it
                                                        under `rocprofv3 --kernel-trace` (a run of its own, the profiler slows the host)
  python tools/bench_chain_pages.py --kernel-table CSV  the band-kernel table from that run's *_kernel_trace.csv: launches grouped by
                                                        the pages they encode (grid z), time per page against single-page launches

Workload: 32 synthetic 2048x1536 pages (pseg_amd.synth), fcn_skip with 3 classes, bf16 engine, the vote as post-processor, files into
tmpfs, encoder levels 0 and 1.  Times are host wall clock around calls that end synchronised with the files written."""
import argparse
import csv
import glob
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402


def make_predictor_and_pages(n_pages, H, W):
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
    for k in range(n_pages):
        img, binary, _ = synth.synth_page(k, H, W, 3)
        data.append(SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page%03d.png" % k))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=False)
    return Predictor(settings, net), Dataset(data, cm)


def leg_a(pred, ds, out_dir, level):
    t0 = time.perf_counter()
    for d in ds.data:
        pred.write_masks(d, out_dir, level=level)
    return (time.perf_counter() - t0) * 1e3 / len(ds.data)


def leg_b(pred, ds, out_dir, level):
    t0 = time.perf_counter()
    n = sum(1 for _ in pred.write_masks_dataset(ds, out_dir, level=level))
    assert n == len(ds.data)
    return (time.perf_counter() - t0) * 1e3 / len(ds.data)


def same_files(a, b):
    names = sorted(os.path.relpath(p, a) for p in glob.glob(os.path.join(a, "*", "*.png")))
    assert names and names == sorted(os.path.relpath(p, b) for p in glob.glob(os.path.join(b, "*", "*.png")))
    return all(open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read() for n in names)


def run_legs(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    pred, ds = make_predictor_and_pages(args.pages, args.height, args.width)
    legs = {"A": leg_a, "B": leg_b}
    which = ["A", "B"] if args.leg == "both" else [args.leg]
    base = tempfile.mkdtemp(prefix="chain_pages_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    lines = ["# %d pages of %dx%d, fcn_skip 3 classes, bf16, cc_majority, files into %s; ms per page, host wall clock"
             % (args.pages, args.height, args.width, os.path.dirname(base) or "tmp"),
             "# leg A: loop of Predictor.write_masks; leg B: Predictor.write_masks_dataset; %d alternations" % args.alternations]
    try:
        for level in args.levels:
            dirs = {k: os.path.join(base, "l%d_%s" % (level, k)) for k in which}
            for k in which:                                        # warm-up: code objects, workspaces, the canvas, page-locked pools
                legs[k](pred, ds, dirs[k], level)
            if len(which) == 2:
                assert same_files(dirs["A"], dirs["B"]), "leg B's files differ from leg A's"
            times = {k: [] for k in which}
            for _ in range(args.alternations):
                for k in which:
                    times[k].append(legs[k](pred, ds, dirs[k], level))
            for k in which:
                t = times[k]
                lines.append("level %d leg %s: median %.3f ms/page, range %.3f .. %.3f, runs %s"
                             % (level, k, statistics.median(t), min(t), max(t), " ".join("%.3f" % v for v in t)))
            if len(which) == 2:
                lines.append("level %d: B / A = %.3f (medians); B below A in %d of %d alternations; files byte-equal"
                             % (level, statistics.median(times["B"]) / statistics.median(times["A"]),
                                sum(b < a for a, b in zip(times["A"], times["B"])), args.alternations))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def kernel_run(args):
    """The list entry on `pages` resident-shape pages at unit sizes 1, 2, 4, 8, both levels; the second round is the one to read (the
    trace holds both: the table takes every launch, the first round's included -- the band kernel has no warm-up state)."""
    import pseg_amd
    from pseg_amd import synth
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    eng = pseg_amd.Engine("fcn_skip", 3, mode=pseg_amd.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    pages = [synth.synth_page(k, args.height, args.width, 3) for k in range(args.pages)]
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    for _ in range(2):
        for level in args.levels:
            for cap in (1, 2, 4, 8):
                eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=lut,
                                        png_level=level, unit_cap=cap, sink=lambda page, name, data: None)
    eng.close()


def kernel_table(args):
    rows = {}
    for path in args.kernel_table:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if "png_band_kernel" not in name:
                    continue
                m = re.search(r"png_band_kernel<[^,>]+,\s*(\d)\s*[,>]", name)
                if not m:
                    continue
                level = int(m.group(1))
                z = int(r["Grid_Size_Z"]) // max(1, int(r.get("Workgroup_Size_Z", 1) or 1))
                rows.setdefault((level, z), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["# png_band_kernel launches by the pages they encode (grid z), from a kernel trace of --kernel-run; us",
             "# level pages launches  median/launch  median/page  vs single launches"]
    for level in sorted({k[0] for k in rows}):
        single = statistics.median(rows[(level, 1)]) if (level, 1) in rows else float("nan")
        for z in sorted(k[1] for k in rows if k[0] == level):
            t = statistics.median(rows[(level, z)])
            lines.append("  %d     %2d    %5d     %10.1f   %10.1f   %.3f" % (level, z, len(rows[(level, z)]), t, t / z, t / z / single))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=32)
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--leg", choices=["both", "A", "B"], default="both")
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-table", nargs="+", metavar="CSV")
    ap.add_argument("--out", default=None, help="report file (default for the two-leg run: profiles/chain_pages.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.kernel_table:
        return kernel_table(args)
    if args.kernel_run:
        return kernel_run(args)
    if args.out is None and args.leg == "both":
        args.out = os.path.join(ROOT, "profiles", "chain_pages.txt")
    return run_legs(args)


if __name__ == "__main__":
    main()
