#!/usr/bin/env python
"""The adaptive binarisation, measured: one pseg_amd.binarize_scans call against the NumPy restatement and the host entry (a), the
default route of Predictor.write_masks_scans on this tree against a checkout of the parent commit (b), and write_masks_scans with
binarize=Sauvola() against binarize=None (c).

  python tools/bench_binarize.py [--parent DIR]         all runs, report to profiles/binarize.txt ((b) needs a built parent checkout)
  python tools/bench_binarize.py --child LEG [DIR]      one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_binarize.py --kernel-run WINDOW    8 scans, 3 list calls at that window, nothing timed: run it under
                                                        `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_binarize.py --kernel-count DIR --window WINDOW     per-kernel times and bytes from that run's *kernel_stats.csv

Workload: tools/bench_chain_scans.py's 64 synthetic scans of 1700x1200 with its line heights (the default windows follow from
them), fcn_skip with 3 classes, bf16 engine, the vote, files into tmpfs.  Three alternations, each leg a process of its own that
warms up before it measures.  Times are host wall clock, ms per scan."""
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
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import bench_chain_scans as S  # noqa: E402

WINDOWS = (15, 37, 255)
NUMPY_SCANS = 4                  # the restatement is timed on a few scans only
HBM_BYTES_PER_S = 8.0e12         # MI355X peak


def synth_scans(n):
    from pseg_amd import synth
    return [(255 - synth.synth_page(k, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], 3)[0]).astype(np.uint8) for k in range(n)]


def child_calls(leg, n):
    import pseg_amd
    scans = synth_scans(n)
    for w in WINDOWS:
        how = pseg_amd.Sauvola(w)
        if leg == "numpy":
            import binarize_cases as C
            run, m = (lambda: [C.sauvola(g, w)[0] for g in scans[:NUMPY_SCANS]]), NUMPY_SCANS
        else:
            run, m = (lambda: pseg_amd.binarize_scans(scans, how, host=(leg == "host"))), n
        run()
        t0 = time.perf_counter()
        run()
        print(json.dumps({"leg": leg, "window": w, "ms": (time.perf_counter() - t0) * 1e3 / m, "scans": m}), flush=True)


def child_masks(leg, directory, n):
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:n]
    lh = S.line_heights(len(paths))
    how = pseg_amd.Sauvola() if leg == "masks-sauvola" else None
    for high_res in (False, True):
        pred, cm = S.make_predictor(high_res)
        loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm, prediction=True)
        entries = [SingleData(image_path=p, line_height_px=h) for p, h in zip(paths, lh)]
        out_dir = os.path.join(directory, "out_%s_%d" % (leg, high_res))
        run = lambda: sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=0, binarize=how))
        run()
        t0 = time.perf_counter()
        run()
        print(json.dumps({"leg": leg, "high_res": int(high_res), "ms": (time.perf_counter() - t0) * 1e3 / len(paths), "scans": len(paths),
                          "windows": sorted({pseg_amd.sauvola_window(h) for h in lh})}), flush=True)
        pred.network.model.close()
        shutil.rmtree(out_dir, ignore_errors=True)


def _rows(cmd, cwd=None):
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900, cwd=cwd).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _line(tag, vals):
    return "%s: median %.3f, runs %s" % (tag, statistics.median(vals), " ".join("%.3f" % v for v in vals))


def drive(args):
    base = tempfile.mkdtemp(prefix="binarize_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    me = os.path.abspath(__file__)
    n = ["--scans", str(args.scans)]
    lines = ["# tools/bench_binarize.py: %d scans of %dx%d (pseg_amd.synth), ms per scan, host wall clock, %d alternations, one process per leg"
             % (args.scans, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], args.alternations)]
    try:
        S.write_scans(base, args.scans)
        # (a)
        rows = []
        for alt in range(args.alternations):
            for leg in ("numpy", "host", "list"):
                print("(a) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg] + n)
        lines.append("## (a) one binarize_scans call over the list (list) against binarize_scans(host=True) (host) and the NumPy restatement "
                     "(numpy, %d scans)" % NUMPY_SCANS)
        for w in WINDOWS:
            t = {leg: [r["ms"] for r in rows if r["leg"] == leg and r["window"] == w] for leg in ("numpy", "host", "list")}
            for leg in ("numpy", "host", "list"):
                lines.append(_line("window %3d %-5s" % (w, leg), t[leg]))
            lines.append("window %3d: list / numpy = %.4f, list / host = %.4f (medians)"
                         % (w, statistics.median(t["list"]) / statistics.median(t["numpy"]), statistics.median(t["list"]) / statistics.median(t["host"])))
        # (b)
        if args.parent:
            rows = {"parent": [], "this": []}
            for alt in range(args.alternations):
                for leg, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                    print("(b) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                    rows[leg] += _rows([sys.executable, os.path.join(tree, "tools", "bench_chain_scans.py"), "--child", "b", "files", base,
                                        "--levels", "0"] + n, cwd=tree)
            lines.append("## (b) write_masks_scans, binarize=None (tools/bench_chain_scans.py --child b files, level 0): the parent commit against this tree")
            for hr in (0, 1):
                tp, tt = ([r["ms"] for r in rows[leg] if r["high_res"] == hr] for leg in ("parent", "this"))
                lines.append(_line("high_res %d parent" % hr, tp))
                lines.append(_line("high_res %d this  " % hr, tt))
                lines.append("high_res %d: this / parent = %.3f (medians); spread of the parent's repeats %.3f ms, this - parent = %+.3f ms"
                             % (hr, statistics.median(tt) / statistics.median(tp), max(tp) - min(tp), statistics.median(tt) - statistics.median(tp)))
        # (c)
        rows = []
        for alt in range(args.alternations):
            for leg in ("masks-none", "masks-sauvola"):
                print("(c) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg, base] + n)
        lines.append("## (c) write_masks_scans(binarize=Sauvola()) against binarize=None, level 0; windows %s"
                     % sorted({w for r in rows for w in r["windows"]}))
        for hr in (0, 1):
            t0, t1 = ([r["ms"] for r in rows if r["leg"] == leg and r["high_res"] == hr] for leg in ("masks-none", "masks-sauvola"))
            lines.append(_line("high_res %d none   " % hr, t0))
            lines.append(_line("high_res %d sauvola" % hr, t1))
            lines.append("high_res %d: the binarisation adds %.3f ms per scan (medians)" % (hr, statistics.median(t1) - statistics.median(t0)))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    scans = synth_scans(8)
    for _ in range(3):
        pseg_amd.binarize_scans(scans, pseg_amd.Sauvola(args.kernel_run))
    print("kernel-run window %d: 8 scans x 3 calls" % args.kernel_run)


def kernel_count(args):
    from pseg_amd import engine as E
    seg, band, tile, _ = E.binarize_geometry()
    H, W = S.SCAN_SHAPE
    w = args.window
    segs = -(-W // (seg - (w - 1)))
    bands = -(-H // band)
    # bytes by count, per scan: the row kernel reads every row once per segment with its halo and writes 8 bytes per pixel; the
    # column kernel reads w words per band and column, then two per further row, the scan byte, and writes the ink byte
    moved = {"bz_rows": H * (W + segs * (w - 1)) + 8 * H * W,
             "bz_cols": 8 * W * (bands * w + 2 * (H - bands)) + 2 * H * W}
    lines = ["## per-kernel times at window %d, rocprofv3 --kernel-trace --stats over `--kernel-run %d` (8 scans per launch, 3 launches)" % (w, w)]
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for key, nbytes in moved.items():
                    if key in r["Name"]:
                        us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]) / 8.0
                        lines.append("  %-22s calls %d  %8.1f us per scan  %6.1f MB per scan by count  %.2f TB/s = %.0f %% of the HBM peak (%.0f TB/s)"
                                     % (r["Name"].split("(")[0].split("::")[-1][:22], int(r["Calls"]), us, nbytes / 1e6, nbytes / us / 1e6,
                                        100.0 * nbytes / (us * 1e-6) / HBM_BYTES_PER_S, HBM_BYTES_PER_S / 1e12))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for (b)")
    ap.add_argument("--child", nargs="+", metavar=("LEG", "DIR"))
    ap.add_argument("--kernel-run", type=int, metavar="WINDOW")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--window", type=int, default=15)
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/binarize.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        if args.child[0] in ("numpy", "host", "list"):
            return child_calls(args.child[0], args.scans)
        return child_masks(args.child[0], args.child[1], args.scans)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "binarize.txt")
    return drive(args)


if __name__ == "__main__":
    main()
