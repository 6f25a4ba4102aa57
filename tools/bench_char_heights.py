#!/usr/bin/env python
"""Line heights of a list of scans: the single-image entry in a loop against the list entry, and the two-pass book workflow against
write_masks_scans that measures the missing line heights itself.

  python tools/bench_char_heights.py                      all runs, report to profiles/char_heights.txt
  python tools/bench_char_heights.py --child LEG DIR      one process of one leg (what the driver starts; prints one JSON line)
  python tools/bench_char_heights.py --kernel-run         8 scans through char_heights, 3 rounds, nothing timed: run it under
                                                          `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_char_heights.py --kernel-times DIR   per-kernel times of the three launches from that run's *kernel_stats.csv or *_results.db

Workload: the 64 synthetic scans of 1700x1200 tools/bench_chain_scans.py makes (pseg_amd.synth, ink dark), as PNG files in tmpfs.
  (a) arrays: `loop` = otsu_char_height per scan, `list` = one char_heights call; ms per scan, the scans decoded beforehand.
  (b) files to mask files, fcn_skip 3 classes, bf16, the vote, encoder level 0: `two` = compute_char_height per file, then
      write_masks_scans with the heights filled in (today's workflow: every scan decoded twice); `one` = write_masks_scans with
      line_height_px=None.
Three alternations of each pair, each run a process of its own that warms up before it measures.  Host wall clock."""
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

import bench_chain_scans as scans_bench  # noqa: E402

KERNELS = ("ch_hist_kernel", "ch_otsu_kernel", "ch_window_kernel")


def child(args):
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData, _imread_gray
    from ocr4all_pixel_classifier.lib.image_ops import compute_char_height
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    leg, directory = args.child
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:args.scans]
    n = len(paths)
    if leg in ("loop", "list"):
        scans = [np.ascontiguousarray(_imread_gray(p), dtype=np.uint8) for p in paths]
        if leg == "loop":
            run = lambda: [pseg_amd.otsu_char_height(s)[0] for s in scans]
        else:
            run = lambda: pseg_amd.char_heights(scans)[0]
    else:
        pred, cm = scans_bench.make_predictor(False)
        loader = DatasetLoader(scans_bench.TARGET_LINE_HEIGHT, cm, prediction=True)
        out_dir = os.path.join(directory, "out_" + leg)

        def run():
            if leg == "two":
                entries = [SingleData(image_path=p, line_height_px=compute_char_height(p, False)) for p in paths]
            else:
                entries = [SingleData(image_path=p, line_height_px=None) for p in paths]
            assert sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=0)) == n
            return [e.line_height_px for e in entries]
    run()                                                                  # warm-up: code objects, workspaces, canvases, page cache
    t0 = time.perf_counter()
    heights = run()
    ms = (time.perf_counter() - t0) * 1e3 / n
    print(json.dumps({"leg": leg, "ms": ms, "scans": n, "heights": heights}), flush=True)
    if leg in ("two", "one"):
        pred.network.model.close()
        shutil.rmtree(out_dir, ignore_errors=True)


def drive(args):
    base = tempfile.mkdtemp(prefix="char_heights_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rows = []
    try:
        scans_bench.write_scans(base, args.scans)
        for pair in (("loop", "list"), ("two", "one")):
            for alt in range(args.alternations):
                for leg in pair:
                    print("alternation %d, leg %s" % (alt, leg), file=sys.stderr, flush=True)
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, base, "--scans", str(args.scans)],
                                         check=True, capture_output=True, text=True, timeout=600).stdout
                    rows += [dict(json.loads(ln), alternation=alt) for ln in out.splitlines() if ln.startswith("{")]
    finally:
        shutil.rmtree(base, ignore_errors=True)
    assert all(r["heights"] == rows[0]["heights"] for r in rows), "the legs disagree on the line heights"
    lines = ["# tools/bench_char_heights.py: %d scans of %dx%d (pseg_amd.synth), ms per scan, host wall clock, %d alternations, one process per run"
             % (args.scans, scans_bench.SCAN_SHAPE[0], scans_bench.SCAN_SHAPE[1], args.alternations),
             "# every leg measured the same line heights: median %s, range %s .. %s" % (
                 statistics.median(rows[0]["heights"]), min(rows[0]["heights"]), max(rows[0]["heights"]))]
    for (old, new), title in ((("loop", "list"), "(a) decoded arrays: otsu_char_height in a loop (loop) against one char_heights call (list)"),
                              (("two", "one"), "(b) PNG files to mask files: compute_char_height per file + write_masks_scans (two) against "
                                               "write_masks_scans with line_height_px=None (one)")):
        lines.append("## " + title)
        ta, tb = [r["ms"] for r in rows if r["leg"] == old], [r["ms"] for r in rows if r["leg"] == new]
        spread = max(max(ta) - min(ta), max(tb) - min(tb))
        wins = sum(x - y > spread for x, y in zip(ta, tb))
        lines.append("%s: median %.3f, runs %s" % (old, statistics.median(ta), " ".join("%.3f" % v for v in ta)))
        lines.append("%s: median %.3f, runs %s" % (new, statistics.median(tb), " ".join("%.3f" % v for v in tb)))
        lines.append("%s / %s = %.3f (medians); spread %.3f ms; %s below %s by more than the spread in %d of %d alternations"
                     % (new, old, statistics.median(tb) / statistics.median(ta), spread, new, old, wins, len(ta)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    from pseg_amd import synth
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    scans = [(255 - synth.synth_page(k, scans_bench.SCAN_SHAPE[0], scans_bench.SCAN_SHAPE[1], 3)[0]).astype(np.uint8) for k in range(8)]
    for _ in range(3):
        heights = pseg_amd.char_heights(scans)[0]
    print("kernel-run: 8 scans x 3 rounds, heights %r" % (heights,))


def kernel_times(args):
    lines = ["## per-kernel times, rocprofv3 --kernel-trace --stats over `--kernel-run` (8 scans of %dx%d per launch, 3 launches each)"
             % scans_bench.SCAN_SHAPE]
    stats = []                                                             # (kernel name, calls, total ns): the CSV, or the run's database
    for path in glob.glob(os.path.join(args.kernel_times, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            stats += [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    for path in glob.glob(os.path.join(args.kernel_times, "**", "*_results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(path) as db:
            stats += list(db.execute("select name, count(*), sum(duration) from kernels group by name"))
    for name, calls, ns in stats:
        if any(k in name for k in KERNELS):
            lines.append("  %-20s calls %d  %9.1f us per launch  %8.1f us per scan" % (
                [k for k in KERNELS if k in name][0], calls, ns / 1e3 / calls, ns / 1e3 / calls / 8))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", nargs=2, metavar=("LEG", "DIR"))
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-times", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "char_heights.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_times:
        return kernel_times(args)
    return drive(args)


if __name__ == "__main__":
    main()
