#!/usr/bin/env python
"""Scoring a list of pages against ground truth: today's per-page route against one evaluate_pages call.

  python tools/bench_eval_pages.py                      all runs, report to profiles/eval_pages.txt
  python tools/bench_eval_pages.py --child LEG          one process of one leg (what the driver starts; prints one JSON line)
  python tools/bench_eval_pages.py --kernel-run         8 pages through eval_pages, 3 rounds, nothing timed: run it under
                                                        `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_eval_pages.py --kernel-times DIR   per-kernel times from that run's *kernel_stats.csv or *_results.db

Workload: 64 synthetic pages of 2048x1536 (pseg_amd.synth), 3 classes, 7 % of the labels flipped, uint8 maps, connectivity 4.
  `page` = per page: count_matches for every label, total_accuracy, image_ops.fgpa, and
           ConnectedComponentEval(...).run_per_component(cc_matching(1, .5, .1)) summed;
  `list` = one evaluate_pages call with the same rule; the same numbers are read from its PageScores.
Three alternations, each run a process of its own that warms up (on 4 pages) before it measures.  Host wall clock, ms per page."""
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
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

SHAPE, CLASSES = (2048, 1536), 3
KERNELS = ("ep_hist_kernel", "ep_tile_kernel", "ep_border_kernel", "ep_merge_kernel", "ep_judge_kernel")
HBM_GBS = 8000.0                                                           # MI355X: 8 TB/s peak


def make_pages(n, directory=None):
    """(binary, mask, pred) of n pages; with a directory, kept there as one .npz per page (the driver makes them once for all runs)."""
    from pseg_amd import synth
    pages = []
    for k in range(n):
        path = os.path.join(directory, "page%03d.npz" % k) if directory else None
        if path and os.path.exists(path):
            with np.load(path) as z:
                pages.append((z["binary"], z["mask"], z["pred"]))
            continue
        _, binary, mask = synth.synth_page(k, SHAPE[0], SHAPE[1], CLASSES)
        rng = np.random.default_rng(k)
        pred = mask.astype(np.uint8)
        flip = rng.random(mask.shape) < 0.07
        pred[flip] = rng.integers(0, CLASSES, int(flip.sum()))
        pages.append((np.ascontiguousarray(binary, dtype=np.uint8), np.ascontiguousarray(mask, dtype=np.uint8), pred))
        if path:
            np.savez(path, binary=pages[-1][0], mask=pages[-1][1], pred=pred)
    return pages


def score_pages(pages):
    from ocr4all_pixel_classifier.lib import evaluation as E
    from ocr4all_pixel_classifier.lib import image_ops as I
    out = []
    for binary, mask, pred in pages:
        row = [E.count_matches(mask, pred, label) for label in range(CLASSES)]
        row.append(E.total_accuracy(mask, pred))
        row.append(I.fgpa(pred, mask, binary))
        res = list(E.ConnectedComponentEval(mask, pred, binary).run_per_component(E.cc_matching(1, .5, .1)))
        row.append([int(v) for v in np.sum(res, axis=0)] + [len(res)])
        out.append(row)
    return out


def score_list(pages):
    from ocr4all_pixel_classifier.lib import evaluation as E
    scores = E.evaluate_pages([m for _, m, _ in pages], [p for _, _, p in pages], [b for b, _, _ in pages], [E.cc_matching(1, .5, .1)])
    return [[s.count_matches(label) for label in range(CLASSES)] + [s.total_accuracy(), s.fgpa(), list(s.cc(0))] for s in scores]


def child(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    pages = make_pages(args.pages, args.dir)
    run = score_pages if args.child == "page" else score_list
    run(pages[:4])                                                         # warm-up: code objects, workspaces
    t0 = time.perf_counter()
    rows = run(pages)
    ms = (time.perf_counter() - t0) * 1e3 / len(pages)
    print(json.dumps({"leg": args.child, "ms": ms, "pages": len(pages), "rows": json.loads(json.dumps(rows))}), flush=True)


def drive(args):
    rows = []
    base = tempfile.mkdtemp(prefix="eval_pages_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        make_pages(args.pages, base)
        for alt in range(args.alternations):
            for leg in ("page", "list"):
                print("alternation %d, leg %s" % (alt, leg), file=sys.stderr, flush=True)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--pages", str(args.pages), "--dir", base],
                                     check=True, capture_output=True, text=True, timeout=900).stdout
                rows += [dict(json.loads(ln), alternation=alt) for ln in out.splitlines() if ln.startswith("{")]
    finally:
        shutil.rmtree(base, ignore_errors=True)
    assert all(r["rows"] == rows[0]["rows"] for r in rows), "the legs disagree on the scores"
    ta, tb = [r["ms"] for r in rows if r["leg"] == "page"], [r["ms"] for r in rows if r["leg"] == "list"]
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    wins = sum(x - y > spread for x, y in zip(ta, tb))
    comps = [r[-1][3] for r in rows[0]["rows"]]
    lines = ["# tools/bench_eval_pages.py: %d pages of %dx%d (pseg_amd.synth), %d classes, connectivity 4, ms per page, host wall clock, "
             "%d alternations, one process per run" % (args.pages, SHAPE[0], SHAPE[1], CLASSES, args.alternations),
             "# every leg gave the same scores; ink components per page: median %s, range %s .. %s" % (statistics.median(comps), min(comps), max(comps)),
             "## (a) per page: count_matches x %d, total_accuracy, fgpa, ConnectedComponentEval.run_per_component(cc_matching(1, .5, .1)) (page) "
             "against (b) one evaluate_pages call (list)" % CLASSES,
             "page: median %.3f, runs %s" % (statistics.median(ta), " ".join("%.3f" % v for v in ta)),
             "list: median %.3f, runs %s" % (statistics.median(tb), " ".join("%.3f" % v for v in tb)),
             "list / page = %.3f (medians); spread %.3f ms; list below page by more than the spread in %d of %d alternations"
             % (statistics.median(tb) / statistics.median(ta), spread, wins, len(ta))]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    pages = make_pages(8)
    for _ in range(3):
        rows = score_list(pages)
    print("kernel-run: 8 pages x 3 rounds, components %r" % ([r[-1][3] for r in rows],))


def kernel_times(args):
    px = SHAPE[0] * SHAPE[1]
    lines = ["## (c) per-kernel times, rocprofv3 --kernel-trace --stats over `--kernel-run` (8 pages of %dx%d per launch, 3 launches each)" % SHAPE]
    stats = []                                                             # (kernel name, calls, total ns): the CSV, or the run's database
    for path in glob.glob(os.path.join(args.kernel_times, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            stats += [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    for path in glob.glob(os.path.join(args.kernel_times, "**", "*_results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(path) as db:
            stats += list(db.execute("select name, count(*), sum(duration) from kernels group by name"))
    total = 0.0
    for name, calls, ns in stats:
        if any(k in name for k in KERNELS):
            total += ns / 1e3 / calls / 8
            lines.append("  %-18s calls %d  %9.1f us per launch  %8.1f us per page" % (
                [k for k in KERNELS if k in name][0], calls, ns / 1e3 / calls, ns / 1e3 / calls / 8))
    lines.append("  all kernels %.1f us per page; the page's three maps (%.1f MB) take %.1f us at %.0f GB/s: once for the histogram, once for the tiles"
                 % (total, 3 * px / 1e6, 3 * px / HBM_GBS / 1e3, HBM_GBS))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", metavar="LEG", choices=("page", "list"))
    ap.add_argument("--dir", default=None, help="where --child finds the driver's pages (none: it makes them)")
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-times", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_pages.txt"))
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
