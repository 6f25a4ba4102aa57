#!/usr/bin/env python
"""Predictor.predict_regions, measured: the list route (label maps down, one text_regions call up and down, polygons traced on the
host) against the chain route (the regions stage and the device tracer inside the page chain; rows and vertices down).

  python tools/bench_predict_regions.py [--parent DIR]   all legs, report to profiles/predict_regions.txt
                                                         (a) route "list" on a built checkout of the parent commit (needs --parent)
                                                         (b) route "list" on this tree    (c) route "chain" on this tree
  python tools/bench_predict_regions.py --child LEG --tree DIR   one process of one leg (what the driver starts; prints a JSON line)
  python tools/bench_predict_regions.py --kernel-run     8 pages, 3 chain calls, nothing timed: run it under
                                                         `rocprofv3 --kernel-trace --stats --output-format csv` (a run of its own, no
                                                         counters)
  python tools/bench_predict_regions.py --kernel-count DIR   the rg_ kernels' time per page from that run's *kernel_stats.csv

Workload: 64 synthetic 1700x1200 pages at the line heights of tools/bench_chain_scans.py, a bf16 fcn_skip with random weights, the
label named "text".  Three alternations, each leg a process of its own that warms up on 8 pages before it measures one
predict_regions call over all pages.  Times are host wall clock, ms per page."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_PAGES = 8


def use_tree(tree):
    for p in (tree, os.path.join(tree, "page-segmentation_amd"), os.path.join(tree, "tools")):
        if p not in sys.path:
            sys.path.insert(0, p)


def workload(n):
    """-> (predictor, dataset) in the tree that use_tree chose."""
    import numpy as np
    import bench_chain_scans as S
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.dataset import Dataset, SingleData
    pred, cm = S.make_predictor(False)
    pred.settings.post_process = []
    H, W = S.SCAN_SHAPE
    data = []
    for k, lh in enumerate(S.line_heights(n)):
        img, binary, _ = synth.synth_page(k, H, W, 3)
        data.append(SingleData(image=img, binary=binary, original_shape=img.shape, line_height_px=int(round(lh)), image_path="page%03d.png" % k))
    return pred, Dataset(data, cm), np


def child(leg, tree, n):
    use_tree(tree)
    pred, ds, np = workload(n)
    from ocr4all_pixel_classifier.lib.dataset import Dataset
    kw = {} if leg == "a" else {"route": "list" if leg == "b" else "chain"}
    warm = Dataset(ds.data[:8], ds.color_map)
    pred.predict_regions(warm, ds.color_map, **kw)
    t0 = time.perf_counter()
    got = pred.predict_regions(ds, ds.color_map, **kw)
    ms = (time.perf_counter() - t0) * 1e3 / n
    out = {"leg": leg, "ms": ms, "pages": n, "regions": sum(len(r) for r in got), "vertices": sum(len(t.polygon) for r in got for t in r)}
    if leg == "c":                                 # how many of the first pages the stage could not finish (they took the list route)
        res = pred.network.model.predict_chain_pages([np.asarray(d.image) for d in ds.data[:8]], which=(), labels=False,
                                                     regions=__import__("pseg_amd").TextRegions(1, char_height=ds.data[0].line_height_px))
        out["fallbacks_of_8"] = sum(r["regions"]["status"] != 0 for r in res)
    print(json.dumps(out), flush=True)


def run_child(leg, tree, n):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--tree", tree, "--pages", str(n)], capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        raise SystemExit("leg %s failed (%d):\n%s" % (leg, r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def drive(args):
    legs = [("b", ROOT), ("c", ROOT)]
    if args.parent:
        legs.insert(0, ("a", os.path.abspath(args.parent)))
    rows = {leg: [] for leg, _ in legs}
    for _ in range(args.alternations):
        for leg, tree in legs:
            rows[leg].append(run_child(leg, tree, args.pages))
            print(rows[leg][-1], flush=True)
    name = {"a": "(a) route list, parent commit", "b": "(b) route list, this tree", "c": "(c) route chain, this tree"}
    lines = ["# tools/bench_predict_regions.py: Predictor.predict_regions over %d pages of 1700x1200, bf16 fcn_skip, ms per page, host wall clock, "
             "%d alternations, one process per leg" % (args.pages, args.alternations)]
    for leg, _ in legs:
        ms = [r["ms"] for r in rows[leg]]
        lines.append("%-32s median %8.3f  (runs %s)  regions %d  vertices %d%s"
                     % (name[leg], statistics.median(ms), " ".join("%.3f" % v for v in ms), rows[leg][0]["regions"], rows[leg][0]["vertices"],
                        "  fallbacks among the first 8 pages: %d" % rows[leg][0]["fallbacks_of_8"] if leg == "c" else ""))
    base = "a" if args.parent else "b"
    bm = [r["ms"] for r in rows[base]]
    spread = max(bm) - min(bm)
    lines.append("spread of %s's repeats: %.3f ms" % (name[base][:3], spread))
    if args.parent:
        lines.append("(b) - (a), medians: %+.3f ms (%s the spread)" % (statistics.median([r["ms"] for r in rows["b"]]) - statistics.median(bm),
                                                                      "inside" if abs(statistics.median([r["ms"] for r in rows["b"]]) - statistics.median(bm)) <= spread else "OUTSIDE"))
    wins = [rows[base][k]["ms"] - rows["c"][k]["ms"] > spread for k in range(args.alternations)]
    lines.append("(c) below %s by more than the spread in %d of %d alternations: the chain route %s the default"
                 % (name[base][:3], sum(wins), len(wins), "may be" if all(wins) else "does not become"))
    assert all(rows[leg][0]["regions"] == rows[base][0]["regions"] and rows[leg][0]["vertices"] == rows[base][0]["vertices"] for leg, _ in legs), "the legs disagree"
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


def kernel_run(args):
    use_tree(ROOT)
    pred, ds, _ = workload(KERNEL_PAGES)
    for _ in range(3):
        pred.predict_regions(ds, ds.color_map, route="chain")
    print("kernel-run: %d pages x 3 calls" % KERNEL_PAGES)


def kernel_count(args):
    lines = ["## the regions kernels inside the chain, rocprofv3 --kernel-trace --stats over `--kernel-run` (%d pages, 3 calls), us per page" % KERNEL_PAGES]
    tracer = rest = 0.0
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "rg_" not in r["Name"]:
                    continue
                per_page = float(r["TotalDurationNs"]) / 1e3 / 3.0 / KERNEL_PAGES
                short = r["Name"].split("(")[0].split("::")[-1][:28]
                if "rg_trace" in r["Name"] or "rg_scan" in r["Name"]:
                    tracer += per_page
                else:
                    rest += per_page
                lines.append("  %-28s calls %3d  %8.1f us per page" % (short, int(r["Calls"]), per_page))
    lines.append("  the tracer (rg_trace_kernel x 2, rg_scan_kernel): %.1f us per page; the other region launches: %.1f us per page" % (tracer, rest))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for leg (a)")
    ap.add_argument("--child", metavar="LEG")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_regions.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.tree, args.pages)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        use_tree(ROOT)
        return kernel_count(args)
    return drive(args)


if __name__ == "__main__":
    main()
