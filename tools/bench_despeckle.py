#!/usr/bin/env python
"""The despeckling, measured: one pseg_amd.despeckle_maps call against the host entry and the scipy.ndimage restatement (a), the
default route of Predictor.write_masks_scans on this tree against a checkout of the parent commit (b), and write_masks_scans with
despeckle=Despeckle() against despeckle=None (c).

  python tools/bench_despeckle.py [--parent DIR]        all runs, report to profiles/despeckle.txt ((b) needs a built parent checkout)
  python tools/bench_despeckle.py --child LEG [DIR]     one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_despeckle.py --kernel-run          8 maps, 3 list calls, nothing timed: run it under
                                                        `rocprofv3 --kernel-trace --stats --output-format csv` (a run of its
                                                        own, no counters)
  python tools/bench_despeckle.py --kernel-count DIR    per-kernel times and bytes from that run's *kernel_stats.csv

Workload: tools/bench_chain_scans.py's 64 synthetic scans of 1700x1200 with its line heights (max_area follows from them),
connectivity 8, ink = scan <= 127; fcn_skip with 3 classes, bf16 engine, the vote, files into tmpfs.  Three alternations, each leg a
process of its own that warms up before it measures.  Times are host wall clock, ms per scan."""
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

SCIPY_MAPS = 4                   # the restatement is timed on a few maps only
HBM_BYTES_PER_S = 8.0e12         # MI355X peak


def synth_inks(n):
    from pseg_amd import synth
    return [((255 - synth.synth_page(k, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], 3)[0]) <= 127).astype(np.uint8) for k in range(n)]


def child_calls(leg, n):
    import pseg_amd
    inks = synth_inks(n)
    how = [pseg_amd.Despeckle().resolved(h) for h in S.line_heights(n)]
    if leg == "scipy":
        import despeckle_cases as C
        run, m = (lambda: [C.restated(g, d.max_area, 8)[0] for g, d in zip(inks[:SCIPY_MAPS], how)]), SCIPY_MAPS
    else:
        run, m = (lambda: pseg_amd.despeckle_maps(inks, how, host=(leg == "host"), counts=True)), n
    got = run()
    t0 = time.perf_counter()
    run()
    row = {"leg": leg, "ms": (time.perf_counter() - t0) * 1e3 / m, "maps": m, "areas": sorted({d.max_area for d in how})}
    if leg != "scipy":
        row["erased"], row["erased_px"], row["kept"] = (int(v) for v in got[1].sum(0))
        row["ink_px"] = int(sum(int(g.sum()) for g in inks))
    print(json.dumps(row), flush=True)


def child_masks(leg, directory, n):
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:n]
    lh = S.line_heights(len(paths))
    how = pseg_amd.Despeckle() if leg == "masks-despeckle" else None
    for high_res in (False, True):
        pred, cm = S.make_predictor(high_res)
        loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm, prediction=True)
        entries = [SingleData(image_path=p, line_height_px=h) for p, h in zip(paths, lh)]
        out_dir = os.path.join(directory, "out_%s_%d" % (leg, high_res))
        run = lambda: sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=0, despeckle=how))
        run()
        t0 = time.perf_counter()
        run()
        print(json.dumps({"leg": leg, "high_res": int(high_res), "ms": (time.perf_counter() - t0) * 1e3 / len(paths), "scans": len(paths),
                          "areas": sorted({pseg_amd.despeckle_area(h) for h in lh})}), flush=True)
        pred.network.model.close()
        shutil.rmtree(out_dir, ignore_errors=True)


def _rows(cmd, cwd=None):
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900, cwd=cwd).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _line(tag, vals):
    return "%s: median %.3f, runs %s" % (tag, statistics.median(vals), " ".join("%.3f" % v for v in vals))


def drive(args):
    base = tempfile.mkdtemp(prefix="despeckle_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    me = os.path.abspath(__file__)
    n = ["--scans", str(args.scans)]
    lines = ["# tools/bench_despeckle.py: %d scans of %dx%d (pseg_amd.synth), ms per scan, host wall clock, %d alternations, one process per leg"
             % (args.scans, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], args.alternations)]
    try:
        S.write_scans(base, args.scans)
        # (a)
        rows = []
        for alt in range(args.alternations):
            for leg in ("scipy", "host", "list"):
                print("(a) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg] + n)
        dev = [r for r in rows if r["leg"] == "list"][0]
        host = [r for r in rows if r["leg"] == "host"][0]
        lines.append("## (a) one despeckle_maps call over the list, copies and counts included (list) against despeckle_maps(host=True) (host) and "
                     "the scipy.ndimage restatement (scipy, %d maps); max_area %s, connectivity 8" % (SCIPY_MAPS, dev["areas"]))
        lines.append("the list's maps: %d ink pixels, %d components erased (%d pixels), %d kept; the host entry counts %s"
                     % (dev["ink_px"], dev["erased"], dev["erased_px"], dev["kept"],
                        "the same" if (host["erased"], host["erased_px"], host["kept"]) == (dev["erased"], dev["erased_px"], dev["kept"]) else "OTHERWISE"))
        t = {leg: [r["ms"] for r in rows if r["leg"] == leg] for leg in ("scipy", "host", "list")}
        for leg in ("scipy", "host", "list"):
            lines.append(_line("%-5s" % leg, t[leg]))
        lines.append("list / scipy = %.4f, list / host = %.4f (medians)"
                     % (statistics.median(t["list"]) / statistics.median(t["scipy"]), statistics.median(t["list"]) / statistics.median(t["host"])))
        # (b)
        if args.parent:
            rows = {"parent": [], "this": []}
            for alt in range(args.alternations):
                for leg, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                    print("(b) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                    rows[leg] += _rows([sys.executable, os.path.join(tree, "tools", "bench_chain_scans.py"), "--child", "b", "files", base,
                                        "--levels", "0"] + n, cwd=tree)
            lines.append("## (b) write_masks_scans, despeckle=None (tools/bench_chain_scans.py --child b files, level 0): the parent commit against this tree")
            for hr in (0, 1):
                tp, tt = ([r["ms"] for r in rows[leg] if r["high_res"] == hr] for leg in ("parent", "this"))
                lines.append(_line("high_res %d parent" % hr, tp))
                lines.append(_line("high_res %d this  " % hr, tt))
                lines.append("high_res %d: this / parent = %.3f (medians); spread of the parent's repeats %.3f ms, this - parent = %+.3f ms"
                             % (hr, statistics.median(tt) / statistics.median(tp), max(tp) - min(tp), statistics.median(tt) - statistics.median(tp)))
        # (c)
        rows = []
        for alt in range(args.alternations):
            for leg in ("masks-none", "masks-despeckle"):
                print("(c) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg, base] + n)
        lines.append("## (c) write_masks_scans(despeckle=Despeckle()) against despeckle=None, level 0; max_area %s"
                     % sorted({a for r in rows for a in r["areas"]}))
        for hr in (0, 1):
            t0, t1 = ([r["ms"] for r in rows if r["leg"] == leg and r["high_res"] == hr] for leg in ("masks-none", "masks-despeckle"))
            lines.append(_line("high_res %d none     " % hr, t0))
            lines.append(_line("high_res %d despeckle" % hr, t1))
            lines.append("high_res %d: the despeckling adds %.3f ms per scan (medians)" % (hr, statistics.median(t1) - statistics.median(t0)))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    inks = synth_inks(8)
    how = [pseg_amd.Despeckle().resolved(h) for h in S.line_heights(8)]
    for _ in range(3):
        pseg_amd.despeckle_maps(inks, how)
    print("kernel-run: 8 maps x 3 calls")


def kernel_count(args):
    from pseg_amd import engine as E
    th, tw, slots, run_cap = E.despeckle_geometry()
    H, W = S.SCAN_SHAPE
    tiles = -(-H // th) * -(-W // tw)
    # bytes by count, per map, as upper bounds where the data decides: the tile kernel reads every pixel once and its ring, and writes
    # per tile the three lengths (the slots, rim bytes, tasks and runs of open components come on top: data dependent, not counted);
    # the other three read per tile the lengths they need, the rest is data dependent
    moved = {"ds_tile": H * W + tiles * (2 * (th + tw) + 4 + 12), "ds_border": tiles * 4, "ds_merge": tiles * 4, "ds_apply": tiles * 8}
    lines = ["## per-kernel times, rocprofv3 --kernel-trace --stats over `--kernel-run` (8 maps per launch, 3 calls); bytes by count are the",
             "## data-independent part (%d tiles of %d x %d per map)" % (tiles, th, tw)]
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for key, nbytes in moved.items():
                    if key in r["Name"]:
                        us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]) / 8.0
                        lines.append("  %-22s calls %d  %8.1f us per map  %7.3f MB per map by count  %.3f TB/s = %.1f %% of the HBM peak (%.0f TB/s)"
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
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/despeckle.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        if args.child[0] in ("scipy", "host", "list"):
            return child_calls(args.child[0], args.scans)
        return child_masks(args.child[0], args.child[1], args.scans)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "despeckle.txt")
    return drive(args)


if __name__ == "__main__":
    main()
