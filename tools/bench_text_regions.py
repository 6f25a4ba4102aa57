#!/usr/bin/env python
"""The text regions, measured: one pseg_amd.text_regions call over a list of label maps (copies included) against the host entry
(host=True) and the NumPy / SciPy restatement of tests/regions_cases.py.

  python tools/bench_text_regions.py                    all legs, report to profiles/text_regions.txt
  python tools/bench_text_regions.py --child LEG        one process of one leg (what the driver starts; prints a JSON line)
  python tools/bench_text_regions.py --kernel-run       8 maps, 3 list calls, nothing timed: run it under
                                                        `rocprofv3 --kernel-trace --stats --output-format csv` (a run of its own, no
                                                        counters)
  python tools/bench_text_regions.py --kernel-count DIR per-kernel time per launch and per page from that run's *kernel_stats.csv

Workload: 64 synthetic label maps of 1700x1200 (text lines of words at each map's line height, an image block of another label), the
line heights of tools/bench_chain_scans.py, sides = region_kernels(line height).  Three alternations, each leg a process of its own
that warms up before it measures.  Times are host wall clock, ms per map."""
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
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import bench_chain_scans as S  # noqa: E402

SCIPY_MAPS = 4                   # the restatement is timed on a few maps only
KERNEL_MAPS = 8


def synth_label_map(seed, H, W, ch):
    """Label 1 in text lines of `ch` pixels (words of noisy ink, gaps, the odd empty line), label 2 in an image block."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.uint8)
    ch = max(4, int(ch))
    for y in range(2 * ch, H - 2 * ch, int(1.5 * ch)):
        if rng.random() < 0.12:
            continue
        x = 3 * ch + int(rng.integers(0, ch))
        while x < W - 4 * ch:
            w = int(rng.integers(ch, 6 * ch))
            x1 = min(x + w, W - 3 * ch)
            lab[y:y + int(0.7 * ch), x:x1] = rng.random((int(0.7 * ch), x1 - x)) < 0.55
            x += w + int(rng.integers(ch // 3, ch)) + (12 * ch if rng.random() < 0.05 else 0)
    by, bx = int(rng.integers(H // 4, H // 2)), int(rng.integers(W // 8, W // 3))
    lab[by:by + H // 5, bx:bx + W // 3] = 2
    return lab


def workload(n):
    import pseg_amd
    H, W = S.SCAN_SHAPE
    hs = S.line_heights(n)
    return [synth_label_map(k, H, W, hs[k]) for k in range(n)], [pseg_amd.TextRegions(1, char_height=h) for h in hs]


def child(leg, n):
    import pseg_amd
    maps, how = workload(n)
    if leg == "scipy":
        import regions_cases as C
        run, m = (lambda: [C.restated(g, 1, *h.kernels) for g, h in zip(maps[:SCIPY_MAPS], how)]), SCIPY_MAPS
    else:
        run, m = (lambda: pseg_amd.text_regions(maps, how, host=(leg == "host"))), n
    got = run()
    t0 = time.perf_counter()
    run()
    row = {"leg": leg, "ms": (time.perf_counter() - t0) * 1e3 / m, "maps": m, "sides": sorted({h.kernels for h in how})}
    if leg != "scipy":
        row["regions"] = int(sum(len(r["areas"]) for r in got))
        row["region_px"] = int(sum(int(r["areas"].sum()) for r in got))
    print(json.dumps(row), flush=True)


def _rows(cmd):
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _line(tag, vals):
    return "%s: median %.3f, runs %s" % (tag, statistics.median(vals), " ".join("%.3f" % v for v in vals))


def drive(args):
    me = os.path.abspath(__file__)
    rows = []
    for alt in range(args.alternations):
        for leg in ("scipy", "host", "list"):
            print("alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
            rows += _rows([sys.executable, me, "--child", leg, "--maps", str(args.maps)])
    dev = [r for r in rows if r["leg"] == "list"][0]
    host = [r for r in rows if r["leg"] == "host"][0]
    lines = ["# tools/bench_text_regions.py: %d label maps of %dx%d, ms per map, host wall clock, %d alternations, one process per leg"
             % (args.maps, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], args.alternations),
             "## one text_regions call over the list, copies, masks and tables included (list) against text_regions(host=True) (host) and the",
             "## NumPy / SciPy restatement (scipy, %d maps); sides %s" % (SCIPY_MAPS, dev["sides"]),
             "the list's maps: %d regions of %d pixels; the host entry finds %s"
             % (dev["regions"], dev["region_px"], "the same" if (host["regions"], host["region_px"]) == (dev["regions"], dev["region_px"]) else "OTHERWISE")]
    t = {leg: [r["ms"] for r in rows if r["leg"] == leg] for leg in ("scipy", "host", "list")}
    for leg in ("scipy", "host", "list"):
        lines.append(_line("%-5s" % leg, t[leg]))
    lines.append("list / scipy = %.4f, list / host = %.4f (medians)"
                 % (statistics.median(t["list"]) / statistics.median(t["scipy"]), statistics.median(t["list"]) / statistics.median(t["host"])))
    lines.append("not measured: label maps of real predictions, other page sizes, cv2 itself (OpenCV is not part of the environment)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    maps, how = workload(KERNEL_MAPS)
    for _ in range(3):
        pseg_amd.text_regions(maps, how)
    print("kernel-run: %d maps x 3 calls" % KERNEL_MAPS)


def kernel_count(args):
    lines = ["## per-kernel times, rocprofv3 --kernel-trace --stats over `--kernel-run` (%d maps per launch, 3 calls)" % KERNEL_MAPS]
    total = 0.0
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "rg_" not in r["Name"]:
                    continue
                calls = int(r["Calls"])
                us = float(r["TotalDurationNs"]) / 1e3 / calls
                per_page = float(r["TotalDurationNs"]) / 1e3 / 3.0 / KERNEL_MAPS
                total += per_page
                lines.append("  %-28s calls %3d  %9.1f us per launch  %8.1f us per page (all its launches of a call)"
                             % (r["Name"].split("(")[0].split("::")[-1][:28], calls, us, per_page))
    lines.append("  all rg_ kernels: %.1f us per page" % total)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", metavar="LEG")
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/text_regions.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.maps)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "text_regions.txt")
    return drive(args)


if __name__ == "__main__":
    main()
