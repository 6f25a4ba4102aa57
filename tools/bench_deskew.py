#!/usr/bin/env python
"""The deskewing, measured: one pseg_amd.deskew_scans call against the host entry and the conventional method with SciPy (a), the
default route of Predictor.write_masks_scans and the bench.py headline on this tree against a checkout of the parent commit (b), and
write_masks_scans with deskew=Skew() against deskew=None (c).

  python tools/bench_deskew.py [--parent DIR]        all runs, report to profiles/deskew.txt ((b) needs a built parent checkout)
  python tools/bench_deskew.py --child LEG [DIR]     one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_deskew.py --kernel-run          8 scans, 3 list calls, nothing timed: run it under
                                                     `rocprofv3 --kernel-trace --stats --output-format csv` (a run of its own,
                                                     no counters)
  python tools/bench_deskew.py --kernel-count DIR    per-kernel times and bytes from that run's *kernel_stats.csv

Workload: tools/bench_chain_scans.py's 64 synthetic scans of 1700x1200, each skewed by a planted index (drawn from a seed in
-80 .. 80 over 1024, rotated on the host, order 1, fill 255); Skew() = 89 steps over 1024.  The SciPy leg is the conventional method
as ocropus-nlbin does it -- scipy.ndimage.rotate, order 0, per candidate angle, the variance of the row means, 8 angles per degree
over +-5 degrees -- on the first few scans only.  Three alternations, each leg a process of its own that warms up before it
measures.  Times are host wall clock, ms per scan."""
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

SCIPY_SCANS = 2                  # the conventional method is timed on a few scans only
HBM_BYTES_PER_S = 8.0e12         # MI355X peak
DENOM = 1024


def planted(n):
    return [int(v) for v in np.random.default_rng(77).integers(-80, 81, n)]


def skewed_scans(n):
    import pseg_amd
    from pseg_amd import synth
    scans = [(255 - synth.synth_page(k, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], 3)[0]).astype(np.uint8) for k in range(n)]
    return [pseg_amd.rotate_maps([s], -a, denom=DENOM, order=1, fill=255, host=True)[0] for s, a in zip(scans, planted(n))]


def scipy_skew(scan):
    """The conventional estimate: the angle whose rotation gives the row means the largest variance, as an index over DENOM."""
    from scipy import ndimage
    ink = (scan <= 127).astype(np.float32)
    angles = np.linspace(-5, 5, 81)
    # ndimage.rotate turns counter-clockwise for a positive angle (y down): the angle that straightens lines of slope +t is +atan(t)
    var = [np.var(ndimage.rotate(ink, a, order=0, reshape=False).mean(1)) for a in angles]
    return int(round(np.tan(np.radians(angles[int(np.argmax(var))])) * DENOM))


def child_calls(leg, n):
    import pseg_amd
    scans, want = skewed_scans(n), planted(n)
    how = pseg_amd.Skew(5.0, DENOM)
    if leg == "scipy":
        run, m = (lambda: [scipy_skew(s) for s in scans[:SCIPY_SCANS]]), SCIPY_SCANS
        t0 = time.perf_counter()
        got = run()
    else:
        run, m = (lambda: pseg_amd.deskew_scans(scans, how, host=(leg == "host"))[1].tolist()), n
        run()
        t0 = time.perf_counter()
        got = run()
    err = [abs(g - w) for g, w in zip(got, want)]
    print(json.dumps({"leg": leg, "ms": (time.perf_counter() - t0) * 1e3 / m, "scans": m, "exact": sum(e == 0 for e in err),
                      "within3": sum(e <= 3 for e in err), "worst": max(err)}), flush=True)


def child_masks(leg, directory, n):
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:n]
    lh = S.line_heights(len(paths))
    how = pseg_amd.Skew(5.0, DENOM) if leg == "masks-deskew" else None
    for high_res in (False, True):
        pred, cm = S.make_predictor(high_res)
        loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm, prediction=True)
        entries = [SingleData(image_path=p, line_height_px=h) for p, h in zip(paths, lh)]
        out_dir = os.path.join(directory, "out_%s_%d" % (leg, high_res))
        run = lambda: sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=0, deskew=how))
        run()
        t0 = time.perf_counter()
        run()
        print(json.dumps({"leg": leg, "high_res": int(high_res), "ms": (time.perf_counter() - t0) * 1e3 / len(paths), "scans": len(paths)}), flush=True)
        pred.network.model.close()
        shutil.rmtree(out_dir, ignore_errors=True)


def _rows(cmd, cwd=None):
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900, cwd=cwd).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def _line(tag, vals):
    return "%s: median %.3f, runs %s" % (tag, statistics.median(vals), " ".join("%.3f" % v for v in vals))


def write_skewed(directory, n):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for k, s in enumerate(skewed_scans(n)):
        Image.fromarray(s).save(os.path.join(directory, "scan%03d.png" % k))


def drive(args):
    base = tempfile.mkdtemp(prefix="deskew_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    me = os.path.abspath(__file__)
    n = ["--scans", str(args.scans)]
    lines = ["# tools/bench_deskew.py: %d scans of %dx%d (pseg_amd.synth), planted skews of -80 .. 80 over %d, ms per scan, host wall clock, "
             "%d alternations, one process per leg" % (args.scans, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], DENOM, args.alternations)]
    try:
        # (a)
        rows = []
        for alt in range(args.alternations):
            for leg in ("scipy", "host", "list"):
                print("(a) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg] + n)
        lines.append("## (a) one deskew_scans call over the list, copies included (list) against deskew_scans(host=True) (host) and the "
                     "conventional method with SciPy (scipy: estimate only, %d scans, 81 angles)" % SCIPY_SCANS)
        t = {leg: [r["ms"] for r in rows if r["leg"] == leg] for leg in ("scipy", "host", "list")}
        for leg in ("scipy", "host", "list"):
            r = [r for r in rows if r["leg"] == leg][0]
            lines.append(_line("%-5s" % leg, t[leg]) + "; of %d planted indices: %d exact, %d within 3 steps, worst %d steps"
                         % (r["scans"], r["exact"], r["within3"], r["worst"]))
        lines.append("list / scipy = %.4f, list / host = %.4f (medians)"
                     % (statistics.median(t["list"]) / statistics.median(t["scipy"]), statistics.median(t["list"]) / statistics.median(t["host"])))
        # (b)
        if args.parent:
            S.write_scans(base, args.scans)
            rows = {"parent": [], "this": []}
            heads = {"parent": [], "this": []}
            for alt in range(args.alternations):
                for leg, tree in (("parent", os.path.abspath(args.parent)), ("this", ROOT)):
                    print("(b) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                    rows[leg] += _rows([sys.executable, os.path.join(tree, "tools", "bench_chain_scans.py"), "--child", "b", "files", base,
                                        "--levels", "0"] + n, cwd=tree)
                    heads[leg] += _rows([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "1000", "--warmup", "20"], cwd=tree)
            lines.append("## (b) write_masks_scans, deskew=None (tools/bench_chain_scans.py --child b files, level 0): the parent commit against this tree")
            for hr in (0, 1):
                tp, tt = ([r["ms"] for r in rows[leg] if r["high_res"] == hr] for leg in ("parent", "this"))
                lines.append(_line("high_res %d parent" % hr, tp))
                lines.append(_line("high_res %d this  " % hr, tt))
                lines.append("high_res %d: this / parent = %.3f (medians); the parent's repeats span %.3f .. %.3f ms, this tree's median %s inside"
                             % (hr, statistics.median(tt) / statistics.median(tp), min(tp), max(tp),
                                "lies" if min(tp) <= statistics.median(tt) <= max(tp) else "DOES NOT lie"))
            lines.append("## bench.py --gpus 1 --steps 1000 --warmup 20, alternated (the headline does not involve this path)")
            for leg in ("parent", "this"):
                lines.append("  %-6s %s Mpixels/s (%s ms per step)" % (leg, " / ".join("%.1f" % r["value"] for r in heads[leg]),
                                                                      " / ".join("%.4f" % r["ms_per_step"] for r in heads[leg])))
            shutil.rmtree(base, ignore_errors=True)
        # (c)
        write_skewed(base, args.scans)
        rows = []
        for alt in range(args.alternations):
            for leg in ("masks-none", "masks-deskew"):
                print("(c) alternation %d, %s" % (alt, leg), file=sys.stderr, flush=True)
                rows += _rows([sys.executable, me, "--child", leg, base] + n)
        lines.append("## (c) write_masks_scans(deskew=Skew()) against deskew=None on the skewed scans, level 0")
        for hr in (0, 1):
            t0, t1 = ([r["ms"] for r in rows if r["leg"] == leg and r["high_res"] == hr] for leg in ("masks-none", "masks-deskew"))
            lines.append(_line("high_res %d none  " % hr, t0))
            lines.append(_line("high_res %d deskew" % hr, t1))
            lines.append("high_res %d: the deskewing adds %.3f ms per scan (medians)" % (hr, statistics.median(t1) - statistics.median(t0)))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    scans = skewed_scans(8)
    for _ in range(3):
        pseg_amd.deskew_scans(scans, pseg_amd.Skew(5.0, DENOM))
    print("kernel-run: 8 scans x 3 calls")


def kernel_count(args):
    H, W = S.SCAN_SHAPE
    K, cand = -(-W // 32), 2 * 89 + 1
    apron = max(abs((a * c + DENOM) // (2 * DENOM)) for a in (-89, 89) for c in (32 - W, 64 * (K - 1) + 32 - W))
    rows_p = H + 2 * apron
    # bytes by count, per scan: the strips read the scan once and write a byte per (row, strip); a score workgroup reads its rows of R
    # once per candidate (from L2 after the first); the rotation reads about every source pixel once (its four taps share cache
    # lines) and writes every output pixel once
    moved = {"sk_strips": H * W + H * K, "sk_score": cand * rows_p * K, "sk_pick": cand * 8, "sk_rotate": 2 * H * W}
    lines = ["## (d) per-kernel times, rocprofv3 --kernel-trace --stats over `--kernel-run` (8 scans per launch, 3 calls); bytes by count,",
             "## %d strips, %d candidates; the score kernel's bytes are R read once per candidate, served by L2, not HBM traffic" % (K, cand)]
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for key, nbytes in moved.items():
                    if key in r["Name"]:
                        us = float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]) / 8.0
                        lines.append("  %-18s calls %d  %8.1f us per scan  %7.3f MB per scan by count  %.3f TB/s = %.1f %% of the HBM peak (%.0f TB/s)"
                                     % (r["Name"].split("(")[0].split("::")[-1][:18], int(r["Calls"]), us, nbytes / 1e6, nbytes / us / 1e6,
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
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/deskew.txt)")
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
        args.out = os.path.join(ROOT, "profiles", "deskew.txt")
    return drive(args)


if __name__ == "__main__":
    main()
