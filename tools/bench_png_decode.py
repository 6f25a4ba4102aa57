#!/usr/bin/env python
"""PNG scans decoded on the device (pseg_png_decode_gray) against PIL on host threads.

  python tools/bench_png_decode.py                        all legs, report to profiles/png_decode.txt
  python tools/bench_png_decode.py --child KIND LEG DIR   one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_png_decode.py --kernel-run DIR       the scans of DIR (written with --write-scans) through png_decode_gray, 3 rounds,
                                                          nothing timed: run it under `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_png_decode.py --kernel-count DIR     the two kernels' times from that run's *kernel_stats.csv

Workload: tools/bench_chain_scans.py's 64 synthetic scans of 1700x1200 (8-bit gray, saved by PIL) as PNG files in tmpfs.
  (a) decode alone: PIL (Image.open(path).convert("L")) on 1, 2 and 16 threads, against reading the files' bytes and ONE
      png_decode_gray call; both include the file reads (page cache).
  (b) files to mask files: Predictor.write_masks_scans, fcn_skip 3 classes, bf16, the vote, encoder levels 0 and 1, high_res_output
      off: decode="host" with decode_threads 2 (the default) and 16, against decode="device" (decode_threads 2).
Three alternations over the legs, each run a process of its own that warms up before it measures.  Host wall clock, ms per scan.
Not measured: real scans, other sizes, RGB files."""
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

DECODE_LEGS = ("pil1", "pil2", "pil16", "device")
MASK_LEGS = ("host2", "host16", "device")


def decode_leg(leg, paths):
    from concurrent.futures import ThreadPoolExecutor
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import _imread_gray
    t0 = time.perf_counter()
    if leg == "device":
        got = pseg_amd.png_decode_gray([pseg_amd.engine.read_file_bytes(p) for p in paths])
        assert all(st == 0 for _, st in got)
        out = [a for a, _ in got]
    else:
        with ThreadPoolExecutor(int(leg[3:])) as pool:
            out = list(pool.map(lambda p: np.ascontiguousarray(_imread_gray(p), dtype=np.uint8), paths))
    return (time.perf_counter() - t0) * 1e3, out


def child(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    kind, leg, directory = args.child
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:args.scans]
    n = len(paths)
    if kind == "decode":
        ref = decode_leg("pil16", paths[:4])[1]
        decode_leg(leg, paths)                                         # warm-up: page cache, code objects, the workspace
        ms, out = decode_leg(leg, paths)
        assert all(np.array_equal(a, b) for a, b in zip(out[:4], ref))
        print(json.dumps({"kind": kind, "leg": leg, "ms": ms / n, "scans": n}), flush=True)
        return
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    pred, cm = S.make_predictor(False)
    loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm, prediction=True)
    entries = [SingleData(image_path=p, line_height_px=h) for p, h in zip(paths, S.line_heights(n))]
    kw = {"host2": dict(decode="host", decode_threads=2), "host16": dict(decode="host", decode_threads=16), "device": dict(decode="device", decode_threads=2)}[leg]
    out_dir = os.path.join(directory, "out_" + leg)
    for level in args.levels:
        def run():
            t0 = time.perf_counter()
            assert sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=level, **kw)) == n
            return (time.perf_counter() - t0) * 1e3
        run()
        print(json.dumps({"kind": kind, "leg": leg, "level": level, "ms": run() / n, "scans": n}), flush=True)
    if args.keep:
        shutil.rmtree(args.keep, ignore_errors=True)
        shutil.copytree(out_dir, args.keep)
    shutil.rmtree(out_dir, ignore_errors=True)
    pred.network.model.close()


def verdict(lines, tag, rows, legs, device="device"):
    t = {leg: [r["ms"] for r in rows if r["leg"] == leg] for leg in legs}
    for leg in legs:
        lines.append("%s %-7s median %.3f, runs %s" % (tag, leg, statistics.median(t[leg]), " ".join("%.3f" % v for v in t[leg])))
    host = [leg for leg in legs if leg != device]
    best = min(host, key=lambda leg: statistics.median(t[leg]))
    spread = max(max(v) - min(v) for v in t.values())
    wins = sum(b - d > spread for b, d in zip(t[best], t[device]))
    lines.append("%s: device / best host leg (%s) = %.3f (medians); spread %.3f ms; device below %s by more than the spread in %d of %d alternations"
                 % (tag, best, statistics.median(t[device]) / statistics.median(t[best]), spread, best, wins, len(t[device])))


def drive(args):
    base = tempfile.mkdtemp(prefix="png_decode_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rows = []
    try:
        S.write_scans(base, args.scans)
        sizes = [os.path.getsize(p) for p in glob.glob(os.path.join(base, "scan*.png"))]
        for alt in range(args.alternations):
            for kind, legs in (("decode", DECODE_LEGS), ("masks", MASK_LEGS)):
                for leg in legs:
                    print("alternation %d, %s, leg %s" % (alt, kind, leg), file=sys.stderr, flush=True)
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, leg, base, "--scans", str(args.scans), "--levels"] + [str(v) for v in args.levels]
                    if kind == "masks" and alt == 0:
                        cmd += ["--keep", os.path.join(base, "kept_" + leg)]
                    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
                    rows += [dict(json.loads(ln), alternation=alt) for ln in out.splitlines() if ln.startswith("{")]
        same = all(S.same_files(os.path.join(base, "kept_host2"), os.path.join(base, "kept_" + leg)) for leg in MASK_LEGS[1:])
    finally:
        shutil.rmtree(base, ignore_errors=True)
    lines = ["# tools/bench_png_decode.py: %d scans of %dx%d, 8-bit gray PNG files saved by PIL, %.0f KiB a file on average, in %s; ms per scan, "
             "host wall clock; %d alternations, one process per leg and alternation"
             % (args.scans, S.SCAN_SHAPE[0], S.SCAN_SHAPE[1], statistics.mean(sizes) / 1024, os.path.dirname(base) or "tmp", args.alternations),
             "## (a) decode alone, file reads included: PIL on 1 / 2 / 16 threads, one png_decode_gray call"]
    verdict(lines, "decode", [r for r in rows if r["kind"] == "decode"], DECODE_LEGS)
    lines.append("## (b) files to mask files: write_masks_scans, fcn_skip 3 classes, bf16, cc_majority, high_res_output off; decode=\"host\" with 2 and "
                 "16 decode threads, decode=\"device\"; the mask files of the three legs are %s" % ("byte-equal" if same else "DIFFERENT"))
    for level in args.levels:
        verdict(lines, "level %d" % level, [r for r in rows if r["kind"] == "masks" and r["level"] == level], MASK_LEGS)
    lines.append("# not measured: real scans, other sizes, RGB files")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def kernel_run(args):
    import pseg_amd
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    paths = sorted(glob.glob(os.path.join(args.kernel_run, "scan*.png")))[:args.scans]
    files = [pseg_amd.engine.read_file_bytes(p) for p in paths]
    for _ in range(3):
        assert all(st == 0 for _, st in pseg_amd.png_decode_gray(files))
    H, W = S.SCAN_SHAPE
    print("kernel-run: %d scans x 3 rounds; %d IDAT bytes and %d inflated bytes a scan on average" % (len(files), sum(map(len, files)) // len(files), H * (W + 1)))


def kernel_count(args):
    lines = []
    H, W = S.SCAN_SHAPE
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "pngdec_" in r["Name"]:
                    calls, us = int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3
                    per_launch = 3 * args.scans // calls               # kernel_run makes 3 rounds; a launch is one group
                    lines.append("  %-28s launches %3d (one per group of %d scans)  %10.1f us per group  %8.1f us per scan  %6.2f inflated bytes per us per stream"
                                 % (r["Name"].split("(")[0].split("::")[-1], calls, per_launch, us / calls, us / (3 * args.scans), H * (W + 1) / (us / calls)))
    text = "## (c) kernel trace, %d scans, 3 rounds (a run of its own)\n" % args.scans + "\n".join(sorted(lines)) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", nargs=3, metavar=("KIND", "LEG", "DIR"))
    ap.add_argument("--keep", default=None, help="(child, masks) copy the written mask files here")
    ap.add_argument("--write-scans", metavar="DIR")
    ap.add_argument("--kernel-run", metavar="DIR")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/png_decode.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.write_scans:
        return S.write_scans(args.write_scans, args.scans)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "png_decode.txt")
    return drive(args)


if __name__ == "__main__":
    main()
