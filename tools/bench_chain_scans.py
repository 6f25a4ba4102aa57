#!/usr/bin/env python
"""Scans to mask PNG files: the route through host arrays (a: DatasetLoader.load_images for every entry, then
Predictor.write_masks_dataset -- what a caller had before pseg_predict_chain_scans_png) against the scan chain (b:
Predictor.write_masks_scans).

  python tools/bench_chain_scans.py                       all runs, report to profiles/chain_scans.txt
  python tools/bench_chain_scans.py --child a files DIR   one process of one route (what the driver starts; prints JSON lines)
  python tools/bench_chain_scans.py --kernel-run a|b      8 scans through one route at the Engine level, 3 rounds, nothing timed: run it
                                                          under `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_chain_scans.py --kernel-count DIR    kernel launches per scan from that run's *kernel_stats.csv

Workload: 64 synthetic scans of 1700x1200 (pseg_amd.synth, ink dark), every scan with its own line height so that the pages land
within +-5 % of 842x595 (the shapes of profiles/chain_mixed.txt), fcn_skip with 3 classes, bf16 engine, the vote, encoder levels 0 and
1, high_res_output off and on, files into tmpfs.  Every route runs twice: from pre-decoded arrays handed to the Engine-level calls
(a: engine.prepare_images per scan, binarised on the host as load_images does, then predict_chain_pages(mixed=True); b:
predict_chain_scans; streams discarded) -- device plus staging only --, and from PNG files through the Predictor, the decode timed on
its own.  Three alternations a b a b a b, each run a process of its own that warms up before it measures.  Times are host wall
clock, ms per scan."""
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

TARGET_LINE_HEIGHT = 6
SCAN_SHAPE = (1700, 1200)


def page_heights(n, H=842, spread=0.05, seed=5):
    rng = np.random.default_rng(seed)
    return [int(round(H * (1 + rng.uniform(-spread, spread)))) for _ in range(n)]


def line_heights(n):
    """Per scan the line height that brings a SCAN_SHAPE scan to a page of the drawn height (the width follows: 1200 / 1700 of it)."""
    return [TARGET_LINE_HEIGHT * SCAN_SHAPE[0] / h for h in page_heights(n)]


def write_scans(directory, n):
    from PIL import Image
    from pseg_amd import synth
    os.makedirs(directory, exist_ok=True)
    for k in range(n):
        scan = (255 - synth.synth_page(k, SCAN_SHAPE[0], SCAN_SHAPE[1], 3)[0]).astype(np.uint8)
        Image.fromarray(scan).save(os.path.join(directory, "scan%03d.png" % k))


def make_predictor(high_res):
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=high_res)
    return Predictor(settings, net), cm


def arrays_a(eng, scans, scales, high_res, level, lut):
    """Route a at the Engine level; -> (ms for the front end, ms for the chain)."""
    from pseg_amd import engine as E
    t0 = time.perf_counter()
    prep = [E.prepare_images(s, np.where(s > 127, 255, 0).astype(np.uint8), sc) for s, sc in zip(scans, scales)]
    t1 = time.perf_counter()
    eng.predict_chain_pages([p[0] for p in prep], binaries=[p[2] if high_res else p[1] for p in prep],
                            out_shapes=[s.shape for s in scans] if high_res else None, post_ops=["cc_vote"], lut=lut, png_level=level,
                            mixed=True, sink=lambda page, name, data: None)
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def arrays_b(eng, scans, scales, high_res, level, lut):
    t0 = time.perf_counter()
    eng.predict_chain_scans(scans, scales, high_res=high_res, post_ops=["cc_vote"], lut=lut, png_level=level, sink=lambda page, name, data: None)
    return 0.0, (time.perf_counter() - t0) * 1e3


def files_a(pred, loader, entries, out_dir, level):
    import dataclasses
    from ocr4all_pixel_classifier.lib.dataset import Dataset
    t0 = time.perf_counter()
    ds = Dataset([loader.load_images(dataclasses.replace(e)) for e in entries], loader.color_map)
    t1 = time.perf_counter()
    n = sum(1 for _ in pred.write_masks_dataset(ds, out_dir, level=level))
    assert n == len(entries)
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def files_b(pred, loader, entries, out_dir, level):
    t0 = time.perf_counter()
    n = sum(1 for _ in pred.write_masks_scans(entries, loader, out_dir, level=level))
    assert n == len(entries)
    return 0.0, (time.perf_counter() - t0) * 1e3


def child(args):
    """One process: every (high_res, level) of one route from one source, each warmed up once and measured once."""
    import pseg_amd
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData, _imread_gray
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    route, source, directory = args.child
    paths = sorted(glob.glob(os.path.join(directory, "scan*.png")))[:args.scans]
    n = len(paths)
    lh = line_heights(n)
    t0 = time.perf_counter()
    scans = [np.ascontiguousarray(_imread_gray(p), dtype=np.uint8) for p in paths]
    decode_ms = (time.perf_counter() - t0) * 1e3 / n
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    for high_res in (False, True):
        pred, cm = make_predictor(high_res)
        loader = DatasetLoader(TARGET_LINE_HEIGHT, cm, prediction=True)
        entries = [SingleData(image_path=p, line_height_px=h) for p, h in zip(paths, lh)]
        scales = [TARGET_LINE_HEIGHT / h for h in lh]
        out_dir = os.path.join(directory, "out_%s_%s_%d" % (route, source, high_res))
        for level in args.levels:
            if source == "arrays":
                run = lambda: (arrays_a if route == "a" else arrays_b)(pred.network.model, scans, scales, high_res, level, lut)
            else:
                run = lambda: (files_a if route == "a" else files_b)(pred, loader, entries, out_dir, level)
            run()                                                      # warm-up: code objects, staging sets, the canvases, page cache
            front, rest = run()
            print(json.dumps({"route": route, "source": source, "high_res": int(high_res), "level": level, "front_ms": front / n,
                              "chain_ms": rest / n, "ms": (front + rest) / n, "decode_ms": decode_ms, "scans": n}), flush=True)
        pred.network.model.close()
        shutil.rmtree(out_dir, ignore_errors=True)


def same_files(a, b):
    names = sorted(os.path.relpath(p, a) for p in glob.glob(os.path.join(a, "*", "*.png")))
    assert names and names == sorted(os.path.relpath(p, b) for p in glob.glob(os.path.join(b, "*", "*.png")))
    return all(open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read() for n in names)


def drive(args):
    base = tempfile.mkdtemp(prefix="chain_scans_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    rows = []
    try:
        write_scans(base, args.scans)
        for source in ("arrays", "files"):
            for alt in range(args.alternations):
                for route in ("a", "b"):
                    print("from %s, alternation %d, route %s" % (source, alt, route), file=sys.stderr, flush=True)
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, source, base, "--scans", str(args.scans),
                                          "--levels"] + [str(v) for v in args.levels], check=True, capture_output=True, text=True, timeout=600).stdout
                    for ln in out.splitlines():
                        if ln.startswith("{"):
                            rows.append(dict(json.loads(ln), alternation=alt))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    lines = ["# tools/bench_chain_scans.py: %d scans of %dx%d, pages within +-5 %% of 842x595, fcn_skip 3 classes, bf16, cc_majority, files into %s"
             % (args.scans, SCAN_SHAPE[0], SCAN_SHAPE[1], os.path.dirname(base) or "tmp"),
             "# ms per scan, host wall clock; route a: load_images (arrays: prepare_images) for every scan, then write_masks_dataset (arrays: "
             "predict_chain_pages(mixed=True)); route b: write_masks_scans (arrays: predict_chain_scans); %d alternations, one process per run"
             % args.alternations]
    for source in ("arrays", "files"):
        lines.append("## from %s" % ("pre-decoded arrays, Engine-level calls, streams discarded: device plus staging" if source == "arrays"
                                     else "PNG files through the Predictor, mask files written"))
        for high_res in (0, 1):
            for level in args.levels:
                sel = lambda route: [r for r in rows if (r["route"], r["source"], r["high_res"], r["level"]) == (route, source, high_res, level)]
                a, b = sel("a"), sel("b")
                ta, tb = [r["ms"] for r in a], [r["ms"] for r in b]
                spread = max(max(ta) - min(ta), max(tb) - min(tb))
                wins = sum(x - y > spread for x, y in zip(ta, tb))
                tag = "high_res %s level %d" % ("on " if high_res else "off", level)
                lines.append("%s route a: median %.3f (front end %.3f + chain %.3f), runs %s" % (
                    tag, statistics.median(ta), statistics.median(r["front_ms"] for r in a), statistics.median(r["chain_ms"] for r in a),
                    " ".join("%.3f" % v for v in ta)))
                lines.append("%s route b: median %.3f, runs %s" % (tag, statistics.median(tb), " ".join("%.3f" % v for v in tb)))
                lines.append("%s: b / a = %.3f (medians); spread %.3f ms; b below a by more than the spread in %d of %d alternations"
                             % (tag, statistics.median(tb) / statistics.median(ta), spread, wins, len(ta)))
        if source == "files":
            dec = [r["decode_ms"] for r in rows if r["source"] == "files"]
            lines.append("decode alone (PIL, one thread, page cache warm): median %.3f ms per scan, range %.3f .. %.3f" % (statistics.median(dec), min(dec), max(dec)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def kernel_run(args):
    import pseg_amd
    from pseg_amd import synth
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    eng = pseg_amd.Engine("fcn_skip", 3, mode=pseg_amd.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    n = 8
    scans = [(255 - synth.synth_page(k, SCAN_SHAPE[0], SCAN_SHAPE[1], 3)[0]).astype(np.uint8) for k in range(n)]
    scales = [TARGET_LINE_HEIGHT / h for h in line_heights(n)]
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    for _ in range(3):
        (arrays_a if args.kernel_run == "a" else arrays_b)(eng, scans, scales, False, 0, lut)
    eng.close()
    print("kernel-run %s: %d scans x 3 rounds" % (args.kernel_run, n))


def kernel_count(args):
    calls, front = 0, {}
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                calls += int(r["Calls"])
                if any(k in r["Name"] for k in ("scan_", "gauss_pass", "minmax", "third_value", "bicubic", "nearest_kernel", "prep_map")):
                    front[r["Name"].split("(")[0][:60]] = (int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3)
    lines = ["kernel launches: %d in all, %.1f per scan (8 scans x 3 rounds); the front end's:" % (calls, calls / 24.0)]
    for name, (c, us) in sorted(front.items()):
        lines.append("  %-60s calls %4d  %.2f per scan  %9.1f us per scan" % (name, c, c / 24.0, us / 24.0))
    lines.append("  front end: %.1f launches, %.1f us per scan" % (sum(c for c, _ in front.values()) / 24.0, sum(u for _, u in front.values()) / 24.0))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", nargs=3, metavar=("ROUTE", "SOURCE", "DIR"))
    ap.add_argument("--kernel-run", choices=["a", "b"])
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/chain_scans.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "chain_scans.txt")
    return drive(args)


if __name__ == "__main__":
    main()
