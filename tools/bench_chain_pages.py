#!/usr/bin/env python
"""A book through the Predictor to mask PNG files: page by page (leg A, a loop of Predictor.write_masks) against the page list
(leg B, Predictor.write_masks_dataset -> pseg_predict_chain_pages_png).

  python tools/bench_chain_pages.py                     both legs, alternated; report to profiles/chain_pages.txt
  python tools/bench_chain_pages.py --leg A             leg A alone (uses only API that older checkouts have: the baseline run)
  python tools/bench_chain_pages.py --kernel-run        the list entry at unit sizes 1, 2, 4, 8 and both levels, nothing timed: run it
                                                        under `rocprofv3 --kernel-trace` (a run of its own, the profiler slows the host)
  python tools/bench_chain_pages.py --kernel-table CSV  the band-kernel table from that run's *_kernel_trace.csv: launches grouped by
                                                        the pages they encode (grid z), time per page against single-page launches

  python tools/bench_chain_pages.py --mixed             a book of pages of DIFFERENT shapes: legs A, B (mixed=False: units of same-shape
                                                        runs) and C (mixed=True: units by canvas); report to profiles/chain_mixed.txt
  python tools/bench_chain_pages.py --mixed-kernel-run  8 mixed pages as one ragged encoder launch and as 8 single launches, for a trace
  python tools/bench_chain_pages.py --mixed-kernel-table CSV   the band-kernel time per page of the two, from that trace

Workload: 32 synthetic 2048x1536 pages (pseg_amd.synth), fcn_skip with 3 classes, bf16 engine, the vote as post-processor, files into
tmpfs, encoder levels 0 and 1.  Times are host wall clock around calls that end synchronised with the files written.
--mixed: 64 pages whose shapes are drawn (seeded) within +-5 % of 842x595 -- an A4 scan at 300 dpi scaled by 6/25, every page by its
own line height -- otherwise the same."""
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


def mixed_shapes(n_pages, H=842, W=595, spread=0.05, seed=5):
    rng = np.random.default_rng(seed)
    return [(int(round(H * (1 + rng.uniform(-spread, spread)))), int(round(W * (1 + rng.uniform(-spread, spread))))) for _ in range(n_pages)]


def make_predictor_and_pages(n_pages, H, W, shapes=None):
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
        img, binary, _ = synth.synth_page(k, *(shapes[k] if shapes else (H, W)), 3)
        data.append(SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page%03d.png" % k))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=False)
    return Predictor(settings, net), Dataset(data, cm)


def leg_a(pred, ds, out_dir, level):
    t0 = time.perf_counter()
    for d in ds.data:
        pred.write_masks(d, out_dir, level=level)
    return (time.perf_counter() - t0) * 1e3 / len(ds.data)


def leg_b(pred, ds, out_dir, level, **kw):
    t0 = time.perf_counter()
    n = sum(1 for _ in pred.write_masks_dataset(ds, out_dir, level=level, **kw))
    assert n == len(ds.data)
    return (time.perf_counter() - t0) * 1e3 / len(ds.data)


def run_mixed(args):
    """Legs A (write_masks loop), B (write_masks_dataset(mixed=False): the same-shape units, one page each on such a book) and C
    (mixed=True), warmed up, alternated."""
    import pseg_amd
    from pseg_amd import engine as E
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    shapes = mixed_shapes(args.pages)
    pred, ds = make_predictor_and_pages(args.pages, 0, 0, shapes)
    import inspect
    has_mixed = "mixed" in inspect.signature(pred.write_masks_dataset).parameters      # (--leg B runs on older checkouts too)
    legs = {"A": leg_a, "B": (lambda *a: leg_b(*a, mixed=False)) if has_mixed else leg_b, "C": lambda *a: leg_b(*a, mixed=True)}
    if args.leg != "both":
        legs = {args.leg: legs[args.leg]}
    base = tempfile.mkdtemp(prefix="chain_mixed_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    units = E.chain_units_mixed(shapes, cap=8)[1] if has_mixed else []
    canvases = sorted({(-(-h // 32) * 32, -(-w // 32) * 32) for h, w in shapes})
    lines = ["# %d pages, shapes within +-5 %% of 842x595 (%d distinct, %d canvases: %s), fcn_skip 3 classes, bf16, cc_majority, files into %s"
             % (args.pages, len(set(shapes)), len(canvases), " ".join("%dx%d" % c for c in canvases), os.path.dirname(base) or "tmp"),
             "# ms per page, host wall clock; leg A: loop of write_masks; B: write_masks_dataset(mixed=False), %d units; C: mixed=True, "
             "%d units at cap 8 (the call's own cap may be lower); %d alternations"
             % (len(E.chain_units(shapes, cap=8)), len(units), args.alternations)]
    try:
        for level in args.levels:
            dirs = {k: os.path.join(base, "l%d_%s" % (level, k)) for k in legs}
            for k in legs:
                legs[k](pred, ds, dirs[k], level)
            assert all(same_files(dirs[k], dirs[j]) for k in legs for j in legs), "the legs' files differ"
            times = {k: [] for k in legs}
            for _ in range(args.alternations):
                for k in legs:
                    times[k].append(legs[k](pred, ds, dirs[k], level))
            for k in legs:
                t = times[k]
                lines.append("level %d leg %s: median %.3f ms/page, range %.3f .. %.3f, runs %s"
                             % (level, k, statistics.median(t), min(t), max(t), " ".join("%.3f" % v for v in t)))
            if len(legs) < 3:
                continue
            spread_b = max(times["B"]) - min(times["B"])
            wins = sum(b - c > spread_b for b, c in zip(times["B"], times["C"]))
            lines.append("level %d: C / B = %.3f, C / A = %.3f (medians); spread of B %.3f ms; C below B by more than that in %d of %d "
                         "alternations; files byte-equal"
                         % (level, statistics.median(times["C"]) / statistics.median(times["B"]),
                            statistics.median(times["C"]) / statistics.median(times["A"]), spread_b, wins, args.alternations))
    finally:
        shutil.rmtree(base, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


def mixed_kernel_run(args):
    """8 pages of 8 shapes on one canvas: mixed=True at unit_cap 8 encodes them in ragged launches (the list's ramps: units of 1, 2, 4
    and 1 pages), mixed=False page by page.  Nothing timed: for `rocprofv3 --kernel-trace --stats`."""
    import pseg_amd
    from pseg_amd import synth
    assert pseg_amd.device_count() > 0, "needs a HIP device"
    eng = pseg_amd.Engine("fcn_skip", 3, mode=pseg_amd.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    shapes = [(835 + 3 * k, 580 + 3 * k) for k in range(8)]          # one canvas: 864 x 608
    pages = [synth.synth_page(k, s[0], s[1], 3) for k, s in enumerate(shapes)]
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    for _ in range(3):
        for level in args.levels:
            for mixed in (False, True):
                eng.predict_chain_pages([p[0] for p in pages], binaries=[p[1] for p in pages], post_ops=["cc_vote"], lut=lut,
                                        png_level=level, unit_cap=8, mixed=mixed, sink=lambda page, name, data: None)
    eng.close()


def mixed_kernel_table(args):
    """Band-kernel time per page: the ragged launches (third template argument 2) against the single-image launches (0) of the same
    8 pages, summed per round of --mixed-kernel-run (3 rounds), from the kernel trace."""
    tot, cnt = {}, {}
    for path in args.mixed_kernel_table:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                m = re.search(r"png_band_kernel<[^,>]+,\s*(\d),\s*(\d)\s*>", r.get("Kernel_Name", ""))
                if not m:
                    continue
                key = (int(m.group(1)), int(m.group(2)))
                tot[key] = tot.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                cnt[key] = cnt.get(key, 0) + 1
    lines = ["# png_band_kernel over 8 pages of 8 shapes (one canvas), 3 rounds, from a kernel trace of --mixed-kernel-run; us",
             "# level  mode (0 single-image launches, 2 ragged)  launches  total  per page"]
    for key in sorted(tot):
        lines.append("  %d      %d   %5d   %10.1f   %8.2f" % (key[0], key[1], cnt[key], tot[key], tot[key] / 24))
    for level in sorted({k[0] for k in tot}):
        if (level, 0) in tot and (level, 2) in tot:
            lines.append("level %d: ragged / single = %.3f" % (level, tot[(level, 2)] / tot[(level, 0)]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


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
    ap.add_argument("--pages", type=int, default=None, help="default 32 (64 with --mixed)")
    ap.add_argument("--height", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--leg", choices=["both", "A", "B", "C"], default="both")
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-table", nargs="+", metavar="CSV")
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--mixed-kernel-run", action="store_true")
    ap.add_argument("--mixed-kernel-table", nargs="+", metavar="CSV")
    ap.add_argument("--out", default=None, help="report file (default for the two-leg run: profiles/chain_pages.txt)")
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if args.pages is None:
        args.pages = 64 if args.mixed else 32
    if args.mixed_kernel_table:
        return mixed_kernel_table(args)
    if args.mixed_kernel_run:
        return mixed_kernel_run(args)
    if args.mixed:
        if args.out is None and args.leg == "both":
            args.out = os.path.join(ROOT, "profiles", "chain_mixed.txt")
        return run_mixed(args)
    if args.kernel_table:
        return kernel_table(args)
    if args.kernel_run:
        return kernel_run(args)
    if args.out is None and args.leg == "both":
        args.out = os.path.join(ROOT, "profiles", "chain_pages.txt")
    return run_legs(args)


if __name__ == "__main__":
    main()
