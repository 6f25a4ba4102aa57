#!/usr/bin/env python
"""Tiled prediction (pseg_predict_tiled_device) against the whole page, and the page the bf16 engine refuses whole.

  python tools/bench_tiled.py                          all runs, report to profiles/tiled.txt
  python tools/bench_tiled.py --child sizes|refused    one process of one leg (what the driver starts; prints JSON lines)
  python tools/bench_tiled.py --kernel-run             one tiled page per size, 3 rounds, nothing timed: run it under
                                                       `rocprofv3 --kernel-trace --stats` (a run of its own)
  python tools/bench_tiled.py --kernel-count DIR       the cut and stitch kernels' own time from that run's *kernel_stats.csv
  python tools/bench_tiled.py --parent DIR             adds the bench.py headline of this tree against a built checkout of the
                                                       parent commit in DIR (alternating, one process per run)

Legs.  sizes: bf16 fcn_skip with 6 classes at 4096x3072 and bf16 unet with 3 at 2048x1536, device-resident page in, uint8 label map
out, the whole page (pseg_predict_device) against tiles of 1024 / 2048 / 4096 -- ms per page next to the compute ratio the plan
predicts, n_tiles * t_h * t_w / (Hp * Wp).  refused: the 8192x8200 page of tests/test_tiles_gpu.py in tiles of 1024 and 2048, ms per
page and the device memory the process holds afterwards (the engine's buffers only grow: its peak).  Three alternations, each leg a
process of its own that warms up before it measures.  Times are host wall clock around a batch of calls and one wait."""
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
for _p in (ROOT, os.path.join(ROOT, "page-segmentation_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

SIZES = [("fcn_skip", 6, (4096, 3072)), ("unet", 3, (2048, 1536))]
TILES = (1024, 2048, 4096)
REFUSED = (8192, 8200)


def _engine(arch, n_classes):
    import pseg_amd
    from pseg_amd import synth
    eng = pseg_amd.Engine(arch, n_classes, mode=pseg_amd.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return eng


def _ratio(arch, shape, tile):
    from pseg_amd import engine as E
    (th, tw), org, _ = E.tile_plan(arch, shape, tile)
    Hp, Wp = (shape[0] + 31) // 32 * 32, (shape[1] + 31) // 32 * 32
    return len(org), len(org) * th * tw / float(Hp * Wp)


def _time(eng, call, reps):
    call()
    eng.status()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    eng.status()
    return (time.perf_counter() - t0) * 1e3 / reps


def child_sizes(args):
    import torch
    from pseg_amd import synth
    assert torch.cuda.is_available(), "needs a HIP device"
    for arch, C, (H, W) in SIZES:
        eng = _engine(arch, C)
        d_img = torch.from_numpy(synth.synth_page(1000, H, W, C)[0]).cuda()
        d_lab, d_ref = torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty((H, W), dtype=torch.uint8, device="cuda")
        ms = _time(eng, lambda: eng.predict_device(d_img.data_ptr(), H, W, d_labels_u8=d_ref.data_ptr()), args.reps)
        print(json.dumps({"leg": "sizes", "arch": arch, "shape": [H, W], "tile": 0, "ms": ms, "tiles": 1, "ratio": 1.0}), flush=True)
        for tile in TILES:
            n, ratio = _ratio(arch, (H, W), tile)
            ms = _time(eng, lambda: eng.predict_tiled_device(d_img.data_ptr(), H, W, tile, d_labels_u8=d_lab.data_ptr()), args.reps)
            torch.cuda.synchronize()
            print(json.dumps({"leg": "sizes", "arch": arch, "shape": [H, W], "tile": tile, "ms": ms, "tiles": n, "ratio": ratio,
                              "equal": bool(torch.equal(d_lab, d_ref))}), flush=True)
        eng.close()


def child_refused(args):
    import torch
    from pseg_amd import synth
    assert torch.cuda.is_available(), "needs a HIP device"
    H, W = REFUSED
    base = synth.synth_page(60, 1024, 1025, 3)[0]
    d_img = torch.from_numpy(np.tile(base, (8, 8))).cuda()
    d_lab = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for tile in (1024, 2048):
        eng = _engine("fcn_skip", 3)
        free0 = torch.cuda.mem_get_info()[0]
        ms = _time(eng, lambda: eng.predict_tiled_device(d_img.data_ptr(), H, W, tile, d_labels_u8=d_lab.data_ptr()), max(1, args.reps // 2))
        held = free0 - torch.cuda.mem_get_info()[0]
        n, ratio = _ratio("fcn_skip", (H, W), tile)
        print(json.dumps({"leg": "refused", "tile": tile, "ms": ms, "tiles": n, "ratio": ratio, "held_MiB": held / 2.0 ** 20}), flush=True)
        eng.close()


def kernel_run(args):
    import torch
    from pseg_amd import synth
    for arch, C, (H, W) in SIZES:
        eng = _engine(arch, C)
        d_img = torch.from_numpy(synth.synth_page(1000, H, W, C)[0]).cuda()
        d_lab = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            eng.predict_tiled_device(d_img.data_ptr(), H, W, 2048, d_labels_u8=d_lab.data_ptr())
        eng.status()
        eng.close()
    print("kernel-run: %d sizes x 3 rounds at tile 2048" % len(SIZES))


def kernel_count(args):
    lines = []
    for path in glob.glob(os.path.join(args.kernel_count, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "tiles_cut_kernel" in r["Name"] or "tiles_stitch_kernel" in r["Name"]:
                    lines.append("  %-24s calls %4d  %9.1f us per call" % (r["Name"].split("(")[0][-24:], int(r["Calls"]),
                                                                           float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"])))
    text = "cut and stitch kernels (kernel trace, tile 2048, the units of both sizes of the sizes leg):\n" + "\n".join(sorted(lines)) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


def _children(leg, args):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(args.reps)], capture_output=True, text=True, timeout=600)
    if run.returncode != 0:
        sys.stderr.write(run.stderr)
        raise SystemExit("leg %s failed with status %d" % (leg, run.returncode))
    return [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith("{")]


def _headline(tree, args):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                         check=True, capture_output=True, text=True, timeout=900, cwd=tree).stdout
    res = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")][-1]
    return res


def drive(args):
    rows = []
    for alt in range(args.alternations):
        for leg in ("sizes", "refused"):
            print("alternation %d, leg %s" % (alt, leg), file=sys.stderr, flush=True)
            rows += [dict(r, alternation=alt) for r in _children(leg, args)]
    lines = ["# tools/bench_tiled.py: bf16 engines, device-resident page in, uint8 label map out, ms per page (host wall clock, %d calls and one wait);"
             % args.reps, "# %d alternations, one process per leg and alternation; ratio = n_tiles * t_h * t_w / (Hp * Wp), the compute the plan predicts" % args.alternations]
    for arch, C, (H, W) in SIZES:
        sel = lambda tile: [r for r in rows if r["leg"] == "sizes" and r["arch"] == arch and r["tile"] == tile]
        whole = statistics.median(r["ms"] for r in sel(0))
        lines.append("%s %d classes %dx%d whole page: median %.3f ms, runs %s" % (arch, C, H, W, whole, " ".join("%.3f" % r["ms"] for r in sel(0))))
        for tile in TILES:
            s = sel(tile)
            med = statistics.median(r["ms"] for r in s)
            lines.append("%s %dx%d tile %4d: %2d tiles, ratio %.3f, median %.3f ms (%.3f x whole), runs %s, equal to the whole page: %s"
                         % (arch, H, W, tile, s[0]["tiles"], s[0]["ratio"], med, med / whole, " ".join("%.3f" % r["ms"] for r in s),
                            all(r["equal"] for r in s)))
    for tile in (1024, 2048):
        s = [r for r in rows if r["leg"] == "refused" and r["tile"] == tile]
        lines.append("fcn_skip 3 classes %dx%d (refused whole) tile %4d: %3d tiles, ratio %.3f, median %.3f ms, runs %s; device memory held %.0f MiB"
                     % (REFUSED[0], REFUSED[1], tile, s[0]["tiles"], s[0]["ratio"], statistics.median(r["ms"] for r in s),
                        " ".join("%.3f" % r["ms"] for r in s), max(r["held_MiB"] for r in s)))
    if args.parent:
        heads = {"this": [], "parent": []}
        for alt in range(args.alternations):
            for name, tree in (("parent", args.parent), ("this", ROOT)):
                heads[name].append(_headline(tree, args))
        key = args.headline_key
        for name in ("parent", "this"):
            lines.append("bench.py headline (%s), %s tree: %s" % (key, name, " ".join("%.4g" % float(h[key]) for h in heads[name])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", choices=["sizes", "refused"])
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-count", metavar="DIR")
    ap.add_argument("--parent", metavar="DIR", help="a built checkout of the parent commit: bench.py's headline there and here")
    ap.add_argument("--headline-key", default="value")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="report file (default for the driver: profiles/tiled.txt)")
    args = ap.parse_args()
    if args.child:
        return child_sizes(args) if args.child == "sizes" else child_refused(args)
    if args.kernel_run:
        return kernel_run(args)
    if args.kernel_count:
        return kernel_count(args)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "tiled.txt")
    return drive(args)


if __name__ == "__main__":
    main()
