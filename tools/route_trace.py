"""Which kernels a bf16 predict launches: one predict per case, random weights, no plan switches -- the cases that reach every route of
mfma_launch_conv (conv_sp_kernel on both tile widths, conv_sp2_kernel's default choice, conv_pp_kernel, conv12_ws_kernel, the persistent
and the plain conv_mfma_kernel instances, the layer-major page launches).  Run it under a kernel trace, once per library, and compare the
two lists of (kernel name with template arguments, calls); PSEG_LIB selects the library:
    PSEG_LIB=<libpseg.so> rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/route_trace.py
    python tools/route_trace.py --summary <dir>         # the (calls, name) list of that run"""
import csv, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SINGLE = [("fcn_skip", 3, 160, 224), ("fcn_skip", 3, 1024, 768), ("fcn_skip", 3, 2048, 1536), ("fcn_skip", 6, 1024, 768), ("fcn", 3, 2048, 1536),
          ("unet", 3, 160, 224), ("unet", 3, 1120, 1312), ("res_unet", 3, 160, 224), ("res_unet", 3, 1120, 1312)]
PAGES = [("fcn_skip", 3, 2048, 1536, 8), ("res_unet", 3, 1120, 1312, 8)]


def summary(d):
    """(calls, kernel name) of every kernel in the trace files under d, sorted by name."""
    calls = {}
    for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            calls[row["Kernel_Name"]] = calls.get(row["Kernel_Name"], 0) + 1
    print("kernels: %d launches of %d names" % (sum(calls.values()), len(calls)))
    for name in sorted(calls):
        print("%7d  %s" % (calls[name], name))


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "page-segmentation_amd")]
    import numpy as np
    import torch
    torch.cuda.is_available()
    from pseg_amd import engine as E, synth
    st = torch.cuda.current_stream().cuda_stream
    for arch, classes, H, W, pages in [c + (1,) for c in SINGLE] + PAGES:
        eng = E.Engine(arch, classes, mode=E.MODE_BF16)
        eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
        img = torch.from_numpy(np.stack([synth.synth_page(1000 + i, H, W, classes)[0] for i in range(pages)])).cuda()
        lab = torch.empty((pages, H, W), dtype=torch.uint8, device="cuda")
        if pages == 1:
            eng.predict_device(img.data_ptr(), H, W, d_labels_u8=lab.data_ptr(), stream=st)
        else:
            eng.predict_pages_device(img.data_ptr(), pages, H, W, d_labels_u8=lab.data_ptr(), stream=st)
        torch.cuda.synchronize()
        print("%s %d classes %dx%d x %d: labels %s" % (arch, classes, H, W, pages, np.bincount(lab.cpu().numpy().ravel(), minlength=classes).tolist()), flush=True)
        del eng


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        summary(sys.argv[2])
    else:
        run()
