"""compute_char_height (reference: lib/image_ops.py:58-82) on the GPU: Otsu histogram,
binarise, union-find CCL, bounding boxes; the glyph filter and the upper median run on the host
over the component list.  compute_char_heights is its list form: one device-resident call per
chunk of files, the heights binned on the device."""
import os

import numpy as np

from pseg_amd import engine


def compute_char_height(file_name: str, inverse: bool):
    if not os.path.exists(file_name):
        raise Exception(f"File does not exist at {file_name}")
    from PIL import Image
    gray = np.asarray(Image.open(file_name).convert("L"))
    height, _ = engine.otsu_char_height(gray, inverse)
    return height


def compute_char_heights(file_names, inverse: bool, decode_threads=2, chunk_files=64, decode="host"):
    """compute_char_height for a list of files: the same heights (None where no component qualifies), the files decoded on
    decode_threads threads chunk_files at a time and every chunk measured in ONE device call (engine.char_heights: no label
    image, no component list, one wait per group of scans).  While the device call of one chunk runs, the next chunk is being
    decoded.  A missing file raises compute_char_height's exception before anything is decoded.
    decode="device": the pool threads only read the files' bytes and one pool task per chunk decodes them on the device
    (engine.png_decode_gray: 8-bit gray and RGB PNG files; every other file, and every file the decoder refuses, is read with PIL as
    under "host", so the heights -- and the exception for a file PIL cannot read -- are the same)."""
    if decode not in ("host", "device"):
        raise Exception(f"decode must be 'host' or 'device', got {decode!r}")
    from concurrent.futures import ThreadPoolExecutor
    file_names = list(file_names)
    for file_name in file_names:
        if not os.path.exists(file_name):
            raise Exception(f"File does not exist at {file_name}")
    from PIL import Image

    def decode_file(file_name):
        return np.ascontiguousarray(Image.open(file_name).convert("L"), dtype=np.uint8)

    step, out = max(1, int(chunk_files)), []
    with ThreadPoolExecutor(max(1, int(decode_threads))) as pool:
        if decode == "device":
            def chunk_task(names, reads):
                got = engine.decode_gray_files(names, fallback=decode_file, reads=reads)
                for g in got:
                    if isinstance(g, BaseException):
                        raise g
                return got
            start = lambda i: pool.submit(chunk_task, file_names[i:i + step], [pool.submit(engine.read_file_bytes, f) for f in file_names[i:i + step]])
        else:
            start = lambda i: [pool.submit(decode_file, f) for f in file_names[i:i + step]]
        ahead = start(0) if file_names else None
        for i in range(0, len(file_names), step):
            pending = ahead
            scans = pending.result() if decode == "device" else [fut.result() for fut in pending]
            ahead = start(i + step) if i + step < len(file_names) else None
            out += engine.char_heights(scans, inverse)[0]
    return out


def _fg_counts(pred, mask, bin, n_classes):
    """counts[b][m][p] from the GPU (pseg_eval_confusion); labels outside [0, n_classes) land in the last slot."""
    return engine.eval_confusion(pred, mask, bin, n_classes)


def fgpa(pred: np.ndarray, mask: np.ndarray, bin: np.ndarray):
    """Foreground pixel accuracy (lib/image_ops.py:8-19): pred*bin != mask*bin happens exactly on the ink pixels
    whose labels differ, so the joint histogram's ink plane gives both counts."""
    pred, mask = np.asarray(pred), np.asarray(mask)
    top = int(max(pred.max(initial=0), mask.max(initial=0))) + 1
    if pred.min(initial=0) < 0 or mask.min(initial=0) < 0 or top > 255:
        raise Exception("fgpa: labels must lie in 0..254")
    return fgpa_from_counts(_fg_counts(pred, mask, bin, top))


def fgpa_from_counts(counts):
    """fgpa from the joint histogram counts[b][m][p] (shared with evaluation.PageScore)."""
    c = np.asarray(counts)[1]
    fg_count = int(c.sum())
    wrong = fg_count - int(np.trace(c))
    return (fg_count - wrong) / fg_count                      # ZeroDivisionError on a page without ink, as the reference


def fgoverlap_per_class(pred: np.ndarray, mask: np.ndarray, bin: np.ndarray, n_classes: int):
    """Per-class foreground overlap (lib/image_ops.py:22-55): index i for class i, i = 0..n_classes (the
    reference's range(n_classes + 1)); (overlaps, tps, fps, fns).  bin must be 0/1 as the reference documents:
    (label + 1) * bin - 1 is the label on ink and -1 (no class) on paper."""
    bin = np.asarray(bin)
    if bin.size and bin.max() > 1:
        raise Exception("fgoverlap_per_class: bin must be 0/1 (1 is foreground)")
    k = int(n_classes) + 1                                    # classes 0..n_classes are reported
    return fgoverlap_from_counts(_fg_counts(pred, mask, bin, k), n_classes)


def fgoverlap_from_counts(counts, n_classes: int):
    """fgoverlap_per_class from the joint histogram counts[b][m][p] (shared with evaluation.PageScore).  The table may have
    more or fewer class slots than n_classes + 1: a class it has no slot for has no pixels, its last slot collects the labels
    beyond its range, and a row / column sum runs over every slot either way."""
    k = int(n_classes) + 1
    c_full = np.asarray(counts)[1]                             # ink plane, [mask][pred]; last slot = other labels
    overlaps, tps, fps, fns = [], [], [], []
    for i in range(k):
        if i >= c_full.shape[0]:
            overlaps.append(np.nan); tps.append(0); fps.append(0); fns.append(0)
            continue
        tp = int(c_full[i, i])
        fp = int(c_full[:, i].sum()) - tp                      # predicted i, expected something else
        fn = int(c_full[i, :].sum()) - tp
        if tp + fp + fn == 0:
            overlaps.append(np.nan); tps.append(0); fps.append(0); fns.append(0)
        else:
            overlaps.append(tp / (tp + fp + fn)); tps.append(tp); fps.append(fp); fns.append(fn)
    return overlaps, tps, fps, fns
