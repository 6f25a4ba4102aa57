"""Dataset records and the dataset-JSON loader (reference: lib/dataset.py).

SingleData / Dataset keep the reference's field names and order (lib/dataset.py:17-41) because
callers build them positionally and from the dataset JSON ({"train": [...], "test": [...],
"eval": [...]} of {binary_path, image_path, mask_path, line_height_px}, README.md:46-70).
Records stay picklable: no GPU handles live in them.
"""
import json
import logging
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple

import numpy as np

from .colors import ColorMap

_log = logging.getLogger(__name__)


@dataclass
class SingleData:
    image: np.ndarray = None
    binary: Optional[np.ndarray] = None
    orig_binary: Optional[np.ndarray] = None
    mask: np.ndarray = None
    image_path: Optional[str] = None
    binary_path: Optional[str] = None
    mask_path: Optional[str] = None
    line_height_px: Optional[int] = 1
    original_shape: Tuple[int, int] = None
    output_path: Optional[str] = None
    user_data: Any = None


@dataclass
class Dataset:
    data: List[SingleData]
    color_map: ColorMap

    def __len__(self):
        return len(self.data)

    def __iter__(self):
        return iter(self.data)


def scale_binary(binary, scale):
    """lib/dataset.py:114-119: skimage rescale(order=0, no anti-aliasing): output shape =
    np.round(shape * scale), nearest gather on the GPU; float64 result."""
    from pseg_amd import engine as _eng
    from .util import preserving_resize
    binary = np.asarray(binary)
    return preserving_resize(binary, _eng.rescale_shape(binary.shape, scale))


def scale_image(img, target_shape):
    """lib/dataset.py:122-128: bicubic resize, Gaussian anti-aliasing when the image has more
    than two distinct values (GPU: pseg_scale_image); float64 result."""
    from pseg_amd import engine as _eng
    return _eng.scale_image(np.asarray(img), target_shape)


def prepare_images(image, binary, target_line_height, line_height_px, max_width=None, keep_orig_bin=False):
    """lib/dataset.py:131-150.  image: gray uint8 scan (ink dark); binary: 0/255 or 0/1 with
    paper = 1 (ink = 0).  Returns the inverted network input (ink bright), ink = 1 binary.  One
    GPU call (pseg_prepare_images) does the whole chain: nearest rescale of the binary, Gaussian
    anti-aliasing + bicubic resize of the image, optional max_width stage, inversion, uint8."""
    from pseg_amd import engine as _eng
    scale = target_line_height / line_height_px
    img, bin_, orig = _eng.prepare_images(image, binary, scale, max_width)
    if keep_orig_bin:
        return img, bin_, orig
    return img, bin_


def _imread_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def _imread_bin(path):
    """ocr4all.files.imread_bin(path, True) stand-in: gray read, > 127 -> 255 else 0."""
    g = _imread_gray(path)
    return np.where(g > 127, 255, 0).astype(np.uint8)


def _imread_scan(path):
    """_imread_gray as the contiguous uint8 array the list entries take (load_data_list's pool threads)."""
    return np.ascontiguousarray(_imread_gray(path), dtype=np.uint8)


def _imread_rgb(path):
    """A mask file as ColorMap.imread_labels reads it, before the lookup: (H,W,3) uint8 (RGB, palette and RGBA files alike)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB")), dtype=np.uint8)


def check_binarize(binarize):
    """binarize=None (the reference's > 127) or a pseg_amd.Sauvola; anything else raises."""
    from pseg_amd import engine as _eng
    if binarize is not None and not isinstance(binarize, _eng.Sauvola):
        raise Exception(f"binarize must be None or a pseg_amd.Sauvola, got {binarize!r}")
    return binarize


def _binarize_gray(gray, binarize, line_height_px):
    """The 0 / 255 map (paper = 255) of a gray scan under an adaptive threshold: where(ink, 0, 255) of pseg_amd.binarize_scans, a
    window=None resolved from the entry's line height."""
    from pseg_amd import engine as _eng
    ink = _eng.binarize_scans([gray], binarize.resolved(line_height_px))[0]
    return np.where(ink != 0, 0, 255).astype(np.uint8)


def check_despeckle(despeckle):
    """despeckle=None (the ink map as the threshold leaves it) or a pseg_amd.Despeckle; anything else raises."""
    from pseg_amd import engine as _eng
    if despeckle is not None and not isinstance(despeckle, _eng.Despeckle):
        raise Exception(f"despeckle must be None or a pseg_amd.Despeckle, got {despeckle!r}")
    return despeckle


def _despeckle_binary(bin_, despeckle, line_height_px):
    """A 0 / 255 map (paper = 255) without its specks: where(clean, 0, 255) of pseg_amd.despeckle_maps of the one ink map, a
    max_area=None resolved from the entry's line height."""
    from pseg_amd import engine as _eng
    clean = _eng.despeckle_maps([bin_ == 0], despeckle.resolved(line_height_px))[0]
    return np.where(clean != 0, 0, 255).astype(np.uint8)


def check_deskew(deskew):
    """deskew=None (the scan as it is) or a pseg_amd.Skew; anything else raises."""
    from pseg_amd import engine as _eng
    if deskew is not None and not isinstance(deskew, _eng.Skew):
        raise Exception(f"deskew must be None or a pseg_amd.Skew, got {deskew!r}")
    return deskew


def check_on_skew(deskew, on_skew):
    if on_skew is not None and (deskew is None or not callable(on_skew)):
        raise Exception("on_skew must be a callable and goes with a deskew")
    return on_skew


class DatasetLoader:
    def __init__(self, target_line_height, color_map: ColorMap, prediction=False, max_width=None, binarize=None, despeckle=None,
                 deskew=None, on_skew=None):
        self.target_line_height = target_line_height
        self.prediction = prediction
        self.color_map = color_map
        self.max_width = max_width
        self.binarize = check_binarize(binarize)    # None: > 127 (imread_bin); a pseg_amd.Sauvola: the adaptive ink map on the device
        self.despeckle = check_despeckle(despeckle)  # None, or a pseg_amd.Despeckle: the ink map derived from the scan loses its specks
        self.deskew = check_deskew(deskew)          # None, or a pseg_amd.Skew: the scan read from image_path is deskewed first, the mask with it
        self.on_skew = check_on_skew(deskew, on_skew)   # on_skew(entry, index, denom) for every entry that was deskewed

    def load_images(self, entry: SingleData) -> SingleData:
        """lib/dataset.py:160-191.  The reference derives the binary from the *image* attribute /
        path (attr 'image', :172) and never reads binary_path; kept.  With a binarize, the adaptive map of the gray scan takes
        _imread_bin's place: the records carry the ink map the scan chain works on.  With a despeckle, the ink map derived from the
        scan's file (either way) loses its specks first; a pre-loaded entry.image, which is its own binary, is left as it is.
        With a deskew, the gray scan read from image_path goes through pseg_amd.deskew_scans first (the skew estimated on
        scan <= 127, the scan rotated by it, order 1, fill 255); the ink map is then derived from the deskewed scan exactly as
        without (> 127, or binarize, then despeckle), and outside prediction the mask is rotated by the same index (order 0, fill 0:
        the background id) before it is resized.  Page, ink map and mask are in the deskewed frame; original_shape is the scan's,
        which the rotation keeps.  on_skew(entry, index, denom) is called where given.  A pre-loaded entry.image is not deskewed."""
        return self._load_images(entry, self.binarize, getattr(self, "despeckle", None), getattr(self, "deskew", None), getattr(self, "on_skew", None))

    def _load_images(self, entry: SingleData, binarize, despeckle=None, deskew=None, on_skew=None) -> SingleData:
        img = entry.image if entry.image is not None else _imread_gray(entry.image_path)
        original_shape = img.shape
        skew_index = None
        if deskew is not None and entry.image is None:
            from pseg_amd import engine as _eng
            (img,), idx = _eng.deskew_scans([img], deskew)
            skew_index = int(idx[0])
            if on_skew is not None:
                on_skew(entry, skew_index, deskew.denom)
        if entry.image is not None:
            bin_ = entry.image
        elif binarize is not None:
            bin_ = _binarize_gray(img, binarize, entry.line_height_px)
        elif skew_index is not None:
            bin_ = np.where(img > 127, 255, 0).astype(np.uint8)        # _imread_bin's rule on the deskewed scan
        else:
            bin_ = _imread_bin(entry.image_path)
        if despeckle is not None and entry.image is None:
            bin_ = _despeckle_binary(bin_, despeckle, entry.line_height_px)
        img, bin_, orig_bin = prepare_images(img, bin_, self.target_line_height, entry.line_height_px,
                                             self.max_width, keep_orig_bin=True)
        if not self.prediction:
            from .util import preserving_resize
            mask = entry.mask if entry.mask is not None else self.color_map.imread_labels(entry.mask_path)
            if skew_index is not None:
                from pseg_amd import engine as _eng
                mask = _eng.rotate_maps([np.asarray(mask).astype(np.uint8)], [skew_index], denom=deskew.denom, order=0, fill=0)[0]
            mask = preserving_resize(mask, img.shape)
            assert mask.shape == img.shape
            entry.mask = mask.astype(np.uint8)
        entry.binary = bin_
        entry.orig_binary = orig_bin
        entry.image = img
        entry.original_shape = original_shape
        return entry

    def load_data(self, all_dataset_files) -> Dataset:
        return Dataset([self.load_images(d) for d in all_dataset_files], self.color_map)

    def _list_candidate(self, entry: SingleData):
        """Whether load_data_list may take this entry, as far as that shows before a file is read: the scan comes from image_path
        (a pre-loaded image is its own binary in load_images, a quirk that stays there), and the mask from mask_path or from a
        pre-loaded (H,W) array of uint8 / bool label ids."""
        if entry.image is not None or entry.image_path is None:
            return False
        if self.prediction:
            return True
        if entry.mask is None:
            return entry.mask_path is not None
        m = np.asarray(entry.mask)
        return m.ndim == 2 and m.dtype in (np.uint8, np.bool_)

    def load_data_list(self, entries, chunk=64, decode_threads=2, report=None) -> Dataset:
        """load_data for entries that name their files, as lists on the device: the records of load_data field by field (image,
        binary, orig_binary, mask, original_shape, dtypes included), the entries modified in place as load_images modifies them.
        Per chunk of `chunk` entries: every scan is decoded ONCE (_imread_gray) and every mask file with PIL's convert("RGB"), by
        decode_threads pool threads that work on the next chunk while the device works on this one; ONE engine.prepare_scans call
        gives page, ink map and scan-sized ink map (self.binarize and self.despeckle as in load_images, a window=None or
        max_area=None resolved from the entry's line height); ONE engine.label_masks call turns the decoded masks into label maps of the pages' shapes (skipped under
        self.prediction).  A pre-loaded entry.mask of uint8 / bool ids stays on this route as a 1-channel source.
        An entry whose line_height_px is None is measured in one engine.char_heights call over the chunk's decoded scans and the
        height is stored into the entry (Predictor.write_masks_scans does the same); a scan without a measurable height raises
        naming the file.  Entries this route cannot take go through self.load_images, in place and in order: a pre-loaded
        entry.image, a pre-loaded mask of another kind, an entry without the paths, and a max_width that brings the second stage
        (which shows only once the scan's shape is known).  A file that cannot be decoded raises when its entry is reached; the
        entries in front of it are loaded.
        report: a list that receives one item per entry, {"label_counts": int64[256] pixels per label id, "unknown": int pixels of
        a colour the colour map does not know (they became label 0)}, or None for a fallback or prediction entry.  Every mask with
        unknown > 0 is logged as one warning with its file name and the count.
        With self.deskew set, EVERY entry goes through self.load_images, in place and in order, on purpose: the list entries hand
        scan and mask to the device in one call each, and the rotation of both by one estimated index sits between them only in
        load_images.  The records are load_data's."""
        from concurrent.futures import ThreadPoolExecutor
        from pseg_amd import engine as _eng
        entries = list(entries)
        if getattr(self, "deskew", None) is not None:
            for e in entries:
                self.load_images(e)
                if report is not None:
                    report.append(None)
            return Dataset(entries, self.color_map)
        step = max(1, int(chunk))
        colors, ids = (None, None) if self.prediction else self.color_map.table()

        with ThreadPoolExecutor(max(1, int(decode_threads))) as pool:
            def start(i):
                """Chunk i and the decodes of its candidates, in flight: (scan, mask file or None) per entry, or None."""
                part = entries[i:i + step]
                jobs = []
                for e in part:
                    if not self._list_candidate(e):
                        jobs.append(None)
                        continue
                    from_file = not self.prediction and e.mask is None
                    jobs.append((pool.submit(_imread_scan, e.image_path), pool.submit(_imread_rgb, e.mask_path) if from_file else None))
                return part, jobs

            ahead = start(0) if entries else None
            for i in range(0, len(entries), step):
                part, jobs = ahead
                ahead = start(i + step) if i + step < len(entries) else None
                scans, masks, failed = [None] * len(part), [None] * len(part), None
                for k, job in enumerate(jobs):
                    if job is None:
                        continue
                    try:
                        scans[k] = job[0].result()
                        masks[k] = job[1].result() if job[1] is not None else None
                    except BaseException as exc:
                        scans[k], failed = None, (k, exc)
                        break
                stop = len(part) if failed is None else failed[0]
                # the entries without a line height: one device call over the chunk's decoded scans
                unmeasured = [k for k in range(stop) if scans[k] is not None and part[k].line_height_px is None]
                if unmeasured:
                    for k, h in zip(unmeasured, _eng.char_heights([scans[k] for k in unmeasured], inverse=False)[0]):
                        if h is None:
                            if failed is None or k < failed[0]:
                                failed = (k, Exception(f"No line height could be measured in {part[k].image_path}"))
                        else:
                            part[k].line_height_px = h
                    stop = len(part) if failed is None else failed[0]
                on_device = []
                for k in range(stop):
                    if scans[k] is None:
                        continue
                    scale = self.target_line_height / part[k].line_height_px
                    # (the max_width stage shows only once the scan's shape is known)
                    if self.max_width is None or self.max_width / _eng.rescale_shape(scans[k].shape, scale)[1] >= 1.0:
                        on_device.append((k, scale))
                loaded = {}
                if on_device:
                    # (the keyword goes only with a binarisation, as in write_masks_scans)
                    how = {} if self.binarize is None else {"binarize": [self.binarize.resolved(part[k].line_height_px) for k, _ in on_device]}
                    if getattr(self, "despeckle", None) is not None:
                        how["despeckle"] = [self.despeckle.resolved(part[k].line_height_px) for k, _ in on_device]
                    pages = _eng.prepare_scans([scans[k] for k, _ in on_device], [sc for _, sc in on_device], **how)
                    labels = [None] * len(on_device)
                    if not self.prediction:
                        src = [masks[k] if masks[k] is not None else np.ascontiguousarray(part[k].mask).view(np.uint8) for k, _ in on_device]
                        labels = _eng.label_masks(src, [p[0].shape for p in pages], colors, ids, counts=True)
                    loaded = {k: (page, lab) for (k, _), page, lab in zip(on_device, pages, labels)}
                for k in range(stop):
                    entry = part[k]
                    if k not in loaded:
                        self.load_images(entry)
                        if report is not None:
                            report.append(None)
                        continue
                    (img, bin_, orig_bin), lab = loaded[k]
                    item = None
                    if lab is not None:
                        entry.mask, counts = lab
                        item = {"label_counts": counts[:256].copy(), "unknown": int(counts[256])}
                        if item["unknown"] > 0:
                            _log.warning("%s: %d pixels of a colour the colour map does not know became label 0", entry.mask_path, item["unknown"])
                    entry.binary = bin_
                    entry.orig_binary = orig_bin
                    entry.image = img
                    entry.original_shape = scans[k].shape
                    if report is not None:
                        report.append(item)
                if failed is not None:
                    raise failed[1]
        return Dataset(entries, self.color_map)

    def load_data_from_json(self, files, type, as_list=False) -> Dataset:
        """lib/dataset.py:200-208.  as_list=True: the entries go through load_data_list."""
        entries = []
        for f in files:
            with open(f, 'r') as fh:
                js = json.load(fh)
            kinds = ["train", "test", "eval"] if type == "all" else [type]
            for t in kinds:
                entries += [SingleData(**d) for d in js[t]]
        print(f"Loading {len(entries)} data of type {type}")
        return self.load_data_list(entries) if as_list else self.load_data(entries)
