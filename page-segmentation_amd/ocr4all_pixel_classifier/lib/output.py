"""Mask generation and output (reference: lib/output.py)."""
import os
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

from pseg_amd import engine

from .colors import ColorMap
from .dataset import SingleData


@dataclass
class Masks:
    color: np.ndarray
    overlay: np.ndarray
    inverted_overlay: np.ndarray
    fg_color_mask: Optional[np.ndarray] = None


def generate_output_masks(data: SingleData, pred: np.ndarray, color_map: ColorMap) -> Masks:
    """lib/output.py:44-60 as one streaming GPU kernel (pseg_masks)."""
    color, overlay, inverted, fg = engine.masks(pred, np.asarray(data.binary).astype(np.uint8), color_map.lut())
    return Masks(color=color, overlay=overlay, inverted_overlay=inverted, fg_color_mask=fg)


#: write ".png" targets with the device encoder (pseg_masks_png); False: PIL writes every file, as the reference does
DEVICE_PNG = True
#: the device encoder's level: 0 = fixed Huffman codes, 1 = a dynamic code per band (smaller files, a second pass on the device)
DEVICE_PNG_LEVEL = 0


def output_paths(output_dir, data: SingleData):
    """The three files output_data writes for this page (lib/output.py:20-38), their directories created:
    (color, overlay, inverted)."""
    if data.output_path:
        filename = data.output_path
        d = os.path.dirname(filename)
        if os.path.isabs(d):
            os.makedirs(d, exist_ok=True)
        elif d:
            for category in ("color", "overlay", "inverted"):
                os.makedirs(os.path.join(output_dir, category, d), exist_ok=True)
    else:
        filename = os.path.basename(data.image_path)
    return tuple(os.path.join(output_dir, category, filename) for category in ("color", "overlay", "inverted"))


def is_png_target(path):
    """PIL picks the file format from the extension; the device encoder writes PNG only."""
    return str(path).lower().endswith(".png")


def write_png_streams(paths, streams):
    for path, stream in zip(paths, streams):
        with open(path, "wb") as f:
            f.write(stream)


def output_data(output_dir, pred, data: SingleData, color_map, level=None):
    """lib/output.py:20-41.  A ".png" target (any letter case) is encoded on the device straight from the label map
    (engine.masks_png: the RGB masks never exist); every other extension, and DEVICE_PNG = False, goes through PIL.
    level: the device encoder's; None: DEVICE_PNG_LEVEL."""
    if pred.ndim == 3:
        assert pred.shape[0] == 1
        pred = pred[0]
    paths = output_paths(output_dir, data)
    if DEVICE_PNG and is_png_target(paths[0]):
        png = engine.masks_png(pred, np.asarray(data.binary).astype(np.uint8), color_map.lut(),
                               level=DEVICE_PNG_LEVEL if level is None else level)
        write_png_streams(paths, (png["color"], png["overlay"], png["inverted"]))
        return
    from PIL import Image
    masks = generate_output_masks(data, pred, color_map)
    Image.fromarray(masks.color).save(paths[0])
    Image.fromarray(masks.overlay).save(paths[1])
    Image.fromarray(masks.inverted_overlay).save(paths[2])


def scale_to_original_shape(data: SingleData, pred):
    """lib/output.py:63-79."""
    from .util import preserving_resize
    resized_image = preserving_resize(data.image, data.original_shape)
    pred = preserving_resize(pred, data.original_shape).astype('int64')
    if data.binary.shape != tuple(data.original_shape):
        if data.orig_binary is not None:
            resized_binary = data.orig_binary
        else:
            resized_binary = preserving_resize(data.binary, data.original_shape).astype('bool')
    else:
        resized_binary = data.binary
    return replace(data, binary=resized_binary, image=resized_image), pred
