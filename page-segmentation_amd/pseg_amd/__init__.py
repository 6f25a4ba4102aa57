"""pseg_amd -- ctypes binding of libpseg.so (MI355X / gfx950 engine) plus build and
synthetic-data helpers.  The drop-in mirror of the reference API lives next to this package
in `ocr4all_pixel_classifier/`."""
from .engine import (  # noqa: F401
    Engine, PsegError, lib, lib_path, device_count, cc_vote, bbox_fill, masks, otsu_char_height, char_heights,
    ARCH_IDS, MODE_F32_EXACT, MODE_BF16, EXPORTED_SYMBOLS, eval_confusion, cc_label, cc_tables, eval_pages, eval_page_groups, eval_rule, pinned_empty, pinned_empty_pooled, pinned_copy,
    png_encode, masks_png, png_bound, png_code_lengths, tile_plan, plan_arena,
    png_probe, png_decode_gray, PNG_OK, PNG_EINVAL, PNG_EUNSUPPORTED,
    Sauvola, sauvola_window, binarize_scans,
    label_masks, label_masks_geometry, label_mask_groups,
    Despeckle, despeckle_area, despeckle_maps, despeckle_geometry,
    Skew, skew_degrees, skew_maps, rotate_maps, deskew_scans, skew_geometry,
    TextRegions, region_kernels, text_regions, trace_regions, regions_geometry,
)
from .build import build_library  # noqa: F401
