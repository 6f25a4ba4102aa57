"""ctypes binding of include/pseg.h.  No compute happens in Python; there is no CPU fallback:
every call raises PsegError when libpseg.so or a HIP device is missing."""
import ctypes
import os

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")

ARCH_IDS = {"fcn_skip": 0, "fcn": 1, "unet": 2, "res_unet": 3}
MODE_F32_EXACT = 0
MODE_BF16 = 1
FLAG_BATCHNORM = 1

# every symbol include/pseg.h declares (tests check that the library exports each one)
EXPORTED_SYMBOLS = (
    "pseg_abi_version", "pseg_last_error", "pseg_device_count", "pseg_create", "pseg_create_ex", "pseg_create_plan", "pseg_env_knobs", "pseg_destroy",
    "pseg_num_weights", "pseg_weight_info", "pseg_set_weights", "pseg_get_weights",
    "pseg_predict", "pseg_predict_device", "pseg_predict_pages_device", "pseg_engine_status", "pseg_engine_trim", "pseg_plan_arena", "pseg_batch_units", "pseg_rccl_abi_pinned", "pseg_predict_batch", "pseg_predict_chain", "pseg_get_activation", "pseg_flops_per_pixel", "pseg_engine_stream",
    "pseg_host_alloc", "pseg_host_free", "pseg_host_register", "pseg_host_unregister",
    "pseg_predict_margin_device", "pseg_predict_exact_labels_device", "pseg_predict_exact_labels", "pseg_label_exact_stats", "pseg_label_exact_stats_ex",
    "pseg_timing_enable", "pseg_timing_reset", "pseg_timing_num_slots", "pseg_timing_get",
    "pseg_train_init", "pseg_train_set_optimizer", "pseg_train_set_loss", "pseg_train_set_dropout_seed", "pseg_train_forward_backward", "pseg_train_forward_backward_f32",
    "pseg_train_forward_backward_aug", "pseg_train_augment_sample", "pseg_train_grad_buffer", "pseg_train_metrics",
    "pseg_train_apply", "pseg_train_get_gradient", "pseg_train_wgrad_layer", "pseg_eval_step",
    "pseg_allreduce_unique_id", "pseg_allreduce_init", "pseg_train_allreduce", "pseg_allreduce_destroy",
    "pseg_cc_vote", "pseg_cc_vote_device", "pseg_cc_vote_device_u8", "pseg_release_workspace", "pseg_bbox_fill",
    "pseg_masks", "pseg_masks_device", "pseg_masks_device_u8", "pseg_bbox_fill_device_u8",
    "pseg_otsu_char_height", "pseg_char_heights", "pseg_char_height_window", "pseg_char_height_median",
    "pseg_png_probe", "pseg_png_decode_gray", "pseg_png_decode_gray_device", "pseg_png_decode_gray_host",
    "pseg_png_bound", "pseg_png_encode_device", "pseg_masks_png_device_u8", "pseg_png_encode", "pseg_masks_png", "pseg_predict_chain_png",
    "pseg_png_bound_lv", "pseg_png_encode_device_lv", "pseg_masks_png_device_u8_lv", "pseg_png_encode_lv", "pseg_masks_png_lv",
    "pseg_predict_chain_png_lv", "pseg_png_code_lengths", "pseg_predict_chain_pages_png", "pseg_chain_units",
    "pseg_predict_chain_pages_mixed_png", "pseg_chain_units_mixed", "pseg_predict_chain_scans_png", "pseg_prepare_scans",
    "pseg_binarize_scans", "pseg_binarize_scans_host", "pseg_binarize_geometry", "pseg_prepare_scans_bin", "pseg_predict_chain_scans_bin_png",
    "pseg_label_masks", "pseg_label_masks_host", "pseg_label_masks_geometry", "pseg_label_masks_groups",
    "pseg_despeckle_maps", "pseg_despeckle_maps_host", "pseg_despeckle_geometry", "pseg_prepare_scans_clean", "pseg_predict_chain_scans_clean_png",
    "pseg_skew_maps", "pseg_skew_maps_host", "pseg_rotate_maps", "pseg_rotate_maps_host", "pseg_deskew_scans", "pseg_deskew_scans_host", "pseg_skew_geometry",
    "pseg_text_regions", "pseg_text_regions_host", "pseg_regions_geometry", "pseg_trace_regions_host",
    "pseg_text_regions_poly", "pseg_text_regions_poly_host", "pseg_predict_chain_pages_regions_png", "pseg_predict_chain_scans_regions_png",
    "pseg_rescale_shape", "pseg_gaussian_kernel", "pseg_resize_nearest", "pseg_resize_nearest_device", "pseg_scale_image",
    "pseg_prepare_images", "pseg_affine_warp", "pseg_affine_warp_fill", "pseg_brightness_shift",
    "pseg_eval_confusion", "pseg_cc_label", "pseg_cc_tables", "pseg_eval_pages", "pseg_eval_page_groups",
    "pseg_tile_plan", "pseg_predict_tiled_device", "pseg_predict_tiled", "pseg_engine_set_tiling", "pseg_engine_page_fits",
)


PLAN_FROM_ENV = bool(os.environ.get("PSEG_PLAN_FROM_ENV"))   # test harness / tools: PSEG_* of os.environ -> plan switches of new engines (see Engine)


# pseg_chain_sink: int (*)(void* user, int page, int which, const uint8_t* data, size_t n_bytes)
CHAIN_SINK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t)


class SCAN(ctypes.Structure):
    """pseg_scan: one gray scan and the page it becomes (pseg_prepare_scans, pseg_predict_chain_scans_png)."""
    _fields_ = [("gray", ctypes.c_void_p), ("H0", ctypes.c_int), ("W0", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("wy", ctypes.c_void_p), ("ry", ctypes.c_int), ("wx", ctypes.c_void_p), ("rx", ctypes.c_int), ("final_is_scan", ctypes.c_int)]


class BINARIZE(ctypes.Structure):
    """pseg_binarize: how a scan becomes its ink map (window 0: scan <= 127; else Sauvola over an odd window)."""
    _fields_ = [("window", ctypes.c_int), ("k", ctypes.c_double), ("R", ctypes.c_double)]


class DESPECKLE(ctypes.Structure):
    """pseg_despeckle: how an ink map loses its specks (max_area 0: not at all; else components of at most max_area pixels)."""
    _fields_ = [("max_area", ctypes.c_int), ("connectivity", ctypes.c_int)]


class SKEW(ctypes.Structure):
    """pseg_skew: the candidates -steps .. steps of the skew estimate, a slope being index / denom."""
    _fields_ = [("steps", ctypes.c_int), ("denom", ctypes.c_int)]


class ROTATE(ctypes.Structure):
    """pseg_rotate: a rotation by index / denom (order 0: nearest, 1: bilinear; fill: the byte outside the map)."""
    _fields_ = [("index", ctypes.c_int), ("denom", ctypes.c_int), ("order", ctypes.c_int), ("fill", ctypes.c_int)]


class REGIONS(ctypes.Structure):
    """pseg_regions: the label id and the sides of the closing, the opening and the joining rectangle (each 1..255)."""
    _fields_ = [("label", ctypes.c_int), ("k_close", ctypes.c_int), ("k_open", ctypes.c_int), ("k_join", ctypes.c_int)]


class MASK_SRC(ctypes.Structure):
    """pseg_mask_src: one decoded ground-truth mask (channels 3: RGB, 1: label ids)."""
    _fields_ = [("px", ctypes.c_void_p), ("H0", ctypes.c_int), ("W0", ctypes.c_int), ("channels", ctypes.c_int)]


class EVAL_PAGE(ctypes.Structure):
    """pseg_eval_page: one page of pseg_eval_pages."""
    _fields_ = [("pred", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("binary", ctypes.c_void_p), ("H", ctypes.c_int), ("W", ctypes.c_int)]


class EVAL_RULE(ctypes.Structure):
    """pseg_eval_rule: cc_matching (kind 0) or cc_equal (kind 1) with its only_label filter."""
    _fields_ = [("kind", ctypes.c_int), ("label", ctypes.c_int), ("threshold_tp", ctypes.c_double), ("threshold_fp", ctypes.c_double),
                ("threshold_mask", ctypes.c_double), ("filter_label", ctypes.c_int), ("filter_threshold", ctypes.c_double)]


class WGRAD_LAYER(ctypes.Structure):
    """pseg_wgrad_layer: one layer's weight gradient on device tensors (pseg_train_wgrad_layer)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("X", "X1", "dY", "maskY", "dW", "dB")] + [(n, ctypes.c_int32) for n in (
        "mode", "KW", "stride", "xup", "in_relu", "logits", "XC0", "XC1", "ci0", "Cin", "Cout", "Hx", "Wx", "xpitch", "Hy", "Wy",
        "slots", "strip_rows")]


class WGRAD_PLAN(ctypes.Structure):
    """pseg_wgrad_plan: what pseg_train_wgrad_layer launched."""
    _fields_ = [(n, ctypes.c_int32) for n in ("variant", "instance", "ti", "tj", "lds_staged", "strip_rows", "cgroups", "nstrips",
                                              "piece_width", "deterministic")]


WGRAD_VARIANTS = ("PAIR", "FLAT", "BLK", "C1", "KX5", "TAP", "WIDE")   # PSEG_WGRAD_*


class PsegError(Exception):
    """The reference raises bare Exception(...) (lib/dataset.py:67, lib/trainer.py:133)."""


_LIB = None


def lib_path():
    # PSEG_LIB selects another build of the same ABI (e.g. csrc/libpseg_diag.so with trace stamps)
    return os.environ.get("PSEG_LIB") or os.path.join(_CSRC, "libpseg.so")


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise PsegError("libpseg.so is not built (%s); run __graft_entry__.build() -- there is "
                        "no CPU fallback" % path)
    L = ctypes.CDLL(path)
    c = ctypes
    vp, i, i64 = c.c_void_p, c.c_int, c.c_int64
    L.pseg_last_error.restype = c.c_char_p
    L.pseg_create.argtypes = [i, i, i, i, i, c.POINTER(vp)]
    L.pseg_create_ex.argtypes = [i, i, i, i, i, c.c_uint, c.POINTER(vp)]
    L.pseg_create_plan.argtypes = [i, i, i, i, i, c.c_uint, c.c_char_p, c.POINTER(vp)]
    L.pseg_env_knobs.restype = c.c_char_p
    L.pseg_destroy.argtypes = [vp]
    L.pseg_num_weights.argtypes = [vp]
    L.pseg_weight_info.argtypes = [vp, i, c.c_char_p, c.c_size_t, c.POINTER(i64), c.POINTER(i)]
    L.pseg_set_weights.argtypes = [vp, c.c_char_p, vp, c.POINTER(i64), i]
    L.pseg_get_weights.argtypes = [vp, c.c_char_p, vp, i64]
    L.pseg_predict.argtypes = [vp, vp, i, i, vp, vp, vp]
    L.pseg_predict_device.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp]
    L.pseg_predict_pages_device.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    L.pseg_engine_status.argtypes = [vp, vp]
    L.pseg_engine_trim.argtypes = [vp]
    L.pseg_predict_batch.argtypes = [vp, i, vp, vp, vp, vp, vp]
    L.pseg_predict_chain.argtypes = [vp, vp, i, i, i, i, vp, c.POINTER(i), i, c.c_uint, vp, vp, vp, i, vp, vp, vp, vp]
    L.pseg_bbox_fill_device_u8.argtypes = [i, vp, vp, i, i, i, vp]
    L.pseg_resize_nearest_device.argtypes = [i, vp, i, i, i, vp, i, i, vp]
    L.pseg_predict_margin_device.argtypes = [vp, vp, i, i, vp, vp, vp]
    L.pseg_predict_exact_labels_device.argtypes = [vp, vp, i, i, vp, vp, vp, vp]
    L.pseg_predict_exact_labels.argtypes = [vp, vp, i, i, vp, vp]
    L.pseg_label_exact_stats.argtypes = [vp, c.POINTER(c.c_double)]
    L.pseg_label_exact_stats_ex.argtypes = [vp, c.POINTER(c.c_double), i]
    L.pseg_host_alloc.argtypes = [c.POINTER(vp), c.c_size_t]
    L.pseg_host_free.argtypes = [vp]
    L.pseg_host_register.argtypes = [vp, c.c_size_t]
    L.pseg_host_unregister.argtypes = [vp]
    L.pseg_get_activation.argtypes = [vp, c.c_char_p, vp, i64, c.POINTER(i)]
    L.pseg_engine_stream.argtypes = [vp]
    L.pseg_engine_stream.restype = vp
    L.pseg_flops_per_pixel.argtypes = [vp]
    L.pseg_flops_per_pixel.restype = c.c_double
    L.pseg_timing_enable.argtypes = [vp, i]
    L.pseg_timing_reset.argtypes = [vp]
    L.pseg_timing_num_slots.argtypes = [vp]
    L.pseg_timing_get.argtypes = [vp, i, c.c_char_p, c.c_size_t, c.POINTER(c.c_double),
                                  c.POINTER(i64), c.POINTER(c.c_double)]
    f = c.c_float
    L.pseg_train_init.argtypes = [vp, f, f, f, f, f]
    L.pseg_train_set_optimizer.argtypes = [vp, i]
    L.pseg_train_set_loss.argtypes = [vp, i]
    L.pseg_train_set_dropout_seed.argtypes = [vp, c.c_uint32]
    L.pseg_train_forward_backward.argtypes = [vp, vp, vp, i, i, c.POINTER(f)]
    L.pseg_train_forward_backward_f32.argtypes = [vp, vp, vp, i, i, c.POINTER(f)]
    L.pseg_train_forward_backward_aug.argtypes = [vp, vp, vp, i, i, vp, vp, c.c_uint, i, f, i, f, i, f, c.POINTER(f)]
    L.pseg_train_augment_sample.argtypes = [vp, vp, vp, i, i, vp, vp, c.c_uint, i, f, i, f, i, f, vp, vp]
    L.pseg_train_grad_buffer.argtypes = [vp, c.POINTER(vp), c.POINTER(i64)]
    L.pseg_train_metrics.argtypes = [vp, c.POINTER(f)]
    L.pseg_train_apply.argtypes = [vp, f, f]
    L.pseg_train_get_gradient.argtypes = [vp, c.c_char_p, vp, i64]
    L.pseg_train_wgrad_layer.argtypes = [vp, c.POINTER(WGRAD_LAYER), c.POINTER(WGRAD_PLAN)]
    L.pseg_eval_step.argtypes = [vp, vp, vp, i, i, c.POINTER(f)]
    L.pseg_allreduce_unique_id.argtypes = [vp]
    L.pseg_allreduce_init.argtypes = [vp, i, i, vp]
    L.pseg_train_allreduce.argtypes = [vp]
    L.pseg_allreduce_destroy.argtypes = [vp]
    L.pseg_cc_vote.argtypes = [i, vp, vp, i, i, i]
    d = c.c_double
    L.pseg_rescale_shape.argtypes = [i, i, d, c.POINTER(i), c.POINTER(i)]
    L.pseg_gaussian_kernel.argtypes = [d, vp, i, c.POINTER(i)]
    L.pseg_resize_nearest.argtypes = [i, vp, i, i, i, vp, i, i]
    L.pseg_scale_image.argtypes = [i, vp, i, i, i, vp, i, i, vp, i, vp, i]
    L.pseg_prepare_images.argtypes = [i, vp, vp, i, i, i, i, vp, i, vp, i, i, i, vp, i, vp, i, vp, vp, vp, vp]
    L.pseg_affine_warp.argtypes = [i, vp, i, i, vp, vp, i, vp]
    L.pseg_affine_warp_fill.argtypes = [i, vp, i, i, vp, vp, i, i, ctypes.c_float, vp]
    L.pseg_brightness_shift.argtypes = [i, vp, i64, ctypes.c_float, vp]
    L.pseg_cc_vote_device.argtypes = [i, vp, vp, i, i, i, vp]
    L.pseg_cc_vote_device_u8.argtypes = [i, vp, vp, i, i, i, vp]
    L.pseg_release_workspace.argtypes = [i]
    L.pseg_masks_device_u8.argtypes = [i, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]
    L.pseg_eval_confusion.argtypes = [i, vp, i, vp, i, vp, i64, i, vp]
    L.pseg_cc_label.argtypes = [i, vp, i, i, i, vp, c.POINTER(c.c_int32)]
    L.pseg_cc_tables.argtypes = [i, vp, i, i, i, vp, i, vp, i, i, vp, vp, vp, vp, vp, vp]
    L.pseg_eval_pages.argtypes = [i, i, c.POINTER(EVAL_PAGE), i, i, i, c.POINTER(EVAL_RULE), vp, vp, vp]
    L.pseg_eval_page_groups.argtypes = [i, vp, vp, vp, vp, i]
    L.pseg_bbox_fill.argtypes = [i, vp, vp, i, i, i]
    L.pseg_masks.argtypes = [i, vp, vp, vp, i, i, i, vp, vp, vp, vp]
    L.pseg_masks_device.argtypes = [i, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]
    L.pseg_otsu_char_height.argtypes = [i, vp, i, i, i, c.POINTER(i), c.POINTER(i)]
    L.pseg_char_heights.argtypes = [i, i, vp, vp, vp, i, vp, vp]
    L.pseg_char_height_window.argtypes = [c.POINTER(i)] * 6
    L.pseg_char_height_median.argtypes = [vp, i, i, c.POINTER(i)]
    sz = c.c_size_t
    L.pseg_png_bound.argtypes = [i, i, i, i]
    L.pseg_png_bound.restype = sz
    L.pseg_png_encode_device.argtypes = [i, vp, i, i, i, i, vp, sz, c.POINTER(sz), vp]
    L.pseg_masks_png_device_u8.argtypes = [i, vp, vp, vp, i, i, i, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz), vp]
    L.pseg_png_encode.argtypes = [i, vp, i, i, i, i, vp, sz, c.POINTER(sz)]
    L.pseg_masks_png.argtypes = [i, vp, vp, vp, i, i, i, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz)]
    L.pseg_predict_chain_png.argtypes = [vp, vp, i, i, i, i, vp, c.POINTER(i), i, c.c_uint, vp, vp, vp, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz)]
    L.pseg_png_bound_lv.argtypes = [i, i, i, i, i]
    L.pseg_png_bound_lv.restype = sz
    L.pseg_png_encode_device_lv.argtypes = [i, vp, i, i, i, i, i, vp, sz, c.POINTER(sz), vp]
    L.pseg_masks_png_device_u8_lv.argtypes = [i, vp, vp, vp, i, i, i, i, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz), vp]
    L.pseg_png_encode_lv.argtypes = [i, vp, i, i, i, i, i, vp, sz, c.POINTER(sz)]
    L.pseg_masks_png_lv.argtypes = [i, vp, vp, vp, i, i, i, i, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz)]
    L.pseg_predict_chain_png_lv.argtypes = [vp, vp, i, i, i, i, vp, c.POINTER(i), i, c.c_uint, vp, vp, vp, i, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(sz)]
    L.pseg_png_code_lengths.argtypes = [vp, i, i, vp]
    L.pseg_predict_chain_pages_png.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, c.POINTER(i), i, c.c_uint, vp, i, i, c.c_uint, i, CHAIN_SINK, vp]
    L.pseg_chain_units.argtypes = [i, vp, vp, vp, vp, i, vp, vp, i]
    L.pseg_predict_chain_pages_mixed_png.argtypes = L.pseg_predict_chain_pages_png.argtypes
    L.pseg_chain_units_mixed.argtypes = [i, vp, vp, i, vp, vp, vp, i]
    L.pseg_prepare_scans.argtypes = [i, i, c.POINTER(SCAN), vp, vp, vp]
    L.pseg_predict_chain_scans_png.argtypes = [vp, i, c.POINTER(SCAN), c.POINTER(i), i, c.c_uint, vp, i, i, c.c_uint, i, CHAIN_SINK, vp]
    L.pseg_binarize_scans.argtypes = [i, i, vp, vp, vp, c.POINTER(BINARIZE), vp, vp]
    L.pseg_binarize_scans_host.argtypes = [i, vp, vp, vp, c.POINTER(BINARIZE), vp, vp]
    L.pseg_binarize_geometry.argtypes = [c.POINTER(i)] * 4
    L.pseg_despeckle_maps.argtypes = [i, i, vp, vp, vp, c.POINTER(DESPECKLE), vp, vp]
    L.pseg_despeckle_maps_host.argtypes = [i, vp, vp, vp, c.POINTER(DESPECKLE), vp, vp]
    L.pseg_despeckle_geometry.argtypes = [c.POINTER(i)] * 4
    L.pseg_skew_maps.argtypes = [i, i, vp, vp, vp, c.POINTER(SKEW), vp, vp]
    L.pseg_skew_maps_host.argtypes = [i, vp, vp, vp, c.POINTER(SKEW), vp, vp]
    L.pseg_rotate_maps.argtypes = [i, i, vp, vp, vp, c.POINTER(ROTATE), vp]
    L.pseg_rotate_maps_host.argtypes = [i, vp, vp, vp, c.POINTER(ROTATE), vp]
    L.pseg_deskew_scans.argtypes = [i, i, vp, vp, vp, vp, c.POINTER(SKEW), vp, vp]
    L.pseg_deskew_scans_host.argtypes = [i, vp, vp, vp, vp, c.POINTER(SKEW), vp, vp]
    L.pseg_skew_geometry.argtypes = [c.POINTER(i)] * 3
    L.pseg_text_regions.argtypes = [i, i, vp, vp, vp, c.POINTER(REGIONS), vp, i, vp, vp]
    L.pseg_text_regions_host.argtypes = [i, vp, vp, vp, c.POINTER(REGIONS), vp, i, vp, vp]
    L.pseg_regions_geometry.argtypes = [c.POINTER(i)] * 6
    L.pseg_trace_regions_host.argtypes = [vp, i, i, i, vp, vp, i64, vp]
    L.pseg_predict_chain_pages_regions_png.argtypes = list(L.pseg_predict_chain_pages_png.argtypes[:-2]) + [i, c.POINTER(REGIONS), i, i] + \
        list(L.pseg_predict_chain_pages_png.argtypes[-2:])
    L.pseg_text_regions_poly.argtypes = [i, i, vp, vp, vp, c.POINTER(REGIONS), vp, i, vp, vp, vp, i64, vp, vp]
    L.pseg_text_regions_poly_host.argtypes = [i, vp, vp, vp, c.POINTER(REGIONS), vp, i, vp, vp, vp, i64, vp, vp]
    L.pseg_prepare_scans_clean.argtypes = [i, i, c.POINTER(SCAN), c.POINTER(BINARIZE), c.POINTER(DESPECKLE), vp, vp, vp]
    L.pseg_predict_chain_scans_clean_png.argtypes = [vp, i, c.POINTER(SCAN), c.POINTER(BINARIZE), c.POINTER(DESPECKLE), c.POINTER(i), i, c.c_uint, vp, i, i,
                                                     c.c_uint, i, CHAIN_SINK, vp]
    L.pseg_predict_chain_scans_regions_png.argtypes = list(L.pseg_predict_chain_scans_clean_png.argtypes[:-2]) + [c.POINTER(REGIONS), i, i] + \
        list(L.pseg_predict_chain_scans_clean_png.argtypes[-2:])
    L.pseg_prepare_scans_bin.argtypes = [i, i, c.POINTER(SCAN), c.POINTER(BINARIZE), vp, vp, vp]
    L.pseg_predict_chain_scans_bin_png.argtypes = [vp, i, c.POINTER(SCAN), c.POINTER(BINARIZE), c.POINTER(i), i, c.c_uint, vp, i, i, c.c_uint, i, CHAIN_SINK, vp]
    L.pseg_label_masks.argtypes = [i, i, c.POINTER(MASK_SRC), vp, vp, vp, vp, i, vp, vp]
    L.pseg_label_masks_host.argtypes = [i, c.POINTER(MASK_SRC), vp, vp, vp, vp, i, vp, vp]
    L.pseg_label_masks_geometry.argtypes = [c.POINTER(i)] * 4 + [c.POINTER(i64)]
    L.pseg_label_masks_groups.argtypes = [i, c.POINTER(MASK_SRC), vp]
    L.pseg_tile_plan.argtypes = [i, i, i, i, c.POINTER(i), c.POINTER(i), vp, vp, vp, i]
    L.pseg_predict_tiled_device.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    L.pseg_predict_tiled.argtypes = [vp, vp, i, i, i, vp, vp]
    L.pseg_engine_set_tiling.argtypes = [vp, i, i]
    L.pseg_engine_page_fits.argtypes = [vp, i, i]
    L.pseg_png_probe.argtypes = [vp, sz, c.POINTER(i), c.POINTER(i), c.POINTER(i)]
    L.pseg_png_decode_gray.argtypes = [i, i, vp, vp, vp, vp]
    L.pseg_png_decode_gray_device.argtypes = [i, i, vp, vp, vp, vp, vp]
    L.pseg_png_decode_gray_host.argtypes = [i, vp, vp, vp, vp]
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise PsegError(lib().pseg_last_error().decode("utf-8", "replace") or "pseg error %d" % rc)


def device_count():
    return int(lib().pseg_device_count())


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _PinnedBlock:
    """Owner of one pseg_host_alloc block; freed when the last array viewing it goes away."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        _check(lib().pseg_host_alloc(ctypes.byref(p), int(nbytes)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().pseg_host_free(ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.uint8):
    """NumPy array in page-locked host memory (pseg_host_alloc): pages and label maps kept in such arrays move by DMA
    straight from / to the array in Engine.predict_batch, overlapped with compute."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
    blk = _PinnedBlock(max(n, 1))
    buf = (ctypes.c_char * max(n, 1)).from_address(blk.ptr)
    buf._pseg_block = blk                       # keeps the block alive as long as any view of the buffer
    a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
    return a


class _PinnedPool:
    """Recycled page-locked blocks for arrays handed to callers (the Predictor chain's label maps and masks): pinning
    150 MB per call costs more than the chain itself, and a fresh pageable array that size pays ~18 ms of first-touch
    page faults before the copy starts.  A block returns to the pool when the last NumPy view of it is collected."""
    MAX_BYTES = 2 << 30

    def __init__(self):
        self.free, self.held = {}, 0

    def take(self, nbytes):
        lst = self.free.get(nbytes)
        if lst:
            self.held -= nbytes
            return lst.pop()
        return _PinnedBlock(nbytes)

    def give(self, blk):
        if self.held + blk.nbytes > self.MAX_BYTES:
            return                                   # dropped: _PinnedBlock.__del__ frees it
        self.free.setdefault(blk.nbytes, []).append(blk)
        self.held += blk.nbytes

    def clear(self):
        self.free, self.held = {}, 0


_POOL = _PinnedPool()


class _PooledLease:
    def __init__(self, blk):
        self.blk = blk

    def __del__(self):
        try:
            _POOL.give(self.blk)
        except Exception:
            pass


def pinned_empty_pooled(shape, dtype=np.uint8):
    """As pinned_empty, from the recycling pool (sizes rounded up to 1 MiB so that pages of one format share blocks)."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape, dtype=np.int64))
    n = max(count * dt.itemsize, 1)
    n = (n + (1 << 20) - 1) >> 20 << 20
    blk = _POOL.take(n)
    buf = (ctypes.c_char * n).from_address(blk.ptr)
    buf._pseg_lease = _PooledLease(blk)
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def pinned_copy(a):
    """A page-locked copy of `a`."""
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class Engine:
    """Opaque pseg_engine handle: one FCN graph + its weights resident on one GPU."""

    def __init__(self, arch="fcn_skip", n_classes=3, in_channels=1, device=0, mode=MODE_BF16, batch_norm=False, plan=None):
        """batch_norm: BatchNormalization at res_unet's bn_act sites (lib/model.py:265-271; PSEG_FLAG_BATCHNORM).
        plan: plan switches for pseg_create_plan, "PSEG_NO_DQ=1;PSEG_NO_PAIRC2=1" or a dict (tests and A/B measurements: every
        switch keeps the results within the documented bars).  With PLAN_FROM_ENV set (tests/conftest.py, tools/) and no plan given,
        the PSEG_* variables of os.environ that the library does not read itself become the plan -- the test suite keeps steering
        kernels with monkeypatch.setenv while the release library ignores the environment beyond pseg_env_knobs()."""
        self._h = None
        L = lib()
        arch_id = ARCH_IDS[arch] if isinstance(arch, str) else int(arch)
        h = ctypes.c_void_p()
        if plan is None and PLAN_FROM_ENV:
            listed = set(L.pseg_env_knobs().decode().split("\n"))
            plan = {k: v for k, v in os.environ.items() if k.startswith("PSEG_") and k not in listed and k not in ("PSEG_LIB",)}
        if isinstance(plan, dict):
            plan = ";".join("%s=%s" % kv for kv in sorted(plan.items()))
        _check(L.pseg_create_plan(arch_id, int(n_classes), int(in_channels), int(device), int(mode),
                                  FLAG_BATCHNORM if batch_norm else 0, (plan or "").encode(), ctypes.byref(h)))
        self._h = h
        self.batch_norm = bool(batch_norm)
        self.arch = arch
        self.n_classes = int(n_classes)
        self.in_channels = int(in_channels)
        self.device = int(device)
        self.mode = int(mode)

    def close(self):
        if self._h is not None:
            lib().pseg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -------------------------------------------------------------------------------
    def weight_specs(self):
        L = lib()
        out = []
        name = ctypes.create_string_buffer(128)
        shape = (ctypes.c_int64 * 4)()
        nd = ctypes.c_int()
        for i in range(L.pseg_num_weights(self._h)):
            _check(L.pseg_weight_info(self._h, i, name, 128, shape, ctypes.byref(nd)))
            out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value))))
        return out

    def set_weights(self, weights):
        """weights: mapping name -> ndarray in Keras layout."""
        L = lib()
        for name, arr in weights.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shp = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            _check(L.pseg_set_weights(self._h, name.encode(), _ptr(a), shp, a.ndim))

    def get_weights(self):
        L = lib()
        out = {}
        for name, shp in self.weight_specs():
            a = np.empty(shp, np.float32)
            _check(L.pseg_get_weights(self._h, name.encode(), _ptr(a), a.size))
            out[name] = a
        return out

    # -- predict -------------------------------------------------------------------------------
    def predict(self, image, want_logits=True, want_probs=True, want_labels=True):
        """uint8 (H,W) [or (H,W,3)] -> (logits f32 (H,W,C) | None, probs | None, labels int64 | None).
        Mirrors Network.predict_single_data (lib/network.py:248-260)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.ndim == 3 and img.shape[2] == 1:
            img = img[..., 0]
        if img.ndim != (2 if self.in_channels == 1 else 3):
            raise PsegError("image of shape %r does not match in_channels=%d" % (img.shape, self.in_channels))
        H, W = img.shape[:2]
        C = self.n_classes
        logits = np.empty((H, W, C), np.float32) if want_logits else None
        probs = np.empty((H, W, C), np.float32) if want_probs else None
        labels = np.empty((H, W), np.int64) if want_labels else None
        _check(lib().pseg_predict(self._h, _ptr(img), H, W, _ptr(logits), _ptr(probs), _ptr(labels)))
        return logits, probs, labels

    def predict_device(self, d_img, H, W, d_logits=0, d_probs=0, d_labels=0, d_labels_u8=0, stream=0):
        """Raw device pointers (ints, e.g. torch.Tensor.data_ptr()); asynchronous."""
        _check(lib().pseg_predict_device(self._h, ctypes.c_void_p(d_img), int(H), int(W),
                                         ctypes.c_void_p(d_logits or None), ctypes.c_void_p(d_probs or None),
                                         ctypes.c_void_p(d_labels or None), ctypes.c_void_p(d_labels_u8 or None),
                                         ctypes.c_void_p(stream or None)))

    def predict_pages_device(self, d_imgs, n_pages, H, W, d_labels=0, d_labels_u8=0, stream=0):
        """n_pages pages of one shape, contiguous on the device -> their label maps, contiguous (lib/predictor.py:27-30); asynchronous."""
        _check(lib().pseg_predict_pages_device(self._h, ctypes.c_void_p(d_imgs), int(n_pages), int(H), int(W), ctypes.c_void_p(d_labels or None),
                                               ctypes.c_void_p(d_labels_u8 or None), ctypes.c_void_p(stream or None)))

    def status(self, stream=0):
        """Waits for `stream` (0: the engine's own), then raises PsegError if a kernel reported an error since the last check
        (pseg_engine_status): what the asynchronous *_device calls cannot tell their caller."""
        _check(lib().pseg_engine_status(self._h, ctypes.c_void_p(stream or None)))

    def trim(self):
        """Frees the activation tensors (every page slot); the next predict call allocates what it needs (pseg_engine_trim)."""
        _check(lib().pseg_engine_trim(self._h))

    # -- tiled prediction (pseg_tile_plan's plan; include/pseg.h) -----------------------------------
    TILING = {"off": 0, "auto": 1, "always": 2}

    def set_tiling(self, mode, tile=0):
        """Where predict / predict_device / predict_chain use tiles when label maps alone are asked for (pseg_engine_set_tiling):
        "off" (the default: never), "auto" (the pages the whole-page path refuses or has no memory for) or "always"; tile: the
        tile edge, 0 = the default.  The label maps are the whole page's, so the route does not show in the output."""
        if mode not in self.TILING and mode not in self.TILING.values():
            raise PsegError("tiling mode %r (one of %r)" % (mode, tuple(self.TILING)))
        _check(lib().pseg_engine_set_tiling(self._h, int(self.TILING.get(mode, mode)), int(tile)))

    def page_fits(self, H, W):
        """True when the whole-page path takes an H x W page on this engine now (pseg_engine_page_fits); False: the pages that
        tiling mode "auto" tiles and the page-list entries refuse."""
        rc = lib().pseg_engine_page_fits(self._h, int(H), int(W))
        _check(min(rc, 0))
        return rc == 1

    def predict_tiled(self, image, tile=0, dtype=np.int64):
        """uint8 (H,W) [or (H,W,3)] page of any size -> its label map, computed in tiles of edge `tile` (0: the default) through
        the page-slot path (pseg_predict_tiled): equal to predict(...)[2] wherever the whole page can run."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.ndim == 3 and img.shape[2] == 1:
            img = img[..., 0]
        if img.ndim != (2 if self.in_channels == 1 else 3):
            raise PsegError("image of shape %r does not match in_channels=%d" % (img.shape, self.in_channels))
        H, W = img.shape[:2]
        out = np.empty((H, W), dtype)
        if np.dtype(dtype) == np.int64:
            _check(lib().pseg_predict_tiled(self._h, _ptr(img), H, W, int(tile), _ptr(out), None))
        elif np.dtype(dtype) == np.uint8:
            _check(lib().pseg_predict_tiled(self._h, _ptr(img), H, W, int(tile), None, _ptr(out)))
        else:
            raise PsegError("labels dtype must be int64 or uint8")
        return out

    def predict_tiled_device(self, d_img, H, W, tile=0, d_labels=0, d_labels_u8=0, stream=0):
        """Raw device pointers (ints); asynchronous (pseg_predict_tiled_device)."""
        _check(lib().pseg_predict_tiled_device(self._h, ctypes.c_void_p(d_img), int(H), int(W), int(tile), ctypes.c_void_p(d_labels or None),
                                               ctypes.c_void_p(d_labels_u8 or None), ctypes.c_void_p(stream or None)))

    def predict_margin_device(self, d_img, H, W, d_margin, d_labels_u8=0, stream=0):
        """As predict_device, plus the float32 (H,W) margin map: top-1 minus top-2 logit per pixel."""
        _check(lib().pseg_predict_margin_device(self._h, ctypes.c_void_p(d_img), int(H), int(W), ctypes.c_void_p(d_labels_u8 or None),
                                                ctypes.c_void_p(d_margin), ctypes.c_void_p(stream or None)))

    def predict_exact_labels_device(self, d_img, H, W, d_labels_u8, d_labels=0, d_margin=0, stream=0):
        """Label-exact throughput mode: bf16 pass + margin map, float32 referee on the blocks that hold near-ties; the
        uint8 label map is the float32 engine's wherever the referee looked and wherever the bf16 margin exceeds the
        calibrated threshold (calibrated, not proven: mode=MODE_F32_EXACT is the only bit-exact mode).  Synchronises the stream."""
        _check(lib().pseg_predict_exact_labels_device(self._h, ctypes.c_void_p(d_img), int(H), int(W), ctypes.c_void_p(d_labels_u8),
                                                      ctypes.c_void_p(d_labels or None), ctypes.c_void_p(d_margin or None),
                                                      ctypes.c_void_p(stream or None)))

    def predict_exact_labels(self, image, dtype=np.int64):
        """uint8 (H,W) page -> label map equal to the float32 engine's (host arrays; label-exact mode)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        H, W = img.shape[:2]
        out = np.empty((H, W), dtype)
        if np.dtype(dtype) == np.int64:
            _check(lib().pseg_predict_exact_labels(self._h, _ptr(img), H, W, _ptr(out), None))
        elif np.dtype(dtype) == np.uint8:
            _check(lib().pseg_predict_exact_labels(self._h, _ptr(img), H, W, None, _ptr(out)))
        else:
            raise PsegError("labels dtype must be int64 or uint8")
        return out

    def label_exact_stats(self):
        """Statistics of the last predict_exact_labels[_device] call."""
        v = (ctypes.c_double * 13)()
        _check(lib().pseg_label_exact_stats_ex(self._h, v, 13))
        return {"tau": float(v[0]), "calib_logit_err": float(v[1]), "flagged_px_frac": float(v[2]), "referee_tile_frac": float(v[3]),
                "referee_area_frac": float(v[4]), "tau_escalations": int(v[5]), "whole_page_fallback": int(v[6]),
                "labels_changed": int(v[7]), "margin_err_running": float(v[8]), "referee_rects": int(v[9]),
                "referee_cost_vs_full_page": float(v[10]), "flag_block": int(v[11]), "direct_float32": int(v[12])}

    POST_OPS = {"cc_vote": 1, "bbox": 2}

    def predict_chain(self, image, binary=None, out_shape=None, post_ops=(), exact_labels=False, labels="u8", lut=None,
                      masks=False, png_level=0):
        """The Predictor chain on the device (pseg_predict_chain; lib/predictor.py:32-54): predict -> [nearest resize of
        the label map to out_shape] -> post-processors ("cc_vote" / "bbox", in order) -> [the four masks].  `binary` must
        have the label map's final shape.  Returns {"labels": uint8 or int64 map or None, "masks": (color, overlay,
        inverted, fg_color) or None}; the arrays live in recycled page-locked memory.  masks="png": the four masks come back as
        PNG streams (bytes objects) encoded on the device (pseg_predict_chain_png_lv, at `png_level`), decoding to the arrays
        masks=True returns."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        H, W = img.shape[:2]
        Ho, Wo = (int(out_shape[0]), int(out_shape[1])) if out_shape is not None else (0, 0)
        Hl, Wl = (Ho, Wo) if Ho > 0 else (H, W)
        b = None
        if binary is not None:
            b = np.ascontiguousarray(binary, dtype=np.uint8)
            if b.shape != (Hl, Wl):
                raise PsegError("binary has shape %r, the label map %r" % (b.shape, (Hl, Wl)))
        ops = (ctypes.c_int * max(len(post_ops), 1))(*[self.POST_OPS[o] if isinstance(o, str) else int(o) for o in post_ops])
        lab = None
        if labels == "u8":
            lab = pinned_empty_pooled((Hl, Wl), np.uint8)
        elif labels == "i64":
            lab = pinned_empty_pooled((Hl, Wl), np.int64)
        elif labels is not None:
            raise PsegError("labels must be 'u8', 'i64' or None")
        t = None
        outs = [None] * 4
        if masks == "png":
            t = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
            bufs, P, caps, sizes = _png_buffers(Hl, Wl, 3, 0, [True] * 4, png_level)
            _check(lib().pseg_predict_chain_png_lv(self._h, _ptr(img), H, W, Ho, Wo, _ptr(b), ops, len(post_ops), 1 if exact_labels else 0,
                                                   _ptr(lab) if labels == "i64" else None, _ptr(lab) if labels == "u8" else None,
                                                   _ptr(t), t.shape[0], int(png_level), P, caps, sizes))
            return {"labels": lab, "masks": tuple(bufs[k][:sizes[k]].tobytes() for k in range(4))}
        if masks:
            t = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
            outs = [pinned_empty_pooled((Hl, Wl, 3), np.uint8) for _ in range(4)]
        _check(lib().pseg_predict_chain(self._h, _ptr(img), H, W, Ho, Wo, _ptr(b), ops, len(post_ops), 1 if exact_labels else 0,
                                        _ptr(lab) if labels == "i64" else None, _ptr(lab) if labels == "u8" else None,
                                        _ptr(t), 0 if t is None else t.shape[0], *[_ptr(o) for o in outs]))
        return {"labels": lab, "masks": tuple(outs) if masks else None}

    def predict_chain_pages(self, images, binaries=None, out_shapes=None, post_ops=(), exact_labels=False, lut=None,
                            which=("color", "overlay", "inverted"), labels=False, png_level=0, unit_cap=0, sink=None, mixed=False,
                            regions=None, max_regions=256, max_vertices=1 << 16):
        """A page list through the chain to PNG streams (pseg_predict_chain_pages_png; lib/predictor.py:27-30 over :49-54): per page
        predict -> [nearest resize to out_shapes[i]] -> post-processors -> the masks named in `which` as PNG streams, units of
        same-shape pages pipelined on the device; every stream (and label map, with labels=True) has predict_chain's bytes for that
        page alone.  binaries[i] / out_shapes[i] may be None.  sink=None: a list of {"labels": uint8 map or None, "masks": {name:
        bytes}} per page.  With a callable, sink(page, name, data) is called per output as it arrives -- page order, then color /
        overlay / inverted / fg_color / "labels" (data: bytes, for "labels" the uint8 map) -- and None is returned; an exception in
        the sink stops the call and is raised again after it.
        mixed=True (pseg_predict_chain_pages_mixed_png): for lists whose pages differ in shape.  Units are formed from the pages of
        one canvas (chain_units_mixed) whatever their own and their final shapes; the bytes are the same, the list return stays in
        page order, a callable sink sees the units in the planner's order (pages of a unit in the permuted order).
        regions: a TextRegions or one per page (pseg_predict_chain_pages_regions_png): the text regions of every page's final label map
        and their polygons, found and traced on the device behind the post-processors.  Every result dict gains "regions": {"boxes",
        "areas", "seeds", "polygons", "status"} as text_regions(polygons=True) gives them for that label map; status 0, or
        PSEG_EUNSUPPORTED (more than max_regions regions: no rows), PSEG_ENOMEM (more than max_vertices vertices: rows, polygons None)
        or PSEG_EHIP.  A callable sink receives the record under the name "regions", after "labels".  which=() with labels=False asks
        for the regions alone."""
        for w in which:
            if w not in MASK_NAMES:
                raise PsegError("unknown mask %r (one of %r)" % (w, MASK_NAMES))
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        n = len(imgs)
        outs = list(out_shapes) if out_shapes is not None else [None] * n
        bins_in = list(binaries) if binaries is not None else [None] * n
        if len(outs) != n or len(bins_in) != n:
            raise PsegError("binaries / out_shapes must have one entry per page")
        final, bins = [], []
        for k in range(n):
            fs = (int(outs[k][0]), int(outs[k][1])) if outs[k] is not None else imgs[k].shape[:2]
            b = None
            if bins_in[k] is not None:
                b = np.ascontiguousarray(bins_in[k], dtype=np.uint8)
                if b.shape != fs:
                    raise PsegError("page %d: binary has shape %r, the label map %r" % (k, b.shape, fs))
            final.append(fs)
            bins.append(b)
        P, I = ctypes.c_void_p * max(n, 1), ctypes.c_int * max(n, 1)
        ip = P(*[im.ctypes.data for im in imgs])
        bp = P(*[None if b is None else b.ctypes.data for b in bins])
        hs, ws = I(*[im.shape[0] for im in imgs]), I(*[im.shape[1] for im in imgs])
        ho = I(*[0 if o is None else int(o[0]) for o in outs])
        wo = I(*[0 if o is None else int(o[1]) for o in outs])
        if regions is not None:
            rg = regions_table(regions, n, "page")
            return self._chain_list(final, post_ops, lut, which, labels, sink,
                                    lambda ops, t, want, cb: lib().pseg_predict_chain_pages_regions_png(
                                        self._h, n, ip, hs, ws, ho, wo, bp, ops, len(post_ops), 1 if exact_labels else 0, _ptr(t),
                                        0 if t is None else t.shape[0], int(png_level), want, int(unit_cap), 1 if mixed else 0, rg, int(max_regions),
                                        int(max_vertices), cb, None), regions=True)
        entry = lib().pseg_predict_chain_pages_mixed_png if mixed else lib().pseg_predict_chain_pages_png
        return self._chain_list(final, post_ops, lut, which, labels, sink,
                                lambda ops, t, want, cb: entry(self._h, n, ip, hs, ws, ho, wo, bp, ops, len(post_ops), 1 if exact_labels else 0,
                                                               _ptr(t), 0 if t is None else t.shape[0], int(png_level), want, int(unit_cap), cb, None))

    def _chain_list(self, final, post_ops, lut, which, labels, sink, call, regions=False):
        """The part the list entries share: op ids, colour table, `want` bits and the C sink that feeds `sink` or collects the result
        dicts; call(ops, table, want, c_sink) -> the entry's return code.  final[i]: the shape of page i's label map."""
        n = len(final)
        want = sum(1 << MASK_NAMES.index(w) for w in set(which)) | (16 if labels else 0) | (32 if regions else 0)
        ops = (ctypes.c_int * max(len(post_ops), 1))(*[self.POST_OPS[o] if isinstance(o, str) else int(o) for o in post_ops])
        t = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
        collected = [{"labels": None, "masks": {}} for _ in range(n)] if sink is None else None
        raised = []

        def on_output(_user, page, k, data, n_bytes):
            try:
                if k == 4:
                    item, name = np.ctypeslib.as_array(data, (n_bytes,)).reshape(final[page]).copy(), "labels"
                elif k == 5:
                    item, name = regions_of_blob(np.frombuffer(ctypes.string_at(data, n_bytes), np.int32)), "regions"
                else:
                    item, name = ctypes.string_at(data, n_bytes), MASK_NAMES[k]
                if sink is not None:
                    sink(page, name, item)
                elif k == 4 or k == 5:
                    collected[page][name] = item
                else:
                    collected[page]["masks"][name] = item
                return 0
            except BaseException as exc:          # (an exception must not cross the C frames: stop the call, raise afterwards)
                raised.append(exc)
                return 1

        rc = call(ops, t, want, CHAIN_SINK(on_output))
        if raised:
            raise raised[0]
        _check(rc)
        return collected

    def predict_chain_scans(self, scans, scales, high_res=False, post_ops=(), exact_labels=False, lut=None,
                            which=("color", "overlay", "inverted"), labels=False, png_level=0, unit_cap=0, sink=None, binarize=None,
                            despeckle=None, regions=None, max_regions=256, max_vertices=1 << 16):
        """Scans as they come off disk through the chain to PNG streams (pseg_predict_chain_scans_png): scans[i] a gray uint8 (H0,W0)
        array, scales[i] = target_line_height / line_height_px.  The binarisation (ink = scan <= 127) and the line-height
        normalisation run on the device in front of the network: neither the normalised page nor the ink map visits the host.
        Every stream and label map equals predict_chain_pages(mixed=True) fed with prepare_images(scan, where(scan > 127, 255, 0),
        scale): the page, `bin` as the binarisation -- with high_res the label map is rescaled to the scan's shape and `orig` is the
        binarisation (PredictSettings.high_res_output).  Keywords, result dicts and the sink contract are predict_chain_pages'
        (mixed=True: a callable sink sees the planner's order).
        binarize: None (ink = scan <= 127), a Sauvola with a window, or one of either per scan (binarize_table): the ink map of
        binarize_scans takes the place of scan <= 127 everywhere (pseg_predict_chain_scans_bin_png).
        despeckle: None, a Despeckle with its max_area, or one of either per scan (despeckle_table): despeckle_maps of that ink map
        takes its place everywhere (pseg_predict_chain_scans_clean_png); None is the call without the argument.
        regions, max_regions, max_vertices: predict_chain_pages' (pseg_predict_chain_scans_regions_png)."""
        for w in which:
            if w not in MASK_NAMES:
                raise PsegError("unknown mask %r (one of %r)" % (w, MASK_NAMES))
        table, keep, plans = scan_table(scans, scales, high_res)
        n = len(plans)
        how = None if binarize is None else binarize_table(binarize, n)
        final = [keep[k].shape if high_res else plans[k][:2] for k in range(n)]
        if regions is not None:
            rg = regions_table(regions, n, "scan")
            dsp = None if despeckle is None else despeckle_table(despeckle, n, "scan")
            return self._chain_list(final, post_ops, lut, which, labels, sink,
                                    lambda ops, t, want, cb: lib().pseg_predict_chain_scans_regions_png(
                                        self._h, n, table, how, dsp, ops, len(post_ops), 1 if exact_labels else 0, _ptr(t), 0 if t is None else t.shape[0],
                                        int(png_level), want, int(unit_cap), rg, int(max_regions), int(max_vertices), cb, None), regions=True)
        if despeckle is not None:
            dsp = despeckle_table(despeckle, n, "scan")
            return self._chain_list(final, post_ops, lut, which, labels, sink,
                                    lambda ops, t, want, cb: lib().pseg_predict_chain_scans_clean_png(
                                        self._h, n, table, how, dsp, ops, len(post_ops), 1 if exact_labels else 0, _ptr(t), 0 if t is None else t.shape[0],
                                        int(png_level), want, int(unit_cap), cb, None))
        return self._chain_list(final, post_ops, lut, which, labels, sink,
                                lambda ops, t, want, cb: lib().pseg_predict_chain_scans_bin_png(
                                    self._h, n, table, how, ops, len(post_ops), 1 if exact_labels else 0, _ptr(t), 0 if t is None else t.shape[0],
                                    int(png_level), want, int(unit_cap), cb, None))

    def predict_batch(self, images, dtype=np.int64, out=None):
        """Label maps of a list of (H,W) uint8 pages (sizes may differ); copies overlap compute.
        `out`: optional list of preallocated C-contiguous label arrays to fill (fresh 25 MB arrays cost
        more in first-touch page faults than the transfer itself)."""
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        n = len(imgs)
        if any(im.ndim != 2 for im in imgs) and self.in_channels == 1:
            raise PsegError("pages must be 2-D uint8 arrays")
        if out is not None:
            if len(out) != n or any(o.shape != im.shape[:2] or o.dtype != np.dtype(dtype) or not o.flags.c_contiguous
                                    for o, im in zip(out, imgs)):
                raise PsegError("out must hold one C-contiguous %s array of the page's shape per page" % np.dtype(dtype))
            outs = list(out)
        else:
            outs = [np.empty(im.shape[:2], dtype) for im in imgs]
        P = ctypes.c_void_p * max(n, 1)
        I = ctypes.c_int * max(n, 1)
        ip = P(*[im.ctypes.data for im in imgs]) if n else P()
        op = P(*[o.ctypes.data for o in outs]) if n else P()
        hs, ws = I(*[im.shape[0] for im in imgs]), I(*[im.shape[1] for im in imgs])
        if np.dtype(dtype) == np.int64:
            _check(lib().pseg_predict_batch(self._h, n, ip, hs, ws, op, None))
        elif np.dtype(dtype) == np.uint8:
            _check(lib().pseg_predict_batch(self._h, n, ip, hs, ws, None, op))
        else:
            raise PsegError("labels dtype must be int64 or uint8")
        return outs

    def activation(self, layer):
        dims = (ctypes.c_int * 3)()
        _check(lib().pseg_get_activation(self._h, layer.encode(), None, 0, dims))
        out = np.empty((dims[0], dims[1], dims[2]), np.float32)
        _check(lib().pseg_get_activation(self._h, layer.encode(), _ptr(out), out.size, dims))
        return out

    # -- training (float32 engine) -----------------------------------------------------------------
    def train_init(self, beta1=0.9, beta2=0.999, eps=1e-7, clipnorm=1.0, clipvalue=0.0):
        """Keras Adam defaults; clipnorm is per tensor (lib/network.py:97), <= 0 disables."""
        _check(lib().pseg_train_init(self._h, beta1, beta2, eps, clipnorm, clipvalue))

    # -- data-parallel training through the C ABI (RCCL bound at run time; pseg_amd.parallel offers torch.distributed instead)
    @staticmethod
    def allreduce_unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check(lib().pseg_allreduce_unique_id(buf))
        return bytes(buf)

    def allreduce_init(self, rank, world, unique_id):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().pseg_allreduce_init(self._h, int(rank), int(world), buf))

    def train_allreduce(self):
        _check(lib().pseg_train_allreduce(self._h))

    def allreduce_destroy(self):
        _check(lib().pseg_allreduce_destroy(self._h))

    OPTIMIZERS = {"adam": 0, "adamax": 1, "adadelta": 2, "adagrad": 3, "rmsprop": 4, "sgd": 5, "nadam": 6}

    def train_set_optimizer(self, name):
        """One of the reference's Optimizers enum values (lib/architecture.py:71-78), Keras defaults."""
        if name not in self.OPTIMIZERS:
            raise PsegError("unknown optimizer %r" % (name,))
        _check(lib().pseg_train_set_optimizer(self._h, self.OPTIMIZERS[name]))

    LOSSES = {"categorical_crossentropy": 0, "jaccard": 1, "dice": 2, "categorical_hinge": 3, "categorical_focal": 4,
              "dice_and_crossentropy": 5}

    def train_set_loss(self, name):
        """One of the reference's Loss enum values (lib/metrics.py:116-121)."""
        if name not in self.LOSSES:
            raise PsegError("unknown loss %r" % (name,))
        _check(lib().pseg_train_set_loss(self._h, self.LOSSES[name]))

    def _img_mask(self, image, mask):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        msk = np.ascontiguousarray(mask, dtype=np.uint8)
        if img.shape[:2] != msk.shape[:2]:
            raise PsegError("image %r and mask %r differ in shape" % (img.shape, msk.shape))
        return img, msk

    def train_forward_backward(self, image, mask):
        """-> (loss, accuracy, jacard_coef, dice_coef) of this page; gradients stay on the device."""
        img, msk = self._img_mask(image, mask)
        m = (ctypes.c_float * 4)()
        _check(lib().pseg_train_forward_backward(self._h, _ptr(img), _ptr(msk), img.shape[0], img.shape[1], m))
        return tuple(float(v) for v in m)

    def train_set_dropout_seed(self, seed):
        """Seed of the Dropout masks (unet); also restarts the step counter the masks depend on."""
        _check(lib().pseg_train_set_dropout_seed(self._h, int(seed) & 0xFFFFFFFF))

    def train_forward_backward_float(self, image, mask):
        """As train_forward_backward with a float32 page on the 0..255 scale (augmented sample)."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if img.shape[:2] != m.shape[:2]:
            raise PsegError("image %r and mask %r differ in shape" % (img.shape, m.shape))
        out = (ctypes.c_float * 4)()
        _check(lib().pseg_train_forward_backward_f32(self._h, _ptr(img), _ptr(m), img.shape[0], img.shape[1], out))
        return tuple(float(v) for v in out)

    def _augment_args(self, image_u8, mask_u8, matrix, offset, flips, image_fill, image_cval, mask_fill, mask_cval, brightness):
        """The common arguments of pseg_train_forward_backward_aug / pseg_train_augment_sample (arrays first: they stay alive
        with the tuple)."""
        img, msk = self._img_mask(image_u8, mask_u8)
        if np.asarray(image_u8).dtype != np.uint8 or np.asarray(mask_u8).dtype != np.uint8:
            raise PsegError("the device augmentation takes the uint8 page and the uint8 mask")
        if msk.ndim != 2 or img.shape[2:] not in ((), (self.in_channels,)) or (img.ndim == 2 and self.in_channels != 1):
            raise PsegError("page %r / mask %r do not fit an engine with %d input channels" % (img.shape, msk.shape, self.in_channels))
        if (matrix is None) != (offset is None):
            raise PsegError("matrix and offset come together (both None: no warp)")
        m = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float64).reshape(4)
        o = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64).reshape(2)
        fills = []
        for fm in (image_fill, mask_fill):
            if fm not in FILL_MODES and fm not in FILL_MODES.values():
                raise PsegError("unknown fill mode %r" % (fm,))
            fills.append(FILL_MODES.get(fm, fm))
        return (img, msk, m, o), (self._h, _ptr(img), _ptr(msk), img.shape[0], img.shape[1], _ptr(m), _ptr(o), int(flips),
                                  int(fills[0]), float(image_cval), int(fills[1]), float(mask_cval),
                                  0 if brightness is None else 1, 0.0 if brightness is None else float(brightness))

    def train_forward_backward_augmented(self, image_u8, mask_u8, matrix, offset, flips, image_fill, image_cval, mask_fill,
                                         mask_cval, brightness=None):
        """One augmented training step without host arrays in between (pseg_train_forward_backward_aug): the uint8 page (H,W[,C])
        and mask (H,W) go up once, the sample of lib/network.py:149-161 -- cubic warp of the image by (matrix, offset) with
        image_fill / image_cval, order-0 warp of the mask with mask_fill / mask_cval, flips (bit 0 horizontal, bit 1 vertical),
        brightness factor (None: none) -- is built on the device and trained on.  matrix None: no warp.
        -> (loss, accuracy, jacard_coef, dice_coef)."""
        keep, args = self._augment_args(image_u8, mask_u8, matrix, offset, flips, image_fill, image_cval, mask_fill, mask_cval, brightness)
        out = (ctypes.c_float * 4)()
        _check(lib().pseg_train_forward_backward_aug(*args, out))
        return tuple(float(v) for v in out)

    def augment_sample(self, image_u8, mask_u8, matrix, offset, flips, image_fill, image_cval, mask_fill, mask_cval, brightness=None):
        """The sample train_forward_backward_augmented trains on -> (float32 image (H,W[,C]) on the 0..255 scale, uint8 mask)."""
        keep, args = self._augment_args(image_u8, mask_u8, matrix, offset, flips, image_fill, image_cval, mask_fill, mask_cval, brightness)
        o_img = np.empty(keep[0].shape, np.float32)
        o_msk = np.empty(keep[1].shape, np.uint8)
        _check(lib().pseg_train_augment_sample(*args, _ptr(o_img), _ptr(o_msk)))
        return o_img, o_msk

    def eval_step(self, image, mask):
        img, msk = self._img_mask(image, mask)
        m = (ctypes.c_float * 4)()
        _check(lib().pseg_eval_step(self._h, _ptr(img), _ptr(msk), img.shape[0], img.shape[1], m))
        return tuple(float(v) for v in m)

    def train_apply(self, lr, grad_scale=1.0):
        _check(lib().pseg_train_apply(self._h, float(lr), float(grad_scale)))

    def grad_buffer(self):
        """(device pointer, float count) of the flat gradient buffer -- what DP all-reduces."""
        ptr, n = ctypes.c_void_p(), ctypes.c_int64()
        _check(lib().pseg_train_grad_buffer(self._h, ctypes.byref(ptr), ctypes.byref(n)))
        return int(ptr.value), int(n.value)

    def gradients(self):
        L = lib()
        out = {}
        for name, shp in self.weight_specs():
            a = np.empty(shp, np.float32)
            _check(L.pseg_train_get_gradient(self._h, name.encode(), _ptr(a), a.size))
            out[name] = a
        return out

    def wgrad_layer(self, X, dY, dW, *, mode=0, KW, Cin, Cout, Hx, Wx, Hy, Wy, XC0, X1=None, XC1=0, ci0=0, maskY=None, dB=None,
                    stride=1, xup=False, in_relu=False, logits=False, xpitch=None, slots=0, strip_rows=0):
        """One layer's weight (+ bias) gradient as the train step launches it, on device tensors (pseg_train_wgrad_layer; needs
        train_init).  X, X1, dY, maskY, dW, dB: device pointers (int) or objects with data_ptr() -- float32, NHWC, already
        written (the call runs on the engine's stream and waits for it).  -> dict of the launch: variant (one of
        WGRAD_VARIANTS), instance, ti, tj, lds_staged, strip_rows, cgroups, nstrips, piece_width, deterministic."""
        def dp(t):
            return None if t is None else int(t.data_ptr() if hasattr(t, "data_ptr") else t)
        a = WGRAD_LAYER(dp(X), dp(X1), dp(dY), dp(maskY), dp(dW), dp(dB), int(mode), int(KW), int(stride), int(bool(xup)),
                        int(bool(in_relu)), int(bool(logits)), int(XC0), int(XC1), int(ci0), int(Cin), int(Cout), int(Hx), int(Wx),
                        int((Wx >> int(bool(xup))) if xpitch is None else xpitch), int(Hy), int(Wy), int(slots), int(strip_rows))
        ran = WGRAD_PLAN()
        _check(lib().pseg_train_wgrad_layer(self._h, ctypes.byref(a), ctypes.byref(ran)))
        out = {n: int(getattr(ran, n)) for n, _ in WGRAD_PLAN._fields_}
        out["variant"] = WGRAD_VARIANTS[out["variant"]]
        return out

    def stream(self):
        """Raw hipStream_t (int) of the engine's own stream."""
        return int(lib().pseg_engine_stream(self._h) or 0)

    def flops_per_pixel(self):
        return float(lib().pseg_flops_per_pixel(self._h))

    # -- per-kernel timing (HIP events on the launch stream) -------------------------------------
    def timing_enable(self, on=True):
        _check(lib().pseg_timing_enable(self._h, int(bool(on))))

    def timing_reset(self):
        _check(lib().pseg_timing_reset(self._h))

    def timing(self):
        """[(layer, total_ms, launches, algorithmic_flops_per_launch)]"""
        L = lib()
        out = []
        name = ctypes.create_string_buffer(128)
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        for i in range(L.pseg_timing_num_slots(self._h)):
            _check(L.pseg_timing_get(self._h, i, name, 128, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
            out.append((name.value.decode(), ms.value, n.value, fl.value))
        return out


# -- post-process (host arrays) ----------------------------------------------------------------
def cc_vote(pred, binary, n_classes=0, device=0):
    """vote_connected_component_class (lib/postprocess.py:9-26); `pred` int64 is updated IN PLACE
    (as the reference does) and returned."""
    if pred.dtype != np.int64 or not pred.flags.c_contiguous:
        raise PsegError("pred must be a C-contiguous int64 array")
    b = np.ascontiguousarray(binary, dtype=np.uint8)
    if b.shape != pred.shape:
        raise PsegError("binary shape %r != pred shape %r" % (b.shape, pred.shape))
    H, W = pred.shape
    _check(lib().pseg_cc_vote(int(device), _ptr(pred), _ptr(b), H, W, int(n_classes)))
    return pred


def bbox_fill(pred, n_classes=0, device=0):
    p = np.ascontiguousarray(pred, dtype=np.int64)
    out = np.zeros_like(p)
    H, W = p.shape
    _check(lib().pseg_bbox_fill(int(device), _ptr(p), _ptr(out), H, W, int(n_classes)))
    return out


def masks(pred, binary, lut, device=0):
    """generate_output_masks (lib/output.py:44-60) -> (color, overlay, inverted, fg_color)."""
    p = np.ascontiguousarray(pred, dtype=np.int64)
    b = np.ascontiguousarray(binary, dtype=np.uint8)
    t = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
    H, W = p.shape
    outs = [np.empty((H, W, 3), np.uint8) for _ in range(4)]
    _check(lib().pseg_masks(int(device), _ptr(p), _ptr(b), _ptr(t), t.shape[0], H, W,
                            *[_ptr(o) for o in outs]))
    return tuple(outs)


# -- PNG output on the device (lib/output.py:20-41) -------------------------------------------------------------------
MASK_NAMES = ("color", "overlay", "inverted", "fg_color")


def png_bound(H, W, channels=3, band_rows=0, level=0):
    """Upper bound of the encoded size of an (H,W[,3]) image (pseg_png_bound_lv: arithmetic, no device)."""
    n = int(lib().pseg_png_bound_lv(int(H), int(W), int(channels), int(band_rows), int(level)))
    if n == 0:
        raise PsegError("png_bound: bad shape (%r, %r), channels %r, band_rows %r or level %r" % (H, W, channels, band_rows, level))
    return n


def png_code_lengths(counts, limit):
    """Code lengths of a prefix code of at most `limit` bits for the symbol counts (pseg_png_code_lengths: the host
    instantiation of the function the level-1 band kernel runs; arithmetic, no device) -> uint8 array, 0 where the count is 0."""
    cnt = np.ascontiguousarray(counts, dtype=np.uint32).ravel()
    out = np.zeros(cnt.size, np.uint8)
    _check(lib().pseg_png_code_lengths(_ptr(cnt), int(cnt.size), int(limit), _ptr(out)))
    return out


def _png_buffers(H, W, channels, band_rows, wanted, level=0):
    """Page-locked output buffers of the bound's size for the wanted streams + the ctypes arrays the C entries take."""
    n = png_bound(H, W, channels, band_rows, level)
    bufs = [pinned_empty_pooled((n,), np.uint8) if w else None for w in wanted]
    P = (ctypes.c_void_p * 4)(*[None if b is None else b.ctypes.data for b in bufs])
    caps = (ctypes.c_size_t * 4)(*[0 if b is None else n for b in bufs])
    return bufs, P, caps, (ctypes.c_size_t * 4)()


def png_encode(array, band_rows=0, device=0, level=0):
    """uint8 (H,W) or (H,W,3) -> the bytes of a PNG file (8-bit gray / truecolour), encoded on the GPU (pseg_png_encode_lv).
    level 0: fixed Huffman codes; level 1: a dynamic code per band where it is smaller (include/pseg.h)."""
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise PsegError("png_encode takes a non-empty uint8 (H,W) or (H,W,3) array, got %s %r" % (a.dtype, a.shape))
    a = np.ascontiguousarray(a)
    H, W = a.shape[:2]
    ch = 1 if a.ndim == 2 else 3
    L = lib()
    cap = int(L.pseg_png_bound_lv(H, W, ch, int(band_rows), int(level)))
    out = pinned_empty_pooled((max(cap, 1),), np.uint8)
    n = ctypes.c_size_t()
    _check(L.pseg_png_encode_lv(int(device), _ptr(a), H, W, ch, int(band_rows), int(level), _ptr(out), cap, ctypes.byref(n)))
    return out[:n.value].tobytes()


def masks_png(pred, binary, lut, which=("color", "overlay", "inverted"), band_rows=0, device=0, level=0):
    """generate_output_masks (lib/output.py:44-60) straight to PNG streams: {name: bytes} for the names in `which` (of "color",
    "overlay", "inverted", "fg_color"), each decoding to the array masks() returns (pseg_masks_png_lv; `level` as in png_encode)."""
    for w in which:
        if w not in MASK_NAMES:
            raise PsegError("unknown mask %r (one of %r)" % (w, MASK_NAMES))
    p = np.ascontiguousarray(pred, dtype=np.int64)
    b = np.ascontiguousarray(binary, dtype=np.uint8)
    t = np.ascontiguousarray(lut, dtype=np.uint8).reshape(-1, 3)
    if p.ndim != 2 or b.shape != p.shape or p.size == 0:
        raise PsegError("pred %r and binary %r must be non-empty (H,W) arrays of one shape" % (p.shape, b.shape))
    H, W = p.shape
    L = lib()
    bufs, P, caps, sizes = _png_buffers(H, W, 3, band_rows, [m in which for m in MASK_NAMES], level)
    _check(L.pseg_masks_png_lv(int(device), _ptr(p), _ptr(b), _ptr(t), t.shape[0], H, W, int(band_rows), int(level), P, caps, sizes))
    return {m: bufs[k][:sizes[k]].tobytes() for k, m in enumerate(MASK_NAMES) if m in which}


# ---- PNG scans decoded on the device (include/pseg.h) ---------------------------------

PNG_OK, PNG_EINVAL, PNG_EUNSUPPORTED = 0, -1, -5      # PSEG_OK, PSEG_EINVAL, PSEG_EUNSUPPORTED: the per-file statuses
PSEG_OK, PSEG_EHIP, PSEG_ENOMEM, PSEG_EUNSUPPORTED = 0, -3, -4, -5   # include/pseg.h: the per-map / per-page statuses of the text regions


def _file_ptr(data):
    """(address, length, keep-alive) of a bytes-like object, without a copy for bytes."""
    if isinstance(data, bytes):
        return ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value or 0, len(data), data
    a = np.frombuffer(data, dtype=np.uint8)
    return a.ctypes.data, a.size, a


def png_probe(data):
    """(status, H, W, channels) of a PNG file held in memory (pseg_png_probe; no device): PNG_OK for what png_decode_gray decodes
    (8-bit gray or RGB, no interlace, no tRNS), PNG_EUNSUPPORTED for every other sound PNG, PNG_EINVAL for a broken container.
    H, W, channels are 0 where no IHDR chunk could be read."""
    p, n, keep = _file_ptr(data)
    H, W, ch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    st = lib().pseg_png_probe(ctypes.c_void_p(p), n, ctypes.byref(H), ctypes.byref(W), ctypes.byref(ch))
    return int(st), H.value, W.value, ch.value


def png_decode_gray(files, device=0, host=False):
    """The gray scans of PNG files held in memory (bytes), as PIL's Image.open(f).convert("L"): a list of (array, status), the
    array in pooled page-locked memory, or None where the status is not PNG_OK (PNG_EUNSUPPORTED: a PNG this decoder does not take;
    PNG_EINVAL: a broken file) -- the other files of the list are unaffected.  Inflate and unfilter run on the device, one workgroup
    per file, 64 files or 64 MiB a group (pseg_png_decode_gray); host=True runs the same code serially on the host, no device."""
    files = list(files)
    n = len(files)
    L = lib()
    if n == 0:
        _check(L.pseg_png_decode_gray_host(0, None, None, None, None) if host else L.pseg_png_decode_gray(int(device), 0, None, None, None, None))
        return []
    refs = [_file_ptr(f) for f in files]
    outs = []
    for f in files:
        st, H, W, _ch = png_probe(f)
        outs.append(None if st != PNG_OK else np.empty((H, W), np.uint8) if host else pinned_empty_pooled((H, W), np.uint8))
    dummy = np.zeros(1, np.uint8)                    # a refused file's output pointer: never written
    ptrs = (ctypes.c_void_p * n)(*[r[0] for r in refs])
    lens = (ctypes.c_size_t * n)(*[r[1] for r in refs])
    optr = (ctypes.c_void_p * n)(*[(dummy if o is None else o).ctypes.data for o in outs])
    status = (ctypes.c_int * n)()
    if host:
        _check(L.pseg_png_decode_gray_host(n, ptrs, lens, optr, status))
    else:
        _check(L.pseg_png_decode_gray(int(device), n, ptrs, lens, optr, status))
    return [(outs[k] if status[k] == PNG_OK else None, int(status[k])) for k in range(n)]


def read_file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def decode_gray_files(paths, device=0, fallback=None, reads=None):
    """The gray scans of the files at `paths` through png_decode_gray: one entry per path, the array, or the exception that
    `fallback(path)` raised.  A file that cannot be read, and every file whose status is not PNG_OK, goes to fallback(path) (the
    callers pass their PIL read), so what comes back for such a file is the fallback's array or the fallback's exception.
    reads: futures of read_file_bytes(path), one per path, submitted to a pool BEFORE the task that runs this function (a pool
    runs its tasks in order, so the task never waits for a read queued behind it); None: the files are read here."""
    datas = []
    for k, path in enumerate(paths):
        try:
            datas.append(read_file_bytes(path) if reads is None else reads[k].result())
        except OSError:
            datas.append(None)
    known = [k for k, d in enumerate(datas) if d is not None]
    out = [None] * len(datas)
    for k, (arr, st) in zip(known, png_decode_gray([datas[k] for k in known], device=device)):
        out[k] = arr if st == PNG_OK else None
    for k, path in enumerate(paths):
        if out[k] is None:
            try:
                out[k] = np.ascontiguousarray(fallback(path), dtype=np.uint8)
            except BaseException as exc:
                out[k] = exc
    return out


def otsu_char_height(gray, inverse=False, device=0):
    """(char_height or None, otsu_threshold) -- lib/image_ops.py:58-82 without the file read."""
    g = np.ascontiguousarray(gray, dtype=np.uint8)
    H, W = g.shape
    h, t = ctypes.c_int(), ctypes.c_int()
    _check(lib().pseg_otsu_char_height(int(device), _ptr(g), H, W, int(bool(inverse)),
                                       ctypes.byref(h), ctypes.byref(t)))
    return (None if h.value < 0 else h.value), t.value


def char_heights(scans, inverse=False, device=0):
    """otsu_char_height for a list of gray scans in one device-resident call (pseg_char_heights): -> (heights, thresholds), two
    lists; heights[i] is an int or None.  The library cuts the list into groups of at most 64 scans / 64 MiB, three launches and
    one wait each."""
    gs = [np.ascontiguousarray(g, dtype=np.uint8) for g in scans]
    for k, g in enumerate(gs):
        if g.ndim != 2:
            raise PsegError("scan %d: an (H,W) gray array is expected, got shape %r" % (k, g.shape))
    n = len(gs)
    if n == 0:
        _check(lib().pseg_char_heights(int(device), 0, None, None, None, int(bool(inverse)), None, None))
        return [], []
    ptrs = (ctypes.c_void_p * n)(*[g.ctypes.data for g in gs])
    Hs = (ctypes.c_int * n)(*[g.shape[0] for g in gs])
    Ws = (ctypes.c_int * n)(*[g.shape[1] for g in gs])
    hs, ts = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    _check(lib().pseg_char_heights(int(device), n, ptrs, Hs, Ws, int(bool(inverse)), hs, ts))
    return [None if h < 0 else int(h) for h in hs], [int(t) for t in ts]


def char_height_window():
    """(tile_h, tile_w, above, below, left, right) of pseg_char_heights' window kernel (pseg_char_height_window; no device)."""
    v = [ctypes.c_int() for _ in range(6)]
    _check(lib().pseg_char_height_window(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def char_height_median(bins, first):
    """The upper median pseg_char_heights takes from its height bins (bins[k]: components of height first + k), or None."""
    b = np.ascontiguousarray(bins, dtype=np.uint32)
    h = ctypes.c_int()
    _check(lib().pseg_char_height_median(_ptr(b), int(b.size), int(first), ctypes.byref(h)))
    return None if h.value < 0 else h.value


# ---- line-height normalisation (lib/dataset.py:114-150, lib/util.py:21-29) --------------------------

def rescale_shape(shape, scale):
    """np.round(scale * shape) of skimage.transform.rescale (half to even)."""
    ho, wo = ctypes.c_int(), ctypes.c_int()
    _check(lib().pseg_rescale_shape(int(shape[0]), int(shape[1]), float(scale), ctypes.byref(ho), ctypes.byref(wo)))
    return ho.value, wo.value


def aa_kernels(in_shape, out_shape):
    """The per-axis anti-aliasing kernels exactly as scipy.ndimage.gaussian_filter builds them with
    this process's NumPy (host set-up arithmetic: a dozen numbers per axis).  -> [(w or None, radius)] x 2."""
    out = []
    for n_in, n_out in zip(in_shape[:2], out_shape[:2]):
        sigma = max(0.0, (float(n_in) / float(n_out) - 1) / 2)
        if sigma <= 1e-15:
            out.append((None, 0))
            continue
        radius = int(4.0 * sigma + 0.5)
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        out.append((np.ascontiguousarray((phi / phi.sum())[::-1], dtype=np.float64), radius))
    return out


def _kptr(k):
    return _ptr(k[0]) if k[0] is not None else None


def resize_nearest(image, out_shape, device=0):
    """Order-0 resize that keeps values and dtype (gather on the GPU); (H,W) or (H,W,C) arrays."""
    a = np.ascontiguousarray(image)
    H, W = a.shape[:2]
    Ho, Wo = int(out_shape[0]), int(out_shape[1])
    eb = a.itemsize * int(np.prod(a.shape[2:], dtype=np.int64))
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    out = np.empty((Ho, Wo) + a.shape[2:], a.dtype)
    _check(lib().pseg_resize_nearest(int(device), _ptr(a), H, W, eb, _ptr(out), Ho, Wo))
    return out


def scale_image(image, out_shape, device=0):
    """scale_image (lib/dataset.py:122-128) -> float64 (Ho,Wo)."""
    a = np.asarray(image)
    f64 = a.dtype != np.uint8
    a = np.ascontiguousarray(a, dtype=np.float64 if f64 else np.uint8)
    H, W = a.shape
    Ho, Wo = int(out_shape[0]), int(out_shape[1])
    ky, kx = aa_kernels((H, W), (Ho, Wo))
    out = np.empty((Ho, Wo), np.float64)
    _check(lib().pseg_scale_image(int(device), _ptr(a), int(f64), H, W, _ptr(out), Ho, Wo,
                                  _kptr(ky), ky[1], _kptr(kx), kx[1]))
    return out


def prepare_images(image, binary, scale, max_width=None, device=0, want_stage1=False):
    """prepare_images (lib/dataset.py:131-150) -> (img uint8, bin uint8, orig_bin uint8[, stage1])."""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    b = np.ascontiguousarray(binary, dtype=np.uint8)
    if img.ndim != 2 or img.shape != b.shape:
        raise PsegError("image and binary must be 2-D arrays of one shape, got %s and %s" % (img.shape, b.shape))
    H0, W0 = img.shape
    H1, W1 = rescale_shape((H0, W0), scale)
    H2 = W2 = 0
    if max_width is not None:
        n_scale = max_width / W1
        if n_scale < 1.0:
            H2, W2 = rescale_shape((H1, W1), n_scale)
    k1 = aa_kernels((H0, W0), (H1, W1))
    k2 = aa_kernels((H1, W1), (H2, W2)) if H2 else [(None, 0), (None, 0)]
    Hf, Wf = (H2, W2) if H2 else (H1, W1)
    o_img, o_bin = np.empty((Hf, Wf), np.uint8), np.empty((Hf, Wf), np.uint8)
    o_orig = np.empty((H0, W0), np.uint8)
    st1 = np.empty((H1, W1), np.float64) if want_stage1 else None
    _check(lib().pseg_prepare_images(int(device), _ptr(img), _ptr(b), H0, W0, H1, W1,
                                     _kptr(k1[0]), k1[0][1], _kptr(k1[1]), k1[1][1], H2, W2,
                                     _kptr(k2[0]), k2[0][1], _kptr(k2[1]), k2[1][1],
                                     _ptr(o_img), _ptr(o_bin), _ptr(o_orig), _ptr(st1) if st1 is not None else None))
    return (o_img, o_bin, o_orig, st1) if want_stage1 else (o_img, o_bin, o_orig)


def scan_plan(shape, scale):
    """What the scan entries are told about one scan: (H, W, (wy or None, ry), (wx or None, rx)) -- the page's shape
    (rescale_shape) and the per-axis anti-aliasing kernels (aa_kernels).  Host arithmetic."""
    H, W = rescale_shape(shape, scale)
    if H <= 0 or W <= 0:
        raise PsegError("scale %r leaves no page of a %r scan" % (scale, tuple(shape)))
    ky, kx = aa_kernels(shape, (H, W))
    return H, W, ky, kx


def scan_table(scans, scales, high_res=False):
    """The pseg_scan array of a list of gray scans -> (table, scans as contiguous uint8 arrays, plans); the table points into the
    arrays and the plans' kernels: keep all three alive while it is in use."""
    arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in scans]
    if len(arrs) != len(scales):
        raise PsegError("scales must have one entry per scan")
    if any(a.ndim != 2 for a in arrs):
        raise PsegError("scans must be 2-D uint8 arrays")
    plans = [scan_plan(a.shape, float(sc)) for a, sc in zip(arrs, scales)]
    table = (SCAN * max(len(arrs), 1))()
    for k, (a, (H, W, ky, kx)) in enumerate(zip(arrs, plans)):
        table[k] = SCAN(a.ctypes.data, a.shape[0], a.shape[1], H, W, None if ky[0] is None else ky[0].ctypes.data, ky[1],
                        None if kx[0] is None else kx[0].ctypes.data, kx[1], 1 if high_res else 0)
    return table, arrs, plans


def prepare_scans(scans, scales, device=0, binarize=None, despeckle=None):
    """prepare_images(scan, where(scan > 127, 255, 0), scale) for a list of gray scans in one call of the scan chain's front end
    (pseg_prepare_scans) -> [(img uint8, bin uint8, orig_bin uint8)], bit for bit.  binarize: None, a Sauvola with a window, or one of
    either per scan (binarize_table): prepare_images(scan, where(ink, 0, 255), scale) with ink from binarize_scans
    (pseg_prepare_scans_bin).  despeckle: None, a Despeckle with its max_area, or one of either per scan (despeckle_table): the ink
    map loses its specks first, prepare_images(scan, where(despeckle_maps(ink), 0, 255), scale) (pseg_prepare_scans_clean)."""
    table, arrs, plans = scan_table(scans, scales)
    n = len(arrs)
    how = None if binarize is None else binarize_table(binarize, n)
    out = [(np.empty(p[:2], np.uint8), np.empty(p[:2], np.uint8), np.empty(a.shape, np.uint8)) for a, p in zip(arrs, plans)]
    P = ctypes.c_void_p * max(n, 1)
    if despeckle is not None:
        dsp = despeckle_table(despeckle, n, "scan")
        _check(lib().pseg_prepare_scans_clean(int(device), n, table, how, dsp, *[P(*[o[k].ctypes.data for o in out]) for k in range(3)]))
        return out
    _check(lib().pseg_prepare_scans_bin(int(device), n, table, how, *[P(*[o[k].ctypes.data for o in out]) for k in range(3)]))
    return out


# ---- adaptive binarisation (pseg_binarize_scans) ------------------------------------------------------

def sauvola_window(line_height_px):
    """The window Sauvola(window=None) takes for a scan of this line height: two line heights and the centre pixel, at most 255.
    Host arithmetic."""
    if line_height_px is None or not np.isfinite(line_height_px) or line_height_px <= 0:
        raise PsegError("sauvola_window needs a positive line height, got %r" % (line_height_px,))
    return min(255, 2 * max(1, int(round(line_height_px))) + 1)


class Sauvola:
    """Sauvola's adaptive threshold over a square window of odd side `window` (3 .. 255): T = m (1 + k (s / R - 1)) from the
    window's mean m and standard deviation s, ink = value <= T (include/pseg.h, pseg_binarize).  window=None: sauvola_window of the
    scan's line height, for the callers that know it (resolved)."""

    def __init__(self, window=None, k=0.2, R=128.0):
        if window is not None:
            if isinstance(window, bool) or int(window) != window:
                raise PsegError("Sauvola: window must be an odd integer in 3..255 or None, got %r" % (window,))
            window = int(window)
            if window < 3 or window > 255 or window % 2 == 0:
                raise PsegError("Sauvola: window must be an odd integer in 3..255 or None, got %r" % (window,))
        k, R = float(k), float(R)
        if not 0.0 <= k <= 1.0:
            raise PsegError("Sauvola: k must lie in [0, 1], got %r" % (k,))
        if not (R > 0.0 and np.isfinite(R)):
            raise PsegError("Sauvola: R must be a positive number, got %r" % (R,))
        self.window, self.k, self.R = window, k, R

    def resolved(self, line_height_px):
        """This threshold with its window fixed for a scan of the given line height."""
        return self if self.window is not None else Sauvola(sauvola_window(line_height_px), self.k, self.R)

    def __repr__(self):
        return "Sauvola(window=%r, k=%r, R=%r)" % (self.window, self.k, self.R)

    def __eq__(self, other):
        return isinstance(other, Sauvola) and (self.window, self.k, self.R) == (other.window, other.k, other.R)

    def __hash__(self):
        return hash((self.window, self.k, self.R))


def binarize_geometry():
    """(segment, band, tile, vector) of pseg_binarize_scans' kernels (pseg_binarize_geometry; no device)."""
    v = [ctypes.c_int() for _ in range(4)]
    _check(lib().pseg_binarize_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def binarize_table(how, n):
    """The pseg_binarize array of n scans: how is a Sauvola for all of them, or a sequence with a Sauvola or None (the fixed
    threshold, ink = scan <= 127) per scan.  Every Sauvola must have its window (Sauvola.resolved)."""
    entries = [how] * n if how is None or isinstance(how, Sauvola) else list(how)
    if len(entries) != n:
        raise PsegError("binarize must have one entry per scan (%d for %d scans)" % (len(entries), n))
    table = (BINARIZE * max(n, 1))()
    for k, b in enumerate(entries):
        if b is None:
            table[k] = BINARIZE(0, 0.0, 0.0)
            continue
        if not isinstance(b, Sauvola):
            raise PsegError("scan %d: binarize takes None or a Sauvola, got %r" % (k, b))
        if b.window is None:
            raise PsegError("scan %d: Sauvola(window=None) needs the scan's line height: pass Sauvola.resolved(line_height_px)" % k)
        table[k] = BINARIZE(b.window, b.k, b.R)
    return table


def binarize_scans(scans, how, device=0, thresholds=False, host=False):
    """The ink maps (uint8, ink = 1) of a list of gray scans in one device-resident call (pseg_binarize_scans): how is a Sauvola or
    one per scan (None: ink = scan <= 127), see binarize_table.  thresholds=True: -> [(ink, T)] with the float64 threshold of
    every pixel.  host=True: the same bits from the host entry (pseg_binarize_scans_host), no device."""
    gs = [np.ascontiguousarray(g, dtype=np.uint8) for g in scans]
    for k, g in enumerate(gs):
        if g.ndim != 2:
            raise PsegError("scan %d: an (H,W) gray array is expected, got shape %r" % (k, g.shape))
    n = len(gs)
    table = binarize_table(how, n)
    if n == 0:
        return []
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    inks = [np.empty(g.shape, np.uint8) for g in gs]
    thr = [np.empty(g.shape, np.float64) for g in gs] if thresholds else None
    args = (n, P(*[g.ctypes.data for g in gs]), I(*[g.shape[0] for g in gs]), I(*[g.shape[1] for g in gs]), table,
            P(*[a.ctypes.data for a in inks]), None if thr is None else P(*[a.ctypes.data for a in thr]))
    _check(lib().pseg_binarize_scans_host(*args) if host else lib().pseg_binarize_scans(int(device), *args))
    return list(zip(inks, thr)) if thresholds else inks


# ---- despeckling of ink maps (pseg_despeckle_maps) -------------------------------------------------------

DESPECKLE_AREA_MAX = 1 << 24


def despeckle_area(line_height_px):
    """The max_area Despeckle(max_area=None) takes for a scan of this line height: the square of an eighth of the line height, at
    least 1.  A convention (a full stop, about a fifth of the line height across, survives it), not a measured optimum.  Host
    arithmetic."""
    if line_height_px is None or not np.isfinite(line_height_px) or line_height_px <= 0:
        raise PsegError("despeckle_area needs a positive line height, got %r" % (line_height_px,))
    return max(1, int(round(line_height_px)) // 8) ** 2


class Despeckle:
    """Erase every ink component (connectivity 4 or 8) of at most max_area pixels, 1 .. 16 777 216 (include/pseg.h,
    pseg_despeckle).  max_area=None: despeckle_area of the scan's line height, for the callers that know it (resolved)."""

    def __init__(self, max_area=None, connectivity=8):
        if max_area is not None:
            if isinstance(max_area, bool) or int(max_area) != max_area:
                raise PsegError("Despeckle: max_area must be an integer in 1..%d or None, got %r" % (DESPECKLE_AREA_MAX, max_area))
            max_area = int(max_area)
            if max_area < 1 or max_area > DESPECKLE_AREA_MAX:
                raise PsegError("Despeckle: max_area must be an integer in 1..%d or None, got %r" % (DESPECKLE_AREA_MAX, max_area))
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise PsegError("Despeckle: connectivity must be 4 or 8, got %r" % (connectivity,))
        self.max_area, self.connectivity = max_area, int(connectivity)

    def resolved(self, line_height_px):
        """This despeckling with its max_area fixed for a scan of the given line height."""
        return self if self.max_area is not None else Despeckle(min(DESPECKLE_AREA_MAX, despeckle_area(line_height_px)), self.connectivity)

    def __repr__(self):
        return "Despeckle(max_area=%r, connectivity=%r)" % (self.max_area, self.connectivity)

    def __eq__(self, other):
        return isinstance(other, Despeckle) and (self.max_area, self.connectivity) == (other.max_area, other.connectivity)

    def __hash__(self):
        return hash((self.max_area, self.connectivity))


def despeckle_geometry():
    """(tile_h, tile_w, slots, run_cap) of pseg_despeckle_maps' kernels (pseg_despeckle_geometry; no device)."""
    v = [ctypes.c_int() for _ in range(4)]
    _check(lib().pseg_despeckle_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def despeckle_table(how, n, what="map"):
    """The pseg_despeckle array of n maps: how is a Despeckle for all of them, or a sequence with a Despeckle or None (the map is
    not despeckled) per map.  Every Despeckle must have its max_area (Despeckle.resolved).  what: the word the messages use."""
    entries = [how] * n if how is None or isinstance(how, Despeckle) else list(how)
    if len(entries) != n:
        raise PsegError("despeckle must have one entry per %s (%d for %d %ss)" % (what, len(entries), n, what))
    table = (DESPECKLE * max(n, 1))()
    for k, d in enumerate(entries):
        if d is None:
            table[k] = DESPECKLE(0, 8)
            continue
        if not isinstance(d, Despeckle):
            raise PsegError("%s %d: despeckle takes None or a Despeckle, got %r" % (what, k, d))
        if d.max_area is None:
            raise PsegError("%s %d: Despeckle(max_area=None) needs the scan's line height: pass Despeckle.resolved(line_height_px)" % (what, k))
        table[k] = DESPECKLE(d.max_area, d.connectivity)
    return table


def despeckle_maps(maps, how, device=0, counts=False, host=False):
    """A list of ink maps (uint8, non-zero = ink) without their specks in one device-resident call (pseg_despeckle_maps): how is a
    Despeckle or one per map (None: the map comes back as it is), see despeckle_table.  Kept ink is 1.  counts=True:
    -> (maps, int64 (n, 3)) with the components erased, the pixels erased and the components kept of every map.  host=True: the
    same bytes from the host entry (pseg_despeckle_maps_host), no device."""
    ms = [np.ascontiguousarray(m, dtype=np.uint8) for m in maps]
    for k, m in enumerate(ms):
        if m.ndim != 2:
            raise PsegError("map %d: an (H,W) ink map is expected, got shape %r" % (k, m.shape))
    n = len(ms)
    table = despeckle_table(how, n)
    cnt = np.zeros((n, 3), np.int64)
    if n == 0:
        return ([], cnt) if counts else []
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    outs = [np.empty(m.shape, np.uint8) for m in ms]
    args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
            P(*[a.ctypes.data for a in outs]), cnt.ctypes.data if counts else None)
    _check(lib().pseg_despeckle_maps_host(*args) if host else lib().pseg_despeckle_maps(int(device), *args))
    return (outs, cnt) if counts else outs


# ---- deskewing: the skew of ink maps from strip profiles, an exact rotation (pseg_skew_maps, pseg_rotate_maps) ----------------

SKEW_DENOM_MIN, SKEW_DENOM_MAX, SKEW_STEPS_MAX = 64, 4096, 128


def _skew_int(v, what, name):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise PsegError("%s: %s must be an integer, got %r" % (what, name, v))
    return int(v)


class Skew:
    """How a page's skew is searched (include/pseg.h, pseg_skew): slopes index / denom for index = -steps .. steps, with
    steps = floor(tan(radians(max_degrees)) * denom) clamped to 1 .. min(128, denom // 4).  denom: 64 .. 4096; max_degrees: a finite
    angle above 0 and below 90.  One step of the default is 0.056 degrees."""

    def __init__(self, max_degrees=5.0, denom=1024):
        denom = _skew_int(denom, "Skew", "denom")
        if not SKEW_DENOM_MIN <= denom <= SKEW_DENOM_MAX:
            raise PsegError("Skew: denom must lie in %d..%d, got %r" % (SKEW_DENOM_MIN, SKEW_DENOM_MAX, denom))
        if isinstance(max_degrees, bool) or not isinstance(max_degrees, (int, float, np.integer, np.floating)) \
                or not np.isfinite(max_degrees) or not 0 < max_degrees < 90:
            raise PsegError("Skew: max_degrees must be a finite angle above 0 and below 90, got %r" % (max_degrees,))
        self.max_degrees, self.denom = float(max_degrees), denom
        self.steps = int(min(max(np.floor(np.tan(np.radians(self.max_degrees)) * denom), 1), SKEW_STEPS_MAX, denom // 4))

    def __repr__(self):
        return "Skew(max_degrees=%r, denom=%r)" % (self.max_degrees, self.denom)

    def __eq__(self, other):
        return isinstance(other, Skew) and (self.steps, self.denom) == (other.steps, other.denom)

    def __hash__(self):
        return hash((self.steps, self.denom))


def skew_degrees(index, denom):
    """The angle of slope index / denom in degrees.  Host arithmetic."""
    return float(np.degrees(np.arctan2(float(index), float(denom))))


def skew_geometry():
    """(strip, max_steps, max_side) of the skew contract (pseg_skew_geometry; no device)."""
    v = [ctypes.c_int() for _ in range(3)]
    _check(lib().pseg_skew_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _skew_table(how, n, what="map"):
    entries = [how] * n if isinstance(how, Skew) else list(how) if isinstance(how, (list, tuple)) else None
    if entries is None:
        raise PsegError("a Skew or one per %s is expected, got %r" % (what, how))
    if len(entries) != n:
        raise PsegError("skew must have one entry per %s (%d for %d %ss)" % (what, len(entries), n, what))
    table = (SKEW * max(n, 1))()
    for k, s in enumerate(entries):
        if not isinstance(s, Skew):
            raise PsegError("%s %d: a Skew is expected, got %r" % (what, k, s))
        table[k] = SKEW(s.steps, s.denom)
    return table, entries


def _skew_maps2d(maps, what="map"):
    ms = [np.ascontiguousarray(m, dtype=np.uint8) for m in maps]
    for k, m in enumerate(ms):
        if m.ndim != 2:
            raise PsegError("%s %d: an (H,W) map is expected, got shape %r" % (what, k, m.shape))
    return ms


def skew_maps(maps, how, device=0, scores=False, host=False):
    """The skew indices (int32, slope index / how.denom) of a list of ink maps (uint8, non-zero = ink) in one device-resident call
    (pseg_skew_maps); how is a Skew or one per map.  scores=True: -> (indices, [uint64 (2 steps + 1,) per map]).  host=True: the same
    numbers from the host entry (pseg_skew_maps_host), no device."""
    ms = _skew_maps2d(maps)
    n = len(ms)
    table, entries = _skew_table(how, n)
    idx = np.zeros(n, np.int32)
    sc = [np.zeros(2 * s.steps + 1, np.uint64) for s in entries] if scores else []
    if n:
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
                idx.ctypes.data, P(*[a.ctypes.data for a in sc]) if scores else None)
        _check(lib().pseg_skew_maps_host(*args) if host else lib().pseg_skew_maps(int(device), *args))
    return (idx, sc) if scores else idx


def rotate_maps(maps, indices, denom=1024, order=0, fill=0, device=0, host=False):
    """A list of uint8 maps turned about their centres by the slopes indices[i] / denom (pseg_rotate_maps): rotating by the index
    skew_maps gave makes the text lines horizontal, rotating by its negative maps a result back.  order 0 (nearest; label maps) or 1
    (bilinear); fill: the byte outside the map.  indices: one integer for all maps or one per map.  host=True: the same bytes from
    the host entry, no device."""
    ms = _skew_maps2d(maps)
    n = len(ms)
    ind = [indices] * n if isinstance(indices, (int, np.integer)) and not isinstance(indices, bool) else list(indices)
    if len(ind) != n:
        raise PsegError("rotate_maps: one index per map (%d for %d maps)" % (len(ind), n))
    denom, order, fill = _skew_int(denom, "rotate_maps", "denom"), _skew_int(order, "rotate_maps", "order"), _skew_int(fill, "rotate_maps", "fill")
    table = (ROTATE * max(n, 1))()
    for k, a in enumerate(ind):
        table[k] = ROTATE(_skew_int(a, "map %d" % k, "index"), denom, order, fill)
    outs = [np.empty(m.shape, np.uint8) for m in ms]
    if n:
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
                P(*[a.ctypes.data for a in outs]))
        _check(lib().pseg_rotate_maps_host(*args) if host else lib().pseg_rotate_maps(int(device), *args))
    return outs


def deskew_scans(scans, how, inks=None, device=0, host=False):
    """A list of gray scans (uint8) deskewed in one device-resident call (pseg_deskew_scans): the skew is estimated on scan <= 127
    -- or on inks[i] (non-zero = ink) where given; inks is None or has an ink map or None per scan --, and the scan is rotated by the
    winner, order 1, fill 255, without a host wait in between.  -> (scans, int32 indices).  host=True: the same bytes from the host
    entry, no device."""
    gs = _skew_maps2d(scans, "scan")
    n = len(gs)
    table, _ = _skew_table(how, n, "scan")
    ks = None
    if inks is not None:
        ks = [None if m is None else np.ascontiguousarray(m, dtype=np.uint8) for m in inks]
        if len(ks) != n:
            raise PsegError("deskew_scans: one ink map (or None) per scan (%d for %d scans)" % (len(ks), n))
        for k, m in enumerate(ks):
            if m is not None and m.shape != gs[k].shape:
                raise PsegError("scan %d: the ink map's shape %r is not the scan's %r" % (k, m.shape, gs[k].shape))
    idx = np.zeros(n, np.int32)
    outs = [np.empty(g.shape, np.uint8) for g in gs]
    if n:
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        args = (n, P(*[g.ctypes.data for g in gs]), None if ks is None else P(*[None if m is None else m.ctypes.data for m in ks]),
                I(*[g.shape[0] for g in gs]), I(*[g.shape[1] for g in gs]), table, P(*[a.ctypes.data for a in outs]), idx.ctypes.data)
        _check(lib().pseg_deskew_scans_host(*args) if host else lib().pseg_deskew_scans(int(device), *args))
    return outs, idx


# ---- text regions from label maps (pseg_text_regions) -----------------------------------------------------

REGION_SIDE_MAX = 255


def region_kernels(ch):
    """The sides of the three rectangles for a line height ch: (int(ch), int(ch / 3), int(ch / 1.1)), each clamped to 1..255 (a side
    of 1 is the identity; the reference fails below a line height of 3).  Host arithmetic."""
    if ch is None or isinstance(ch, bool) or not np.isfinite(ch) or ch < 0:
        raise PsegError("region_kernels needs a non-negative line height, got %r" % (ch,))
    return tuple(min(REGION_SIDE_MAX, max(1, int(v))) for v in (ch, ch / 3, ch / 1.1))


class TextRegions:
    """How a label map becomes text regions (include/pseg.h, pseg_regions): the label id, 0..255, and either the page's line height
    (char_height: the sides are region_kernels of it) or the three sides themselves (kernels, each 1..255)."""

    def __init__(self, label, char_height=None, kernels=None):
        if isinstance(label, bool) or not isinstance(label, (int, np.integer)) or not 0 <= int(label) <= 255:
            raise PsegError("TextRegions: label must be an integer in 0..255, got %r" % (label,))
        if (char_height is None) == (kernels is None):
            raise PsegError("TextRegions takes either char_height or kernels")
        if kernels is None:
            kernels = region_kernels(char_height)
        else:
            kernels = tuple(kernels)
            if len(kernels) != 3 or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= REGION_SIDE_MAX
                                        for k in kernels):
                raise PsegError("TextRegions: kernels must be three integers in 1..%d, got %r" % (REGION_SIDE_MAX, kernels))
        self.label, self.kernels = int(label), tuple(int(k) for k in kernels)

    def __repr__(self):
        return "TextRegions(label=%r, kernels=%r)" % (self.label, self.kernels)

    def __eq__(self, other):
        return isinstance(other, TextRegions) and (self.label, self.kernels) == (other.label, other.kernels)

    def __hash__(self):
        return hash((self.label, self.kernels))


def regions_table(regions, n, what="page"):
    """A TextRegions, or one per page, as the C table of the chain's regions stage."""
    entries = [regions] * n if isinstance(regions, TextRegions) else list(regions)
    if len(entries) != n:
        raise PsegError("regions must have one entry per %s (%d for %d)" % (what, len(entries), n))
    for k, e in enumerate(entries):
        if not isinstance(e, TextRegions):
            raise PsegError("%s %d: regions takes a TextRegions, got %r" % (what, k, e))
    return (REGIONS * max(n, 1))(*[REGIONS(e.label, *e.kernels) for e in entries])


def regions_of_blob(blob):
    """One page's blob of the chain's regions stage (include/pseg.h, pseg_predict_chain_pages_regions_png; int32) as a record: "boxes",
    "areas", "seeds", "polygons" (None unless status is 0) and "status"."""
    r, v, status = int(blob[0]), int(blob[1]), int(blob[2])
    have_rows = blob.size >= 4 + 8 * r and (status == 0 or blob.size > 4)
    rows = blob[4:4 + 8 * r].reshape(r, 8) if have_rows else np.zeros((0, 8), np.int32)
    polys = None
    if status == 0:
        first = blob[4 + 8 * r:4 + 8 * r + r + 1]
        xy = blob[4 + 9 * r + 1:4 + 9 * r + 1 + 2 * v].reshape(v, 2)
        polys = [xy[first[j]:first[j + 1]].copy() for j in range(r)]
    return {"boxes": rows[:, 0:4].copy(), "areas": rows[:, 4].copy(), "seeds": rows[:, 5:7].copy(), "polygons": polys, "status": status}


def regions_geometry():
    """(word, band, band_words, tile_h, tile_w, slots) of pseg_text_regions' kernels (pseg_regions_geometry; no device)."""
    v = [ctypes.c_int() for _ in range(6)]
    _check(lib().pseg_regions_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _regions_call(ms, entries, device, masks, max_regions, host):
    n = len(ms)
    table = (REGIONS * n)(*[REGIONS(e.label, *e.kernels) for e in entries])
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    outs = [np.empty(m.shape, np.uint8) for m in ms] if masks else None
    rows = np.zeros((n, max_regions, 8), np.int32)
    cnt = np.zeros(n, np.int32)
    args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
            P(*[a.ctypes.data for a in outs]) if masks else None, int(max_regions), rows.ctypes.data if max_regions else None, cnt.ctypes.data)
    _check(lib().pseg_text_regions_host(*args) if host else lib().pseg_text_regions(int(device), *args))
    return outs, rows, cnt


def _regions_poly_call(ms, entries, device, masks, max_regions, host):
    """_regions_call with the polygons (pseg_text_regions_poly / _host): -> outs, rows, cnt, polys; polys[k] is the list of (v,2) int32
    arrays of map k, or None where the map has more than max_regions regions.  One retry with the needed capacity."""
    n = len(ms)
    table = (REGIONS * n)(*[REGIONS(e.label, *e.kernels) for e in entries])
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    cap = 1024 * n
    for _ in range(2):
        outs = [np.empty(m.shape, np.uint8) for m in ms] if masks else None
        rows = np.zeros((n, max_regions, 8), np.int32)
        cnt = np.zeros(n, np.int32)
        xy = np.zeros((cap, 2), np.int32)
        first = np.zeros((n, max_regions + 1), np.int64)
        status = np.zeros(n, np.int32)
        args = (n, P(*[m.ctypes.data for m in ms]), I(*[m.shape[0] for m in ms]), I(*[m.shape[1] for m in ms]), table,
                P(*[a.ctypes.data for a in outs]) if masks else None, int(max_regions), rows.ctypes.data if max_regions else None,
                cnt.ctypes.data, xy.ctypes.data, cap, first.ctypes.data, status.ctypes.data)
        _check(lib().pseg_text_regions_poly_host(*args) if host else lib().pseg_text_regions_poly(int(device), *args))
        if first[n - 1, max_regions] <= cap:
            break
        cap = int(first[n - 1, max_regions])
    polys = []
    for k in range(n):
        if status[k] == PSEG_EUNSUPPORTED:                # more regions than max_regions
            polys.append(None)
            continue
        if status[k] != 0:
            raise PsegError("map %d: a region's boundary walk did not close (status %d)" % (k, int(status[k])))
        polys.append([xy[first[k, r]:first[k, r + 1]].copy() for r in range(int(cnt[k]))])
    return outs, rows, cnt, polys


def text_regions(label_maps, how, device=0, masks=True, max_regions=256, host=False, polygons=False):
    """The text regions of a list of label maps (uint8 (H,W)) in one device-resident call (pseg_text_regions): how is a TextRegions
    or one per map.  -> one dict per map: "mask" (uint8 (H,W), 1 = region; None with masks=False), "boxes" (r,4) int32 x0, y0, x1, y1
    (exclusive), "areas" (r,) int32, "seeds" (r,2) int32 (y, x) -- the region's first pixel in raster order, by which the rows are
    sorted.  A map with more than max_regions regions is run again alone with max_regions = its count.  host=True: the same bytes from
    the host entry (pseg_text_regions_host), no device.  polygons=True: every record also has "polygons", a list of (v,2) int32 arrays of
    (x, y) pixel corners -- trace_regions' polygons, traced on the device from the bit planes in the same call
    (pseg_text_regions_poly; with host=True its host twin)."""
    ms = [np.ascontiguousarray(m, dtype=np.uint8) for m in label_maps]
    for k, m in enumerate(ms):
        if m.ndim != 2:
            raise PsegError("map %d: an (H,W) label map is expected, got shape %r" % (k, m.shape))
    n = len(ms)
    entries = [how] * n if isinstance(how, TextRegions) else list(how)
    if len(entries) != n:
        raise PsegError("text_regions must have one entry per map (%d for %d maps)" % (len(entries), n))
    for k, e in enumerate(entries):
        if not isinstance(e, TextRegions):
            raise PsegError("map %d: text_regions takes a TextRegions, got %r" % (k, e))
    if isinstance(max_regions, bool) or int(max_regions) != max_regions or max_regions < 0:
        raise PsegError("text_regions: max_regions must be a non-negative integer, got %r" % (max_regions,))
    if n == 0:
        return []
    polys = None
    if polygons:
        outs, rows, cnt, polys = _regions_poly_call(ms, entries, device, masks, int(max_regions), host)
    else:
        outs, rows, cnt = _regions_call(ms, entries, device, masks, int(max_regions), host)
    res = []
    for k in range(n):
        r, c = rows[k], int(cnt[k])
        pk = polys[k] if polygons else None
        if c > max_regions:
            if polygons:
                _, r1, c1, p1 = _regions_poly_call([ms[k]], [entries[k]], device, False, c, host)
                pk = p1[0]
            else:
                _, r1, c1 = _regions_call([ms[k]], [entries[k]], device, False, c, host)
            r, c = r1[0], int(c1[0])
        r = r[:c]
        res.append({"mask": outs[k] if masks else None, "boxes": r[:, 0:4].copy(), "areas": r[:, 4].copy(), "seeds": r[:, 5:7].copy()})
        if polygons:
            res[-1]["polygons"] = pk
    return res


def trace_regions(mask, record):
    """The crack polygons of the regions of one text_regions record on its mask (pseg_trace_regions_host; host only): a list of (v,2)
    int32 arrays of (x, y) pixel corners, clockwise from the seed's top-left corner, direction changes only."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.ndim != 2:
        raise PsegError("trace_regions: an (H,W) mask is expected, got shape %r" % (m.shape,))
    seeds = np.asarray(record["seeds"], np.int32).reshape(-1, 2)
    r = seeds.shape[0]
    table = np.zeros((max(r, 1), 8), np.int32)
    table[:r, 5:7] = seeds
    first = np.zeros(r + 1, np.int64)
    cap = 64 * max(r, 1)
    for _ in range(2):
        xy = np.zeros((cap, 2), np.int32)
        first[:] = 0
        _check(lib().pseg_trace_regions_host(m.ctypes.data, m.shape[0], m.shape[1], r, table.ctypes.data, xy.ctypes.data, cap, first.ctypes.data))
        if first[r] <= cap:
            break
        cap = int(first[r])
    return [xy[first[i]:first[i + 1]].copy() for i in range(r)]


# ---- training masks as label maps (pseg_label_masks) ----------------------------------------------------

def label_masks_geometry():
    """(run, runs, rows, group_masks, group_bytes) of pseg_label_masks (pseg_label_masks_geometry; no device): pixels per thread,
    runs and rows per workgroup, and the group cut."""
    v = [ctypes.c_int() for _ in range(4)] + [ctypes.c_int64()]
    _check(lib().pseg_label_masks_geometry(*[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def color_table(colors, ids):
    """The checked table of label_masks: -> (colors (n,3) uint8, ids (n,) uint8).  More than 256 colours, a colour channel or an id
    outside 0..255, or a duplicate colour raises."""
    col = np.asarray(colors if len(colors) else np.zeros((0, 3), np.uint8))
    idv = np.asarray(ids if len(ids) else np.zeros((0,), np.uint8))
    if col.ndim != 2 or col.shape[1] != 3 or idv.ndim != 1 or idv.shape[0] != col.shape[0]:
        raise PsegError("label_masks: colors must be (n,3) and ids (n,), got shapes %r and %r" % (col.shape, idv.shape))
    if col.shape[0] > 256:
        raise PsegError("label_masks: %d colours, at most 256 fit the table" % col.shape[0])
    for name, a in (("colour channel", col), ("id", idv)):
        if a.size and (a.dtype.kind not in "iub" or int(a.min()) < 0 or int(a.max()) > 255):
            raise PsegError("label_masks: every %s must be an integer in 0..255" % name)
    col, idv = np.ascontiguousarray(col, dtype=np.uint8), np.ascontiguousarray(idv, dtype=np.uint8)
    seen = {}
    for k, rgb in enumerate(map(tuple, col.tolist())):
        if rgb in seen:
            raise PsegError("label_masks: colour %d repeats colour %d %r" % (k, seen[rgb], rgb))
        seen[rgb] = k
    return col, idv


def _mask_sources(masks):
    arrs = []
    for k, m in enumerate(masks):
        a = np.asarray(m)
        if a.dtype != np.uint8:
            raise PsegError("mask %d: a uint8 array is expected, got dtype %s" % (k, a.dtype))
        if a.ndim == 3 and a.shape[2] == 4:
            raise PsegError("mask %d: an (H,W,4) array has an alpha channel; pass RGB, (H,W,3), or label ids, (H,W)" % k)
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise PsegError("mask %d: an (H,W,3) RGB or (H,W) id array is expected, got shape %r" % (k, a.shape))
        arrs.append(np.ascontiguousarray(a))
    table = (MASK_SRC * max(len(arrs), 1))()
    for k, a in enumerate(arrs):
        table[k] = MASK_SRC(a.ctypes.data, a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1)
    return table, arrs


def label_mask_groups(masks):
    """The group pseg_label_masks puts each mask of the list into (pseg_label_masks_groups; no device)."""
    table, arrs = _mask_sources(masks)
    n = len(arrs)
    out = (ctypes.c_int * max(n, 1))()
    _check(lib().pseg_label_masks_groups(n, table, out))
    return [int(g) for g in out[:n]]


def label_masks(masks, out_shapes, colors, ids, device=0, counts=False, host=False):
    """The label maps of a list of ground-truth masks at the shapes of their pages in one device-resident call (pseg_label_masks):
    masks[i] is a uint8 (H0,W0,3) RGB array, looked up in the table (colors (n,3), ids (n,), at most 256; an unknown colour gives
    0), or a uint8 (H0,W0) array of label ids; out_shapes[i] = (H,W).  Equals
    preserving_resize(color_map.to_labels(rgb), (H,W)).astype(uint8).  -> [labels uint8 (H,W)], or with counts=True
    [(labels, counts int64[257])]: pixels per id, and under [256] the pixels of unknown colour (also counted under id 0).
    host=True: the same bytes from the host entry (pseg_label_masks_host), no device."""
    table, arrs = _mask_sources(masks)
    n = len(arrs)
    if len(out_shapes) != n:
        raise PsegError("label_masks: out_shapes must have one entry per mask (%d for %d masks)" % (len(out_shapes), n))
    col, idv = color_table(colors, ids)
    if n == 0:
        return []
    shapes = [(int(s[0]), int(s[1])) for s in out_shapes]
    for k, s in enumerate(shapes):
        if s[0] <= 0 or s[1] <= 0:
            raise PsegError("mask %d: empty output shape %r" % (k, s))
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    labs = [np.empty(s, np.uint8) for s in shapes]
    cnt = np.zeros((n, 257), np.int64) if counts else None
    args = (n, table, I(*[s[0] for s in shapes]), I(*[s[1] for s in shapes]), _ptr(col) if len(col) else None, _ptr(idv) if len(col) else None,
            len(col), P(*[a.ctypes.data for a in labs]), _ptr(cnt))
    _check(lib().pseg_label_masks_host(*args) if host else lib().pseg_label_masks(int(device), *args))
    return [(a, cnt[k].copy()) for k, a in enumerate(labs)] if counts else labs


FILL_MODES = {"nearest": 0, "constant": 1, "reflect": 2, "wrap": 3}


def affine_warp(plane, matrix, offset, order, device=0, fill_mode="nearest", cval=0.0):
    """scipy.ndimage.affine_transform(plane, matrix, offset, order=order, mode=fill_mode, cval=cval) for a float32 (H,W)
    plane, order 0 or 3, fill_mode 'nearest', 'constant', 'reflect' or 'wrap' (the four keras-preprocessing accepts), on the GPU
    (the augmentation warp of lib/data_generator.py)."""
    if fill_mode not in FILL_MODES:
        raise PsegError("affine_warp: unknown fill_mode %r" % (fill_mode,))
    a = np.ascontiguousarray(plane, dtype=np.float32)
    if a.ndim != 2:
        raise PsegError("affine_warp takes one (H,W) plane")
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(4)
    o = np.ascontiguousarray(offset, dtype=np.float64).reshape(2)
    out = np.empty_like(a)
    _check(lib().pseg_affine_warp_fill(int(device), _ptr(a), a.shape[0], a.shape[1], _ptr(m), _ptr(o), int(order),
                                       FILL_MODES[fill_mode], float(cval), _ptr(out)))
    return out


def batch_units(shapes, cap=8):
    """The units pseg_predict_batch would cut a list of page shapes into: [(first page, page count), ...] (host logic, no GPU)."""
    n = len(shapes)
    H = (ctypes.c_int * max(n, 1))(*[int(s[0]) for s in shapes])
    W = (ctypes.c_int * max(n, 1))(*[int(s[1]) for s in shapes])
    first, count = (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))()
    nu = lib().pseg_batch_units(n, H, W, int(cap), first, count, n)
    _check(min(nu, 0))
    return [(first[u], count[u]) for u in range(nu)]


class _ArenaRow(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("producer_name", ctypes.c_char * 32), ("last_reader_name", ctypes.c_char * 32),
                ("bytes", ctypes.c_int64), ("offset", ctypes.c_int64),
                ("producer", ctypes.c_int), ("last_reader", ctypes.c_int), ("shared", ctypes.c_int), ("reserved", ctypes.c_int)]


def plan_arena(arch, H, W, n_classes=3, in_channels=1, plan=None):
    """The compact address map of a bf16 engine for an H x W page (pseg_plan_arena; host logic, no GPU): (rows, arena_bytes, full_bytes),
    rows = [dict(name, bytes, offset, producer, last_reader, producer_name, last_reader_name, shared)] in placement order.  plan: the
    engine's plan switches, a string or a dict as for Engine."""
    arch_id = ARCH_IDS[arch] if isinstance(arch, str) else int(arch)
    if isinstance(plan, dict):
        plan = ";".join("%s=%s" % kv for kv in sorted(plan.items()))
    L = lib()
    L.pseg_plan_arena.argtypes = [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_ArenaRow), ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    args = (arch_id, int(n_classes), int(in_channels), (plan or "").encode(), int(H), int(W))
    n = L.pseg_plan_arena(*args, None, 0, None, None)
    _check(min(n, 0))
    rows = (_ArenaRow * max(n, 1))()
    arena, full = ctypes.c_int64(), ctypes.c_int64()
    _check(min(L.pseg_plan_arena(*args, rows, n, ctypes.byref(arena), ctypes.byref(full)), 0))
    return ([dict(name=r.name.decode(), bytes=r.bytes, offset=r.offset, producer=r.producer, last_reader=r.last_reader,
                  producer_name=r.producer_name.decode(), last_reader_name=r.last_reader_name.decode(), shared=bool(r.shared)) for r in rows[:n]],
            arena.value, full.value)


def chain_units(shapes, out_shapes=None, cap=8):
    """The units pseg_predict_chain_pages_png cuts a page list into: [(first page, page count), ...]; out_shapes[i]: the final shape
    of page i's label map or None (host logic, no GPU).  Without out_shapes: batch_units."""
    n = len(shapes)
    I = ctypes.c_int * max(n, 1)
    H, W = I(*[int(s[0]) for s in shapes]), I(*[int(s[1]) for s in shapes])
    Ho = Wo = None
    if out_shapes is not None:
        if len(out_shapes) != n:
            raise PsegError("out_shapes must have one entry per page")
        Ho = I(*[0 if o is None else int(o[0]) for o in out_shapes])
        Wo = I(*[0 if o is None else int(o[1]) for o in out_shapes])
    first, count = I(), I()
    nu = lib().pseg_chain_units(n, H, W, Ho, Wo, int(cap), first, count, n)
    _check(min(nu, 0))
    return [(first[u], count[u]) for u in range(nu)]


def chain_units_mixed(shapes, cap=8):
    """How pseg_predict_chain_pages_mixed_png cuts a list of page shapes: (order, units).  order: a permutation of the pages, canvases
    (shapes rounded up to multiples of 32) by first appearance, list order within a canvas; units: [(first position in order, page
    count), ...], chain_units' cut of the permuted canvas list (host logic, no GPU)."""
    n = len(shapes)
    I = ctypes.c_int * max(n, 1)
    H, W = I(*[int(s[0]) for s in shapes]), I(*[int(s[1]) for s in shapes])
    order, first, count = I(), I(), I()
    nu = lib().pseg_chain_units_mixed(n, H, W, int(cap), order, first, count, n)
    _check(min(nu, 0))
    return [order[k] for k in range(n)], [(first[u], count[u]) for u in range(nu)]


def tile_plan(arch, shape, tile=0):
    """The tiles pseg_predict_tiled_device cuts an (H, W) page into (pseg_tile_plan; host arithmetic, no GPU):
    ((tile_h, tile_w), [(y, x), ...] origins on the page's canvas, [(y0, y1, x0, x1), ...] the owned rectangles, half-open).
    arch: a graph name or id; tile: the tile edge, 0 = the default."""
    arch_id = ARCH_IDS[arch] if isinstance(arch, str) else int(arch)
    H, W = int(shape[0]), int(shape[1])
    th, tw = ctypes.c_int(), ctypes.c_int()
    n = lib().pseg_tile_plan(arch_id, H, W, int(tile), ctypes.byref(th), ctypes.byref(tw), None, None, None, 0)
    _check(min(n, 0))
    oy, ox, own = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 4), np.int32)
    _check(min(lib().pseg_tile_plan(arch_id, H, W, int(tile), ctypes.byref(th), ctypes.byref(tw), _ptr(oy), _ptr(ox), _ptr(own), n), 0))
    return (th.value, tw.value), [(int(a), int(b)) for a, b in zip(oy, ox)], [tuple(int(v) for v in r) for r in own]


def brightness_shift(x, brightness, device=0):
    """keras-preprocessing 1.1.2 apply_brightness_shift(x, brightness, scale=False) on a float array (H,W[,C]) -> float32,
    on the GPU (pseg_brightness_shift; lib/trainer.py:21 brightness_range)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(a)
    _check(lib().pseg_brightness_shift(int(device), _ptr(a), a.size, float(brightness), _ptr(out)))
    return out


def _labels_arg(a):
    """A label map as a contiguous array of 1-, 4- or 8-byte integers (no copy for uint8 / int32 / int64)."""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype not in (np.uint8, np.int32, np.int64):
        a = a.astype(np.int64)
    return np.ascontiguousarray(a)


def eval_confusion(pred, mask, binary, n_classes, device=0):
    """counts[b][m][p] (2, n_classes+1, n_classes+1) int64: the joint histogram of (binary != 0, mask label,
    predicted label) behind fgpa / fgoverlap_per_class / count_matches / total_accuracy."""
    p, m = _labels_arg(pred), _labels_arg(mask)
    if p.shape != m.shape:
        raise PsegError("pred %r and mask %r differ in shape" % (p.shape, m.shape))
    b = None
    if binary is not None:
        b = np.ascontiguousarray(np.asarray(binary) != 0).view(np.uint8)
        if b.shape != p.shape:
            raise PsegError("binary %r and pred %r differ in shape" % (b.shape, p.shape))
    k = int(n_classes) + 1
    out = np.zeros((2, k, k), np.int64)
    _check(lib().pseg_eval_confusion(int(device), _ptr(p), p.dtype.itemsize, _ptr(m), m.dtype.itemsize,
                                     _ptr(b) if b is not None else None, ctypes.c_int64(p.size), int(n_classes), _ptr(out)))
    return out


def cc_label(binary, connectivity=4, device=0):
    """(num_labels, labels int32) as cv2.connectedComponents(binary, connectivity=...)."""
    b = np.ascontiguousarray(binary, dtype=np.uint8)
    if b.ndim != 2:
        raise PsegError("binary must be 2-dimensional")
    labels = np.zeros(b.shape, np.int32)
    n = ctypes.c_int32()
    _check(lib().pseg_cc_label(int(device), _ptr(b), b.shape[0], b.shape[1], int(connectivity), _ptr(labels), ctypes.byref(n)))
    return int(n.value), labels


def cc_tables(labels, num_labels, pred=None, mask=None, n_classes=0, want_stats=True, want_order=False, device=0):
    """dict with stats (N,5) int32 / centroids (N,2) float64 (cv2's), and with pred+mask: eq (N,), hist_pred,
    hist_mask (N, n_classes+1) int64; order (H*W,) int32 when asked."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    n = int(num_labels)
    out = {}
    stats = cent = eq = hp = hm = order = None
    if want_stats:
        stats, cent = np.zeros((n, 5), np.int32), np.zeros((n, 2), np.float64)
        out.update(stats=stats, centroids=cent)
    p = m = None
    if pred is not None and mask is not None:
        p, m = _labels_arg(pred), _labels_arg(mask)
        if p.shape != lab.shape or m.shape != lab.shape:
            raise PsegError("labels, pred and mask differ in shape")
        k = int(n_classes) + 1
        eq, hp, hm = np.zeros(n, np.int64), np.zeros((n, k), np.int64), np.zeros((n, k), np.int64)
        out.update(eq=eq, hist_pred=hp, hist_mask=hm)
    if want_order:
        order = np.zeros(lab.size, np.int32)
        out["order"] = order
    opt = lambda a: _ptr(a) if a is not None else None
    _check(lib().pseg_cc_tables(int(device), _ptr(lab), lab.shape[0], lab.shape[1], n, opt(p), p.dtype.itemsize if p is not None else 0,
                                opt(m), m.dtype.itemsize if m is not None else 0, int(n_classes), opt(stats), opt(cent), opt(eq),
                                opt(hp), opt(hm), opt(order)))
    return out


EVAL_MAX_RULES = 8


def eval_rule(kind, label=0, threshold_tp=0.0, threshold_fp=0.0, threshold_mask=0.0, filter_label=0, filter_threshold=0.0):
    """One rule of eval_pages as a plain tuple: kind 0 cc_matching(label, threshold_tp, threshold_fp, threshold_mask), kind 1
    cc_equal(threshold_tp); filter_label / filter_threshold are only_label()'s arguments (a falsy label: no filter)."""
    return (int(kind), int(label), float(threshold_tp), float(threshold_fp), float(threshold_mask), int(filter_label or 0),
            float(filter_threshold or 0.0))


def eval_page_groups(shapes):
    """The groups pseg_eval_pages would cut a list of page shapes into: [(first page, page count), ...] (host logic, no GPU)."""
    n = len(shapes)
    H = (ctypes.c_int * max(n, 1))(*[int(s[0]) for s in shapes])
    W = (ctypes.c_int * max(n, 1))(*[int(s[1]) for s in shapes])
    first, count = (ctypes.c_int * max(n, 1))(), (ctypes.c_int * max(n, 1))()
    ng = lib().pseg_eval_page_groups(n, H, W, first, count, n)
    _check(min(ng, 0))
    return [(first[g], count[g]) for g in range(ng)]


def _eval_map(a, what, k):
    """A label map of eval_pages as a contiguous uint8 (H,W) array; labels outside 0..254 raise, naming the page."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise PsegError("page %d: %s must be an (H,W) label map, got shape %r" % (k, what, a.shape))
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype.kind not in "iu":
        raise PsegError("page %d: %s must hold integer labels, got %s" % (k, what, a.dtype))
    if a.dtype != np.uint8:
        if a.size and (a.min() < 0 or a.max() > 254):
            raise PsegError("page %d: %s has labels outside 0..254" % (k, what))
        a = a.astype(np.uint8)
    elif a.size and a.max() > 254:
        raise PsegError("page %d: %s has labels outside 0..254" % (k, what))
    return np.ascontiguousarray(a)


def eval_pages(preds, masks, binaries=None, n_classes=None, connectivity=4, rules=(), device=0):
    """A list of pages scored against ground truth in one device-resident call (pseg_eval_pages): {"counts": (n, 2, K, K) int64, the
    joint histogram eval_confusion gives per page (K = n_classes + 1; binaries[i] None: every pixel counts as ink), "components":
    (n,) int64, the ink components per page, "verdicts": (n, len(rules), 4) int64, per rule (eval_rule tuples) the summed
    cc_matching vector or the cc_equal (true, false) counts over the components the rule keeps, and their number}.
    n_classes None: the top label over maps and rules, plus 1."""
    preds, masks = list(preds), list(masks)
    n = len(preds)
    if len(masks) != n or (binaries is not None and len(binaries) != n):
        raise PsegError("preds, masks and binaries must have one entry per page")
    rules = [eval_rule(*r) for r in rules]
    if len(rules) > EVAL_MAX_RULES:
        raise PsegError("%d rules (at most %d in one call)" % (len(rules), EVAL_MAX_RULES))
    if connectivity not in (4, 8):
        raise PsegError("connectivity %r (4 or 8)" % (connectivity,))
    ps, ms, bs = [], [], []
    for k in range(n):
        p, m = _eval_map(preds[k], "pred", k), _eval_map(masks[k], "mask", k)
        if p.shape != m.shape:
            raise PsegError("page %d: pred %r and mask %r differ in shape" % (k, p.shape, m.shape))
        b = None
        if binaries is not None and binaries[k] is not None:
            b = np.ascontiguousarray(np.asarray(binaries[k]) != 0).view(np.uint8)
            if b.shape != p.shape:
                raise PsegError("page %d: binary %r and pred %r differ in shape" % (k, b.shape, p.shape))
        ps.append(p); ms.append(m); bs.append(b)
    if n_classes is None:
        top = max([int(a.max(initial=0)) for a in ps + ms] + [max(r[1], r[5]) for r in rules] + [0])
        n_classes = top + 1
    n_classes = int(n_classes)
    if not 1 <= n_classes <= 255:
        raise PsegError("n_classes %d outside 1..255" % n_classes)
    for k, r in enumerate(rules):
        if r[0] not in (0, 1):
            raise PsegError("rule %d: kind %d (0: cc_matching, 1: cc_equal)" % (k, r[0]))
        if not (0 <= r[1] < n_classes and 0 <= r[5] < n_classes):
            raise PsegError("rule %d: label %d / filter label %d outside [0, %d)" % (k, r[1], r[5], n_classes))
    K, nr = n_classes + 1, len(rules)
    out = {"counts": np.zeros((n, 2, K, K), np.int64), "components": np.zeros(n, np.int64), "verdicts": np.zeros((n, nr, 4), np.int64)}
    pages = (EVAL_PAGE * max(n, 1))()
    for k in range(n):
        pages[k] = EVAL_PAGE(ps[k].ctypes.data, ms[k].ctypes.data, bs[k].ctypes.data if bs[k] is not None else None,
                             ps[k].shape[0], ps[k].shape[1])
    crules = (EVAL_RULE * max(nr, 1))(*[EVAL_RULE(*r) for r in rules])
    _check(lib().pseg_eval_pages(int(device), n, pages, n_classes, int(connectivity), nr, crules, _ptr(out["counts"]),
                                 _ptr(out["components"]), _ptr(out["verdicts"]) if nr else None))
    return out
