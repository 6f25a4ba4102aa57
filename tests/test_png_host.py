"""Host-side contract of the device PNG encoder: pseg_png_bound is arithmetic (no device), and without a device the encoder
entries fail loudly like the rest of the package (no CPU fallback)."""
import numpy as np
import pytest


def _bound(H, W, ch, band_rows=0):
    import pseg_amd
    return pseg_amd.png_bound(H, W, ch, band_rows)


def test_bound_covers_the_filtered_bytes_and_is_monotonic():
    for ch in (1, 3):
        for band_rows in (0, 1, 7):
            prev_h = 0
            for H in (1, 2, 3, 7, 8, 64, 65, 1000):
                b = _bound(H, 333, ch, band_rows)
                assert b >= H * (ch * 333 + 1) and b > prev_h
                prev_h = b
            prev_w = 0
            for W in list(range(1, 40)) + [1365, 1366, 5461, 5462, 5463, 16383, 16384, 40000]:      # around the default band's steps
                b = _bound(50, W, ch, band_rows)
                assert b >= 50 * (ch * W + 1) and b > prev_w, (ch, band_rows, W)
                prev_w = b


def test_bound_is_tight_for_the_default_band_and_does_not_wrap():
    for H, W, ch in ((64, 64, 3), (64, 64, 1), (2048, 1536, 3), (4096, 3072, 3)):
        raw = H * W * ch
        assert _bound(H, W, ch) <= 1.25 * raw + 4096                 # fixed Huffman: 9 bits per byte at worst, plus framing
    b = _bound(40000, 40000, 3)
    assert b > 2 ** 32 and b >= 40000 * (3 * 40000 + 1) and b < 1.25 * 40000 * 40000 * 3
    # the formula include/pseg.h states: 80 + sum over the bands of (12 + n + n / 8 + 8)
    L = 3 * 100 + 1
    assert _bound(10, 100, 3, 4) == 80 + 2 * (20 + 4 * L + 4 * L // 8) + (20 + 2 * L + 2 * L // 8)


def test_bound_rejects_bad_arguments():
    import pseg_amd
    L = pseg_amd.lib()
    for args in ((0, 5, 3, 0), (5, 0, 3, 0), (5, 5, 2, 0), (5, 5, 4, 0), (5, 5, 3, -1), (-1, 5, 1, 0)):
        assert L.pseg_png_bound(*args) == 0
        with pytest.raises(pseg_amd.PsegError):
            pseg_amd.png_bound(*args)


def test_no_cpu_fallback_without_a_device():
    """Without a device the entries raise; with one they encode (this file runs on both kinds of machine)."""
    import pseg_amd
    a, lab = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.int64)
    if pseg_amd.device_count() > 0:
        assert pseg_amd.png_encode(a)[:8] == b"\x89PNG\r\n\x1a\n"
        assert sorted(pseg_amd.masks_png(lab, np.ones((4, 4), np.uint8), np.zeros((3, 3), np.uint8))) == ["color", "inverted", "overlay"]
        return
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.png_encode(a)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.masks_png(lab, np.ones((4, 4), np.uint8), np.zeros((3, 3), np.uint8))


def test_python_surface():
    import pseg_amd
    from ocr4all_pixel_classifier.lib import output, predictor
    assert callable(pseg_amd.png_encode) and callable(pseg_amd.masks_png) and callable(pseg_amd.png_bound)
    assert output.DEVICE_PNG is True and callable(predictor.Predictor.write_masks)
    assert output.is_png_target("a/PAGE.PNG") and output.is_png_target("x.png") and not output.is_png_target("page.jpg")
    for sym in ("pseg_png_bound", "pseg_png_encode_device", "pseg_masks_png_device_u8", "pseg_png_encode", "pseg_masks_png", "pseg_predict_chain_png"):
        assert sym in pseg_amd.EXPORTED_SYMBOLS and hasattr(pseg_amd.lib(), sym)
