"""The PNG reader on the device: pseg_png_decode_gray / pseg_png_decode_gray_device (pngdec_inflate_kernel, pngdec_unfilter_kernel)
against PIL and against the host entry on the files of tests/pngdec_cases.py, and the decode="device" routes of
compute_char_heights and Predictor.write_masks_scans against decode="host".  The corrupt corpus is the one the host test and the
stand-alone sanitizer check (tools/pngdec_check.cpp) pass on the host: the device is expected to return the same codes."""
import ctypes
import os

import numpy as np
import pytest

import pngdec_cases as C

pytestmark = pytest.mark.gpu


def _valid():
    return C.matrix() + C.splits() + C.hand_streams()


def test_valid_files_equal_pil_and_the_host_entry_twice(gpu):
    cases = _valid()
    files = [d for _, d, _ in cases]
    host = gpu.png_decode_gray(files, host=True)
    for turn in range(2):
        got = gpu.png_decode_gray(files)
        assert len(got) == len(cases)
        for (name, _, want), (arr, st), (harr, hst) in zip(cases, got, host):
            assert st == C.OK and hst == C.OK, (turn, name, st)
            assert arr.shape == want.shape and np.array_equal(arr, want), (turn, name)
            assert np.array_equal(arr, harr), (turn, name)


def test_seventy_files_in_two_groups_permuted(gpu):
    cases = _valid()
    order = np.random.RandomState(1).permutation(70) % len(cases)
    got = gpu.png_decode_gray([cases[k][1] for k in order])
    for k, (arr, st) in zip(order, got):
        assert st == C.OK and np.array_equal(arr, cases[k][2]), cases[k][0]


def test_refusals_and_corrupt_files_among_good_ones(gpu):
    good = C.matrix()[3]
    bad = [(n, d, C.EUNSUPPORTED) for n, d in C.refusals()] + [(n, d, C.EINVAL) for n, d, *_ in C.corrupt()]
    files = [good[1]]
    for _, d, _ in bad:
        files += [d, good[1]]
    host = gpu.png_decode_gray(files, host=True)
    got = gpu.png_decode_gray(files)
    assert [st for _, st in got] == [st for _, st in host]
    for k, (arr, st) in enumerate(got):
        if k % 2 == 0:
            assert st == C.OK and np.array_equal(arr, good[2]), k
        else:
            assert st == bad[k // 2][2] and arr is None, bad[k // 2][0]


def _c_lists(files):
    n = len(files)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p).value for f in files])
    lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
    return n, ptrs, lens


def test_a_refused_files_output_is_untouched(gpu):
    bad = [d for _, d in C.refusals()[:2]] + [d for n, d, *_ in C.corrupt() if n in ("bitflip", "adler", "row-long", "row-short", "filter5", "too-far")]
    good = C.matrix()[3]
    files = bad + [good[1]]
    n, ptrs, lens = _c_lists(files)
    outs = [gpu.pinned_empty((70 * 50 * 2,), np.uint8) for _ in files]
    for o in outs:
        o[...] = 0xA5
    status = (ctypes.c_int * n)(*([7] * n))
    rc = gpu.lib().pseg_png_decode_gray(0, n, ptrs, lens, (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs]), status)
    assert rc == 0
    assert list(status)[:-1] == [C.EUNSUPPORTED] * 2 + [C.EINVAL] * (len(bad) - 2) and status[n - 1] == C.OK
    for o in outs[:-1]:
        assert (o == 0xA5).all()
    H, W = good[2].shape
    assert np.array_equal(outs[-1][:H * W].reshape(H, W), good[2]) and (outs[-1][H * W:] == 0xA5).all()


def test_device_output_entry(gpu):
    import torch
    cases = [C.matrix()[8], C.matrix()[17], C.hand_streams()[0], C.splits()[1]]
    bad = C.corrupt()[6][1]
    files = [c[1] for c in cases] + [bad]
    n, ptrs, lens = _c_lists(files)
    bufs = [torch.full((c[2].size + 64,), 0xA5, dtype=torch.uint8, device="cuda") for c in cases] + [torch.full((70 * 50,), 0xA5, dtype=torch.uint8, device="cuda")]
    torch.cuda.synchronize()
    status = (ctypes.c_int * n)(*([7] * n))
    stream = torch.cuda.current_stream().cuda_stream
    rc = gpu.lib().pseg_png_decode_gray_device(0, n, ptrs, lens, (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs]), status, ctypes.c_void_p(stream))
    assert rc == 0, gpu.lib().pseg_last_error()
    assert list(status) == [C.OK] * len(cases) + [C.EINVAL]
    for c, b in zip(cases, bufs):
        h = b.cpu().numpy()
        assert np.array_equal(h[:c[2].size].reshape(c[2].shape), c[2]) and (h[c[2].size:] == 0xA5).all(), c[0]
    assert (bufs[-1].cpu().numpy() == 0xA5).all()
    assert gpu.lib().pseg_release_workspace(0) == 0                      # and the decoder works again after the release
    (arr, st), = gpu.png_decode_gray([cases[0][1]])
    assert st == C.OK and np.array_equal(arr, cases[0][2])


def _text_scan(k, H, W):
    from pseg_amd import synth
    return (255 - synth.synth_page(k, H, W, 3)[0]).astype(np.uint8)


SCAN_SHAPES = ((260, 200), (240, 230), (300, 260), (280, 210), (250, 250))   # with seeds 60 .. 64: text whose line height measures


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_compute_char_heights_device_equals_host(gpu, tmp_path):
    from PIL import Image
    from ocr4all_pixel_classifier.lib import image_ops
    paths = []
    for k, (H, W) in enumerate(SCAN_SHAPES[:3]):
        scan = _text_scan(60 + k, H, W)
        paths.append(_write(str(tmp_path / ("s%d.png" % k)), C.make_png(scan, [y % 5 for y in range(H)], 6)))
    rgb = np.repeat(_text_scan(63, *SCAN_SHAPES[3])[..., None], 3, axis=2)
    paths.append(_write(str(tmp_path / "rgb.png"), C.make_png(rgb, 4, 1)))
    Image.fromarray(_text_scan(64, *SCAN_SHAPES[4]).astype(np.uint16) * 257).save(str(tmp_path / "deep.png"))   # 16 bit: the PIL fallback
    paths.append(str(tmp_path / "deep.png"))
    for inverse in (False, True):
        want = image_ops.compute_char_heights(paths, inverse)
        assert image_ops.compute_char_heights(paths, inverse, decode="device") == want
        assert image_ops.compute_char_heights(paths, inverse, decode="device", chunk_files=2, decode_threads=1) == want
        assert inverse or all(isinstance(h, int) for h in want[:4])
    _write(str(tmp_path / "broken.png"), C.corrupt()[6][1])
    errs = []
    for decode in ("host", "device"):
        with pytest.raises(Exception) as ei:
            image_ops.compute_char_heights(paths + [str(tmp_path / "broken.png")], False, decode=decode)
        errs.append((type(ei.value), str(ei.value)))
    assert errs[0] == errs[1]                                            # PIL's exception on both routes


def test_write_masks_scans_device_decode_writes_the_same_files(gpu, tmp_path):
    from PIL import Image
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    from ocr4all_pixel_classifier.lib.dataset import DatasetLoader, SingleData
    net = Network("Predict", n_classes=3, exact=False)
    net.model.set_weights(synth.glorot_weights(net.model.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    pred = Predictor(PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor("cc_majority")], high_res_output=False), net)
    loader = DatasetLoader(6, cm, prediction=True)
    os.makedirs(str(tmp_path / "scans"))
    scans = [_text_scan(60 + k, H, W) for k, (H, W) in enumerate(SCAN_SHAPES)]

    def entries():
        out = []
        for k, kind in enumerate(("gray", "gray", "rgb", "deep", "unmeasured", "corrupt")):
            path = str(tmp_path / "scans" / ("%d-%s.png" % (k, kind)))
            if not os.path.exists(path):
                if kind == "rgb":
                    _write(path, C.make_png(np.repeat(scans[k][..., None], 3, axis=2), [y % 5 for y in range(scans[k].shape[0])], 1))
                elif kind == "deep":
                    Image.fromarray(scans[k].astype(np.uint16) * 257).save(path)
                elif kind == "corrupt":
                    _write(path, C.corrupt()[6][1])
                else:
                    _write(path, C.make_png(scans[k], 4 if k else 2, 6))
            out.append(SingleData(image_path=path, line_height_px=None if kind == "unmeasured" else 12))
        return out

    results = {}
    for decode, kw in (("host", {}), ("device", {}), ("device", {"chunk_pages": 2, "decode_threads": 1})):
        name = decode + ("-chunks" if kw else "")
        mine, paths, err = entries(), [], None
        try:
            for p in pred.write_masks_scans(mine, loader, str(tmp_path / name), level=1, decode=decode, **kw):
                paths.append(p)
        except Exception as exc:
            err = (type(exc), str(exc))
        files = [[open(f, "rb").read() for f in p] for p in paths]
        results[name] = ([[os.path.relpath(f, str(tmp_path / name)) for f in p] for p in paths], files, err, [e.line_height_px for e in mine])
    want = results["host"]
    assert len(want[0]) == 5 and want[2] is not None and want[3][4] is not None      # five entries, then PIL's exception at the sixth
    assert results["device"] == want
    assert results["device-chunks"] == want
