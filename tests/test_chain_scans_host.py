"""The host side of the scan chain (pseg_predict_chain_scans_png / Predictor.write_masks_scans): routing, chunking, the decode pool, the
shapes and radii the binding computes, the declared argument types.  No GPU: the engine is a stub that records its calls."""
import ctypes
import os
import threading

import numpy as np
import pytest

# the scales of tests/test_chain_scans_gpu.py: the front-end table (target / line height) and the chain's list
FRONT = [((97, 131), 1 / 2), ((200, 333), 37 / 100), ((130, 90), 1 / 5), ((300, 260), 2 / 25), ((64, 48), 1.0), ((37, 19), 8 / 5), ((61, 70), 1 / 10)]
CHAIN = list(zip([(150, 110), (180, 150), (260, 200), (240, 130), (200, 160), (220, 170)], [0.9, 0.5, 0.5, 0.4, 0.7, 0.4]))


def test_shapes_and_radii_equal_the_oracle():
    from oracle import resize as oresize
    from pseg_amd import engine as E
    for shape, scale in FRONT + CHAIN:
        H, W, ky, kx = E.scan_plan(shape, scale)
        assert (H, W) == oresize.rescale_shape(shape, scale), (shape, scale)
        for k, sigma in zip((ky, kx), oresize.aa_sigmas(shape, (H, W))):
            if sigma <= 1e-15:
                assert k == (None, 0), (shape, scale)
                continue
            w, r = oresize.gaussian_kernel(float(sigma))
            assert k[1] == r == int(4.0 * float(sigma) + 0.5) and np.array_equal(k[0], w), (shape, scale)
    # the table the binding hands to the library: shapes, radii, flag, and pointers into arrays it returns for keeping
    scans = [np.zeros(s, np.uint8) for s, _ in CHAIN]
    table, keep, plans = E.scan_table(scans, [sc for _, sc in CHAIN], high_res=True)
    for k, (shape, scale) in enumerate(CHAIN):
        t = table[k]
        assert (t.H0, t.W0, t.H, t.W, t.ry, t.rx, t.final_is_scan) == shape + plans[k][:2] + (plans[k][2][1], plans[k][3][1], 1)
        assert t.gray == keep[k].ctypes.data and t.wy == plans[k][2][0].ctypes.data and t.wx == plans[k][3][0].ctypes.data
    assert E.scan_table(scans[:1], [1.0])[0][0].wy is None and E.scan_table(scans[:1], [1.0])[0][0].final_is_scan == 0
    with pytest.raises(E.PsegError):
        E.scan_table(scans, [0.5])
    with pytest.raises(E.PsegError):
        E.scan_table([np.zeros((4, 4, 3), np.uint8)], [0.5])
    with pytest.raises(E.PsegError):
        E.scan_plan((3, 3), 0.1)


def test_new_symbols_and_their_argument_types():
    import pseg_amd
    from pseg_amd import engine as E
    L = pseg_amd.lib()
    c = ctypes
    assert "pseg_predict_chain_scans_png" in E.EXPORTED_SYMBOLS and "pseg_prepare_scans" in E.EXPORTED_SYMBOLS
    assert [(n, t) for n, t in E.SCAN._fields_] == [("gray", c.c_void_p), ("H0", c.c_int), ("W0", c.c_int), ("H", c.c_int), ("W", c.c_int),
                                                    ("wy", c.c_void_p), ("ry", c.c_int), ("wx", c.c_void_p), ("rx", c.c_int), ("final_is_scan", c.c_int)]
    assert c.sizeof(E.SCAN) == 56 and E.SCAN.wy.offset == 24 and E.SCAN.wx.offset == 40 and E.SCAN.final_is_scan.offset == 52
    assert L.pseg_prepare_scans.argtypes == [c.c_int, c.c_int, c.POINTER(E.SCAN), c.c_void_p, c.c_void_p, c.c_void_p]
    assert L.pseg_predict_chain_scans_png.argtypes == [c.c_void_p, c.c_int, c.POINTER(E.SCAN), c.POINTER(c.c_int), c.c_int, c.c_uint, c.c_void_p,
                                                       c.c_int, c.c_int, c.c_uint, c.c_int, E.CHAIN_SINK, c.c_void_p]
    # what needs no device: the argument checks of pseg_prepare_scans come first
    assert L.pseg_prepare_scans(0, -1, None, None, None, None) == -1
    assert L.pseg_prepare_scans(0, 0, None, None, None, None) == 0
    table, keep, plans = E.scan_table([np.zeros((20, 30), np.uint8)], [0.5])
    out = np.zeros(plans[0][:2], np.uint8)
    P = c.c_void_p * 1
    table[0].rx += 1
    assert L.pseg_prepare_scans(0, 1, table, P(out.ctypes.data), P(out.ctypes.data), None) == -1 and b"radius" in L.pseg_last_error()
    assert L.pseg_predict_chain_scans_png(None, 1, table, None, 0, 0, None, 0, 0, 7, 0, E.CHAIN_SINK(lambda *a: 0), None) == -1 and b"radius" in L.pseg_last_error()
    table[0].rx -= 1
    assert L.pseg_predict_chain_scans_png(None, 1, table, None, 0, 0, None, 0, 0, 7, 0, ctypes.cast(None, E.CHAIN_SINK), None) == -1 and b"sink" in L.pseg_last_error()


# ---- Predictor.write_masks_scans over a stub -------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self, log):
        self.log = log

    def predict_chain_scans(self, scans, scales, high_res=False, post_ops=(), exact_labels=False, lut=None, which=(), labels=False, png_level=0,
                            unit_cap=0, sink=None):
        self.log.append(("device", [int(s[0, 0]) for s in scans], list(scales), high_res, list(post_ops), png_level))
        for page in range(len(scans)):
            for name in which:
                sink(page, name, ("%s %d" % (name, int(scans[page][0, 0]))).encode())


class _StubNetwork:
    n_classes = 3
    _rgb = False
    exact = False

    def __init__(self, log):
        self.model = _StubEngine(log)


class _StubLoader:
    target_line_height = 6
    max_width = None

    def __init__(self, log):
        self.log = log

    def load_images(self, entry):
        self.log.append(("load", os.path.basename(entry.image_path)))
        entry.binary = "loaded"
        return entry


def _predictor(log, monkeypatch, post_process=()):
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    from ocr4all_pixel_classifier.lib import dataset
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    pred = Predictor(PredictSettings(n_classes=3, color_map=cm, post_process=list(post_process), high_res_output=True), _StubNetwork(log))
    monkeypatch.setattr(pred, "write_masks", lambda data, output_dir=None, level=None: log.append(("write_masks", os.path.basename(data.image_path), data.binary)))

    def imread(path):
        # "scan7.png" decodes to a (40, 30) plane of sevens
        k = int(os.path.basename(path)[4:-4])
        log.append(("decode", k, threading.current_thread() is threading.main_thread()))
        if k == 13:
            raise IOError("scan13.png is broken")
        return np.full((40, 30), k, np.uint8)
    monkeypatch.setattr(dataset, "_imread_gray", imread)
    return pred


def _entries(n):
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    return [SingleData(image_path="/in/scan%d.png" % k, line_height_px=12 + k) for k in range(n)]


def test_routing_chunking_and_path_order(tmp_path, monkeypatch):
    import dataclasses
    from ocr4all_pixel_classifier.lib import output, postprocess
    log = []
    pred = _predictor(log, monkeypatch, [postprocess.vote_connected_component_class])
    entries = _entries(7)
    entries[2] = dataclasses.replace(entries[2], image=np.zeros((40, 30), np.uint8))       # pre-loaded
    entries[4] = dataclasses.replace(entries[4], output_path="four.jpg")                   # not a PNG target
    got = list(pred.write_masks_scans(entries, _StubLoader(log), str(tmp_path), level=1, chunk_pages=3))
    assert got == [output.output_paths(str(tmp_path), e) for e in entries]                 # every entry's paths, in order
    device = [e for e in log if e[0] == "device"]
    # chunks of three entries; only the device candidates of a chunk reach the engine, with their own scales
    assert [d[1] for d in device] == [[0, 1], [3, 5], [6]]
    assert [d[2] for d in device] == [[6 / 12, 6 / 13], [6 / 15, 6 / 17], [6 / 18]]
    assert all(d[3] is True and d[4] == ["cc_vote"] and d[5] == 1 for d in device)
    assert [e for e in log if e[0] in ("load", "write_masks")] == [("load", "scan2.png"), ("write_masks", "scan2.png", "loaded"),
                                                                   ("load", "scan4.png"), ("write_masks", "scan4.png", "loaded")]
    assert sorted(e[1] for e in log if e[0] == "decode") == [0, 1, 3, 5, 6] and not any(e[2] for e in log if e[0] == "decode")
    for k in (0, 1, 3, 5, 6):
        assert [open(p, "rb").read() for p in got[k]] == [b"%s %d" % (nm, k) for nm in (b"color", b"overlay", b"inverted")]
    assert entries[0].binary is None and entries[2].binary == "loaded"                     # the device path leaves its entries alone
    assert list(pred.write_masks_scans([], _StubLoader(log), str(tmp_path))) == []


def test_everything_falls_back_where_the_device_path_is_off(tmp_path, monkeypatch):
    from ocr4all_pixel_classifier.lib import output
    log = []
    # a foreign post-processor
    pred = _predictor(log, monkeypatch, [lambda pred, data: pred])
    assert len(list(pred.write_masks_scans(_entries(3), _StubLoader(log), str(tmp_path)))) == 3
    # an rgb network, more than 256 classes, DEVICE_PNG off
    for attr, value in (("_rgb", True), ("n_classes", 300)):
        pred = _predictor(log, monkeypatch)
        setattr(pred.network, attr, value)
        assert len(list(pred.write_masks_scans(_entries(3), _StubLoader(log), str(tmp_path)))) == 3
    pred = _predictor(log, monkeypatch)
    monkeypatch.setattr(output, "DEVICE_PNG", False)
    assert len(list(pred.write_masks_scans(_entries(3), _StubLoader(log), str(tmp_path)))) == 3
    monkeypatch.setattr(output, "DEVICE_PNG", True)
    assert [e[0] for e in log] == ["load", "write_masks"] * 12                             # nothing decoded here, nothing sent to the engine
    # a max_width that brings the second stage shows once the scan is decoded: (40, 30) scans, line heights 12 13 14 -> widths 15 14 13
    log.clear()
    loader = _StubLoader(log)
    loader.max_width = 14
    pred = _predictor(log, monkeypatch)
    assert len(list(pred.write_masks_scans(_entries(3), loader, str(tmp_path)))) == 3
    assert [e[1] for e in log if e[0] == "device"] == [[1, 2]] and [e for e in log if e[0] == "load"] == [("load", "scan0.png")]


def test_the_pool_decodes_the_next_chunk_during_the_device_call(tmp_path, monkeypatch):
    log = []
    pred = _predictor(log, monkeypatch)
    started = {}
    real = pred.network.model.predict_chain_scans

    def device(scans, scales, **kw):
        # what has been handed to the pool by the time the device call of a chunk starts: the next chunk's files too
        started[int(scans[0][0, 0])] = pred_pool_seen()
        return real(scans, scales, **kw)

    submitted = []
    from concurrent import futures
    real_submit = futures.ThreadPoolExecutor.submit

    def submit(self, fn, entry):
        submitted.append(os.path.basename(entry.image_path))
        return real_submit(self, fn, entry)
    monkeypatch.setattr(futures.ThreadPoolExecutor, "submit", submit)
    pred_pool_seen = lambda: list(submitted)
    monkeypatch.setattr(pred.network.model, "predict_chain_scans", device)
    assert len(list(pred.write_masks_scans(_entries(6), _StubLoader(log), str(tmp_path), chunk_pages=2, decode_threads=2))) == 6
    assert started == {0: ["scan%d.png" % k for k in range(4)], 2: ["scan%d.png" % k for k in range(6)], 4: ["scan%d.png" % k for k in range(6)]}


def test_a_decode_error_surfaces_at_its_entry(tmp_path, monkeypatch):
    from ocr4all_pixel_classifier.lib import output
    log = []
    pred = _predictor(log, monkeypatch)
    entries = _entries(16)
    it = pred.write_masks_scans(entries, _StubLoader(log), str(tmp_path), chunk_pages=4)
    got = []
    with pytest.raises(IOError, match="scan13.png is broken"):
        for paths in it:
            got.append(paths)
    # the twelve entries of the chunks in front and the one entry in front of it in its own chunk; nothing behind it
    assert got == [output.output_paths(str(tmp_path), e) for e in entries[:13]]
    assert [d[1] for d in log if d[0] == "device"] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12]]
