"""The device PNG encoder (csrc/pseg_png.hip) against two independent decoders: a strict one written here over zlib
(signature, chunk walk with every CRC, IHDR fields, one zlib stream that must end exactly -- which validates the Adler-32 and
the final block --, all five PNG filters undone in NumPy) and PIL.  PNG is lossless: a valid file that decodes to the source
pixels is correct.  The shapes are the smallest at which each mechanism of the encoder can break."""
import ctypes
import io
import os
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIG = b"\x89PNG\r\n\x1a\n"


def strict_decode(png, want_shape):
    """-> the image as uint8 (H,W) or (H,W,3); asserts everything a reader may rely on."""
    assert isinstance(png, bytes) and png[:8] == SIG
    pos, chunks = 8, []
    while pos < len(png):
        assert pos + 12 <= len(png)
        n, = struct.unpack(">I", png[pos:pos + 4])
        typ, body = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        assert len(body) == n and pos + 12 + n <= len(png)
        crc, = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(typ + body), "CRC of chunk %r at %d" % (typ, pos)
        chunks.append((typ, body))
        pos += 12 + n
    assert pos == len(png) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    ch = {2: 3, 0: 1}[ctype]
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    assert (H, W) == tuple(want_shape[:2]) and ch == (3 if len(want_shape) == 3 else 1)
    kinds = [t for t, _ in chunks[1:-1]]
    assert kinds and set(kinds) == {b"IDAT"}                       # consecutive IDATs, nothing else
    d = zlib.decompressobj()
    raw = d.decompress(b"".join(body for t, body in chunks if t == b"IDAT"))
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    L = ch * W + 1
    assert len(raw) == H * L
    rows = np.frombuffer(raw, np.uint8).reshape(H, L)
    out = np.zeros((H, ch * W), np.uint8)
    prev = np.zeros(ch * W, np.int32)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        assert f in (0, 1, 2, 3, 4)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:                                                      # Sub / Average / Paeth: left neighbour -> sequential per channel
            cur = np.zeros(ch * W, np.int32)
            for i in range(ch * W):
                a = cur[i - ch] if i >= ch else 0
                b = prev[i]
                c = prev[i - ch] if i >= ch else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (line[i] + p) & 255
        out[y] = cur
        prev = cur
    return out.reshape(want_shape)


def check(gpu, a, band_rows=0):
    """Encode, decode with both decoders, compare; -> the stream."""
    from PIL import Image
    png = gpu.png_encode(a, band_rows=band_rows)
    assert np.array_equal(strict_decode(png, a.shape), a), (a.shape, band_rows)
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == ("RGB" if a.ndim == 3 else "L") and np.array_equal(np.asarray(im), a), (a.shape, band_rows)
    ch = 3 if a.ndim == 3 else 1
    assert len(png) <= gpu.png_bound(a.shape[0], a.shape[1], ch, band_rows)
    return png


def patches(rng, H, W, ch):
    """Three random colours in random 4 x 5 patches: matches and literals both occur."""
    pal = rng.integers(0, 256, (3, ch)).astype(np.uint8)
    idx = rng.integers(0, 3, (H // 4 + 1, W // 5 + 1)).repeat(4, 0).repeat(5, 1)[:H, :W]
    return np.ascontiguousarray(pal[idx].reshape((H, W, 3) if ch == 3 else (H, W)))


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("H", [1, 2, 3, 17])
def test_tiny_and_ragged_shapes(gpu, H, ch):
    """Rows of 4 bytes (shorter than any match), 64 / 67 (a wave), 256 / 259 / 262 (the 258-byte match limit); H no multiple of the
    band; 1, 2 and many bands."""
    rng = np.random.default_rng(100 * H + ch)
    for W in (1, 2, 3, 21, 22, 85, 86, 87):
        a = patches(rng, H, W, ch)
        for band_rows in (1, 2, 3, 0):
            check(gpu, a, band_rows)


@pytest.mark.parametrize("rows", [1, 3])
def test_run_lengths(gpu, rows):
    """A run of n bytes, then another colour: the split into 258s with remainders 0, 1 and 2 (literals) and >= 3 (a shorter match).
    Gray: the run of equal filtered bytes is n - 1 (first row) long behind its first literal; RGB: 3 n - 3."""
    for run in (2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518):
        for n in (run, run + 1):                                   # the run itself / the run behind the literal that starts it
            g = np.full((rows, n + 3), 17, np.uint8)
            g[:, :n] = 200
            check(gpu, g, 1)
            check(gpu, g, 0)
        if run % 3 == 0:
            c = np.zeros((rows, run // 3 + 2, 3), np.uint8)
            c[:, :run // 3] = (10, 200, 90)
            c[:, run // 3:] = (7, 7, 250)
            check(gpu, c, 0)


def test_literal_classes(gpu):
    rng = np.random.default_rng(3)
    for ch in (3, 1):
        a = rng.integers(0, 256, (64, 64, 3) if ch == 3 else (64, 64)).astype(np.uint8)      # incompressible: 8- and 9-bit literals
        for band_rows in (0, 1, 5):
            png = check(gpu, a, band_rows)
            assert len(png) <= gpu.png_bound(64, 64, ch, band_rows)
        assert gpu.png_bound(64, 64, ch, 0) <= 1.25 * a.size + 4096                           # fixed Huffman: 9/8 plus framing
    for v in (255, 0, 143, 144):
        check(gpu, np.full((64, 64), v, np.uint8), 0)
        check(gpu, np.full((64, 64, 3), v, np.uint8), 7)
    alt = np.zeros((64, 64), np.uint8)                              # 143 / 144 alternate along both axes: the 8 / 9-bit border as literals
    alt[::2, ::2], alt[1::2, 1::2], alt[::2, 1::2], alt[1::2, ::2] = 143, 143, 144, 144
    check(gpu, alt, 0)


def test_adler32(gpu):
    """256x256x3 all-255: s2 overflows when the modulo is deferred too long, many bands to combine.  40x1536x3 with 16-row
    bands: a band has more than 65 521 bytes -- the length-mod-65521 term of the combine."""
    check(gpu, np.full((256, 256, 3), 255, np.uint8), 0)
    check(gpu, np.full((256, 256, 3), 255, np.uint8), 256)
    rng = np.random.default_rng(4)
    check(gpu, rng.integers(0, 256, (40, 1536, 3)).astype(np.uint8), 16)
    check(gpu, np.full((40, 1536, 3), 255, np.uint8), 16)
    col = np.zeros((40, 1536, 3), np.uint8)                         # Up leaves 255s in every row: 255 -> 0 -> 255 ...
    col[::2] = 255
    check(gpu, col, 16)


@pytest.mark.parametrize("W", [10922, 10923])
def test_window_limit(gpu, W):
    """Row strides 32 767 / 32 770 around deflate's 32 768-byte window: identical rows, no period inside a row."""
    rng = np.random.default_rng(5)
    row = rng.integers(0, 256, (1, W, 3)).astype(np.uint8)
    a = np.ascontiguousarray(np.repeat(row, 3, 0))
    check(gpu, a, 0)
    check(gpu, a, 3)


def _synth_masks(gpu, page, H, W, C):
    from pseg_amd import synth
    _, binary, mask = synth.synth_page(page, H, W, C)
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255]], np.uint8)[:C]
    return mask.astype(np.int64), binary, lut


def test_compression_really_happens(gpu):
    a = np.full((512, 512, 3), (12, 200, 77), np.uint8)
    assert len(check(gpu, a, 0)) < a.size / 32
    pred, binary, lut = _synth_masks(gpu, 0, 384, 512, 3)
    raw = 384 * 512 * 3
    for name, png in gpu.masks_png(pred, binary, lut).items():
        assert len(png) < raw / 8, (name, len(png), raw)


def test_fused_mask_source(gpu):
    """The band kernel computes the masks' pixels from labels / binarisation / colour table: equal to pseg_masks' arrays."""
    cases = [_synth_masks(gpu, 1, 160, 224, 6)]
    rng = np.random.default_rng(7)
    cases.append((rng.integers(0, 256, (37, 86)).astype(np.int64), rng.integers(0, 3, (37, 86)).astype(np.uint8),   # binary 2: numpy's wrap-around rule
                  rng.integers(0, 256, (256, 3)).astype(np.uint8)))
    names = ("color", "overlay", "inverted", "fg_color")
    for pred, binary, lut in cases:
        want = dict(zip(names, gpu.masks(pred, binary, lut)))
        got = gpu.masks_png(pred, binary, lut, which=names)
        assert sorted(got) == sorted(names)
        for n in names:
            assert np.array_equal(strict_decode(got[n], want[n].shape), want[n]), n
        from PIL import Image
        im = Image.open(io.BytesIO(got["overlay"]))
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), want["overlay"])
        sub = gpu.masks_png(pred, binary, lut, which=("inverted", "color"), band_rows=5)
        assert sorted(sub) == ["color", "inverted"]
        assert np.array_equal(strict_decode(sub["inverted"], want["inverted"].shape), want["inverted"])
        assert gpu.masks_png(pred, binary, lut) == {n: got[n] for n in names[:3]}             # deterministic bytes, default `which`


def _predictor(gpu, oracle_mod, shape, posts, high_res, tmp_path=None):
    import dataclasses
    from pseg_amd import synth
    from ocr4all_pixel_classifier.lib.network import Network
    from ocr4all_pixel_classifier.lib.dataset import SingleData
    from ocr4all_pixel_classifier.lib.predictor import Predictor
    from ocr4all_pixel_classifier.lib.predictor_data import PredictSettings
    from ocr4all_pixel_classifier.lib.postprocess import find_postprocessor
    from ocr4all_pixel_classifier.lib.colors import ColorMap
    img, binary, _ = synth.synth_page(4, shape[0], shape[1], 3)
    net = Network("Predict", n_classes=3, exact=True)
    net.model.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    data = SingleData(image=img, binary=binary, original_shape=img.shape, image_path="page.png")
    if high_res:
        orig = (shape[0] + 71, shape[1] + 41)
        data = dataclasses.replace(data, original_shape=orig, orig_binary=(np.random.default_rng(1).random(orig) < 0.2).astype(np.uint8))
    cm = ColorMap({"(255, 255, 255)": [0, "bg"], "(255, 0, 0)": [1, "text"], "(0, 255, 0)": [2, "image"]})
    settings = PredictSettings(n_classes=3, color_map=cm, post_process=[find_postprocessor(p) for p in posts], high_res_output=high_res,
                               output=str(tmp_path) if tmp_path is not None else None)
    return Predictor(settings, net), data, cm


@pytest.mark.parametrize("shape", [(96, 64), (160, 224)])
def test_chain_png_equals_chain_arrays(gpu, oracle_mod, shape):
    from pseg_amd import synth
    img, binary, _ = synth.synth_page(4, shape[0], shape[1], 3)
    eng = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_F32_EXACT)
    eng.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    out_shape = (shape[0] + 71, shape[1] + 41)
    big_bin = (np.random.default_rng(1).random(out_shape) < 0.2).astype(np.uint8)
    for posts, osh, b in ((["cc_vote"], None, binary), (["bbox"], None, binary), (["cc_vote", "bbox"], out_shape, big_bin), ([], out_shape, big_bin)):
        want = eng.predict_chain(img, binary=b, out_shape=osh, post_ops=posts, labels="u8", lut=lut, masks=True)
        got = eng.predict_chain(img, binary=b, out_shape=osh, post_ops=posts, labels="u8", lut=lut, masks="png")
        assert np.array_equal(got["labels"], want["labels"])
        assert len(got["masks"]) == 4 and all(isinstance(m, bytes) for m in got["masks"])
        for png, arr in zip(got["masks"], want["masks"]):
            assert np.array_equal(strict_decode(png, arr.shape), arr), (posts, osh)
    eng.close()


@pytest.mark.parametrize("posts,high_res", [(["cc_majority"], False), (["cc_majority", "bounding_boxes"], True)])
def test_write_masks_and_output_data(gpu, oracle_mod, tmp_path, posts, high_res):
    import dataclasses
    from PIL import Image
    from ocr4all_pixel_classifier.lib import output
    pred, data, cm = _predictor(gpu, oracle_mod, (96, 64), posts, high_res, tmp_path / "a")
    m = pred.predict_masks(data)
    want = (m.color, m.overlay, m.inverted_overlay)
    paths = pred.write_masks(data)
    assert [os.path.relpath(p, str(tmp_path / "a")) for p in paths] == ["color/page.png", "overlay/page.png", "inverted/page.png"]
    for p, arr in zip(paths, want):
        assert np.array_equal(strict_decode(open(p, "rb").read(), arr.shape), arr)
        assert np.array_equal(np.asarray(Image.open(p)), arr)
    # a foreign post-processor: the host chain, same files
    pred.settings.post_process = list(pred.settings.post_process) + [lambda lab, d: lab]
    assert pred._chain_ops() is None
    paths_b = pred.write_masks(data, str(tmp_path / "b"))
    for p, q in zip(paths, paths_b):
        assert open(p, "rb").read() == open(q, "rb").read()
    # output_data: ".png" in any case -> the device encoder's bytes; other extensions and DEVICE_PNG = False -> PIL
    d2, _, lab = pred._labels(data)
    streams = gpu.masks_png(lab, np.asarray(d2.binary).astype(np.uint8), cm.lut())
    arrays = dict(zip(("color", "overlay", "inverted"), gpu.masks(lab, np.asarray(d2.binary).astype(np.uint8), cm.lut())[:3]))
    for name in ("page.png", "PAGE.PNG", "sub/page.jpg"):
        root = tmp_path / ("o_" + name.replace("/", "_"))
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(root / sub)
        output.output_data(str(root), lab, dataclasses.replace(d2, output_path=name), cm)
        for sub in ("color", "overlay", "inverted"):
            blob = open(root / sub / name, "rb").read()
            if name.endswith(".jpg"):
                assert blob[:2] == b"\xff\xd8"                      # PIL picked JPEG from the extension
            else:
                assert blob == streams[sub]
    try:
        output.DEVICE_PNG = False
        root = tmp_path / "pil"
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(root / sub)
        output.output_data(str(root), lab, dataclasses.replace(d2, output_path="page.png"), cm)
        for sub in ("color", "overlay", "inverted"):
            buf = io.BytesIO()
            Image.fromarray(arrays[sub]).save(buf, format="PNG")
            assert open(root / sub / "page.png", "rb").read() == buf.getvalue()
        paths_c = pred.write_masks(data, str(tmp_path / "c"))       # ... and write_masks follows the switch
        for p, arr in zip(paths_c, want):
            buf = io.BytesIO()
            Image.fromarray(np.asarray(arr)).save(buf, format="PNG")
            assert open(p, "rb").read() == buf.getvalue()
    finally:
        output.DEVICE_PNG = True


def test_errors(gpu):
    L = gpu.lib()
    a = np.random.default_rng(9).integers(0, 256, (9, 11, 3)).astype(np.uint8)
    bound = gpu.png_bound(9, 11, 3, 0)
    buf = np.full(bound + 64, 0xA5, np.uint8)
    n = ctypes.c_size_t(12345)
    rc = L.pseg_png_encode(0, a.ctypes.data_as(ctypes.c_void_p), 9, 11, 3, 0, buf.ctypes.data_as(ctypes.c_void_p), bound - 1, ctypes.byref(n))
    assert rc == -1 and b"pseg_png_bound" in L.pseg_last_error() and (buf == 0xA5).all()
    rc = L.pseg_png_encode(0, a.ctypes.data_as(ctypes.c_void_p), 9, 11, 3, 0, buf.ctypes.data_as(ctypes.c_void_p), bound, ctypes.byref(n))
    assert rc == 0 and n.value <= bound and (buf[bound:] == 0xA5).all()
    assert np.array_equal(strict_decode(buf[:n.value].tobytes(), a.shape), a)
    for H, W, ch, br in ((9, 11, 2, 0), (9, 11, 4, 0), (0, 11, 3, 0), (9, 0, 3, 0), (9, 11, 3, -1)):
        rc = L.pseg_png_encode(0, a.ctypes.data_as(ctypes.c_void_p), H, W, ch, br, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n))
        assert rc == -1 and len(L.pseg_last_error()) > 0, (H, W, ch, br)
    assert L.pseg_png_encode(0, None, 9, 11, 3, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n)) == -1
    with pytest.raises(gpu.PsegError):
        gpu.png_encode(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(gpu.PsegError):
        gpu.png_encode(np.zeros((4, 4), np.float32))
    with pytest.raises(gpu.PsegError):
        gpu.masks_png(np.zeros((4, 4), np.int64), np.zeros((4, 5), np.uint8), np.zeros((3, 3), np.uint8))
    with pytest.raises(gpu.PsegError, match="n_lut"):
        gpu.masks_png(np.zeros((4, 4), np.int64), np.zeros((4, 4), np.uint8), np.zeros((257, 3), np.uint8))
    with pytest.raises(gpu.PsegError):
        gpu.masks_png(np.zeros((4, 4), np.int64), np.zeros((4, 4), np.uint8), np.zeros((3, 3), np.uint8), which=("colour",))
    # the workspace is released and grown again
    assert L.pseg_release_workspace(0) == 0
    check(gpu, a, 2)
