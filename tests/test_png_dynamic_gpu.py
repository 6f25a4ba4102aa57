"""Level 1 of the device PNG encoder (csrc/pseg_png.hip): one dynamic Huffman code per band where it beats the fixed code.
Every stream goes through the two decoders of tests/test_png_gpu.py (its strict zlib decoder and PIL); PNG is lossless, so a
valid file that decodes to the source is correct.  Level 0 is pinned by SHA-256 digests recorded on the commit before level 1
existed (tests/golden/png_level0_sha256.json)."""
import hashlib
import io
import json
import os
import struct

import numpy as np
import pytest

from test_png_gpu import strict_decode, patches, _synth_masks, _predictor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_level0_sha256.json")
NAMES = ("color", "overlay", "inverted", "fg_color")


def check1(gpu, a, band_rows=0):
    """Encode at level 1, decode with both decoders, compare, check the bound; -> the stream."""
    from PIL import Image
    png = gpu.png_encode(a, band_rows=band_rows, level=1)
    assert np.array_equal(strict_decode(png, a.shape), a), (a.shape, band_rows)
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.mode == ("RGB" if a.ndim == 3 else "L") and np.array_equal(np.asarray(im), a), (a.shape, band_rows)
    ch = 3 if a.ndim == 3 else 1
    assert len(png) <= gpu.png_bound(a.shape[0], a.shape[1], ch, band_rows, level=1)
    return png


def band_chunks(png):
    """The bodies of the IDAT chunks that hold bands: all but the first (zlib header) and the last (final block, Adler-32)."""
    pos, idat = 8, []
    while pos < len(png):
        n, = struct.unpack(">I", png[pos:pos + 4])
        if png[pos + 4:pos + 8] == b"IDAT":
            idat.append(png[pos + 8:pos + 8 + n])
        pos += 12 + n
    assert len(idat) >= 3 and idat[0] == b"\x78\x01" and len(idat[-1]) == 9
    return idat[1:-1]


def all_lengths_row():
    """For every n in 3..258 a pixel of a new value followed by n repeats: every length symbol and every extra-bit count."""
    parts, v = [], 0
    for n in range(3, 259):
        v = (v + 37) % 251 + 1                                     # differs from the value before it
        parts.append(np.full(n + 1, v, np.uint8))
    row = np.concatenate(parts)
    assert row.size == 33664
    return row.reshape(1, -1)


def adler_cases():
    rng = np.random.default_rng(4)
    col = np.zeros((40, 1536, 3), np.uint8)
    col[::2] = 255
    return [("random", rng.integers(0, 256, (40, 1536, 3)).astype(np.uint8)), ("all255", np.full((40, 1536, 3), 255, np.uint8)),
            ("altrows", col)]


def level0_cases(gpu):
    """[(key, callable(**kw) -> bytes)]: the level-0 streams whose digests the golden file holds; kw is {} or {"level": 0}."""
    cases = []

    def enc(key, a, band_rows):
        cases.append(("%s/br%d" % (key, band_rows), lambda **kw: gpu.png_encode(a, band_rows=band_rows, **kw)))

    t = patches(np.random.default_rng(1703), 17, 87, 3)
    enc("tiny17x87x3", t, 0)
    enc("tiny17x87x3", t, 2)
    enc("tiny3x22x1", patches(np.random.default_rng(301), 3, 22, 1), 1)
    enc("tiny1x3x3", patches(np.random.default_rng(103), 1, 3, 3), 0)
    row = all_lengths_row()
    enc("lengths", row, 1)
    enc("lengths", row, 0)
    ad = dict(adler_cases())
    enc("adler_random", ad["random"], 16)
    enc("adler_altrows", ad["altrows"], 16)
    enc("adler256_all255", np.full((256, 256, 3), 255, np.uint8), 0)
    pred, binary, lut = _synth_masks(gpu, 0, 384, 512, 3)
    cases.append(("masks384x512/br0", lambda **kw: b"".join(gpu.masks_png(pred, binary, lut, **kw)[n] for n in NAMES[:3])))
    p6, b6, l6 = _synth_masks(gpu, 1, 160, 224, 6)
    cases.append(("masks160x224x6/br5", lambda **kw: b"".join(gpu.masks_png(p6, b6, l6, which=NAMES, band_rows=5, **kw)[n] for n in NAMES)))
    return cases


# ---- 1, 2: tiny and ragged shapes, the fixed fallback ---------------------------------------------------------------------
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("H", [1, 2, 3, 17])
def test_tiny_and_ragged_shapes(gpu, H, ch):
    rng = np.random.default_rng(100 * H + ch)
    for W in (1, 2, 3, 21, 22, 85, 86, 87):
        a = patches(rng, H, W, ch)
        for band_rows in (1, 2, 3, 0):
            png = check1(gpu, a, band_rows)
            if band_rows:
                png0 = gpu.png_encode(a, band_rows=band_rows)
                assert len(png) <= len(png0), (H, W, ch, band_rows, len(png), len(png0))
                if H == 1 and W <= 3:                              # a dynamic header alone is longer than these bands
                    assert png == png0
                    assert all(c[0] & 7 == 2 for c in band_chunks(png))


# ---- 3: all length symbols ------------------------------------------------------------------------------------------------
def test_all_length_symbols(gpu):
    png = check1(gpu, all_lengths_row(), 1)
    bands = band_chunks(png)
    assert len(bands) == 1 and bands[0][0] & 7 == 4                # BFINAL 0, BTYPE 10


# ---- 4: the length limit --------------------------------------------------------------------------------------------------
def fibonacci_row():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    row = np.repeat(np.arange(24, dtype=np.uint8) * 9 + 3, fib)
    assert row.size == 121392
    rng = np.random.default_rng(11)
    rng.shuffle(row)
    for _ in range(64):                                            # re-draw until no three consecutive pixels are equal
        bad = np.flatnonzero((row[2:] == row[1:-1]) & (row[1:-1] == row[:-2])) + 1
        if bad.size == 0:
            break
        for i, j in zip(bad.tolist(), rng.integers(0, row.size, bad.size).tolist()):
            row[i], row[j] = row[j], row[i]
    assert not ((row[2:] == row[1:-1]) & (row[1:-1] == row[:-2])).any()
    assert np.array_equal(np.bincount(row // 9, minlength=24), fib)
    return row.reshape(1, -1)


def test_length_limit(gpu):
    """24 literals with Fibonacci counts: the unconstrained Huffman tree is 23 deep, deflate allows 15."""
    png = check1(gpu, fibonacci_row(), 1)
    bands = band_chunks(png)
    assert len(bands) == 1 and bands[0][0] & 7 == 4


# ---- 5: one segment far above 9 bits per byte -----------------------------------------------------------------------------
def test_segment_local_expansion(gpu):
    """40 rows of 4096 filtered bytes = 40 segments.  39 rows alternate two values; one row holds 250 other values 16 times each,
    whose codes are 13 bits and longer: that segment needs far more than the 9 bits per byte of the fixed code."""
    W = 4095
    filt = np.empty((40, W), np.uint8)
    filt[:, 0::2], filt[:, 1::2] = 1, 2
    rng = np.random.default_rng(12)
    rare = np.resize(np.arange(3, 253, dtype=np.uint8), W)
    rng.shuffle(rare)
    while (rare[1:] == rare[:-1]).any():
        rng.shuffle(rare)
    filt[20] = rare
    a = np.cumsum(filt.astype(np.int64), axis=0).astype(np.uint8)
    png = check1(gpu, a, 40)
    bands = band_chunks(png)
    assert len(bands) == 1 and bands[0][0] & 7 == 4
    assert len(png) < a.size / 4                                   # two alternating literals: a bit or two each


# ---- 6: Adler-32 and the band combine -------------------------------------------------------------------------------------
def test_adler_and_band_combine(gpu):
    for _, a in adler_cases():
        check1(gpu, a, 16)
    check1(gpu, np.full((256, 256, 3), 255, np.uint8), 0)
    check1(gpu, np.full((256, 256, 3), 255, np.uint8), 256)


# ---- 7: masks -------------------------------------------------------------------------------------------------------------
def test_masks(gpu):
    from PIL import Image
    pred, binary, lut = _synth_masks(gpu, 0, 384, 512, 3)
    want = dict(zip(NAMES, gpu.masks(pred, binary, lut)))
    l0 = gpu.masks_png(pred, binary, lut)
    l1 = gpu.masks_png(pred, binary, lut, level=1)
    assert sorted(l1) == ["color", "inverted", "overlay"]
    for n in NAMES[:3]:
        assert np.array_equal(strict_decode(l1[n], want[n].shape), want[n]), n
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(l1[n]))), want[n]), n
        buf = io.BytesIO()
        Image.fromarray(want[n]).save(buf, format="PNG")
        pil = len(buf.getvalue())
        print("masks 384x512 %-8s level 1 %6d  level 0 %6d  PIL %6d  -> %.3f of level 0, %.3f of PIL"
              % (n, len(l1[n]), len(l0[n]), pil, len(l1[n]) / len(l0[n]), len(l1[n]) / pil))
        assert len(l1[n]) <= 0.5 * len(l0[n]), (n, len(l1[n]), len(l0[n]))
        assert len(l1[n]) <= 1.5 * pil, (n, len(l1[n]), pil)
    assert gpu.masks_png(pred, binary, lut, level=1) == l1         # deterministic bytes
    pred, binary, lut = _synth_masks(gpu, 1, 160, 224, 6)
    want = dict(zip(NAMES, gpu.masks(pred, binary, lut)))
    got = gpu.masks_png(pred, binary, lut, which=NAMES, level=1)
    assert sorted(got) == sorted(NAMES)
    for n in NAMES:
        assert np.array_equal(strict_decode(got[n], want[n].shape), want[n]), n
    sub = gpu.masks_png(pred, binary, lut, which=("inverted", "color"), band_rows=5, level=1)
    assert sorted(sub) == ["color", "inverted"]
    for n in sub:
        assert np.array_equal(strict_decode(sub[n], want[n].shape), want[n]), n
        assert len(sub[n]) <= gpu.png_bound(160, 224, 3, 5, level=1)
    assert gpu.masks_png(pred, binary, lut, which=NAMES, level=1) == got


# ---- 8: chain and files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(96, 64), (160, 224)])
def test_chain_png_level1(gpu, oracle_mod, shape):
    from pseg_amd import synth
    img, binary, _ = synth.synth_page(4, shape[0], shape[1], 3)
    eng = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_F32_EXACT)
    eng.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    lut = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
    out_shape = (shape[0] + 71, shape[1] + 41)
    big_bin = (np.random.default_rng(1).random(out_shape) < 0.2).astype(np.uint8)
    try:
        for posts, osh, b in ((["cc_vote"], None, binary), (["cc_vote", "bbox"], out_shape, big_bin)):
            want = eng.predict_chain(img, binary=b, out_shape=osh, post_ops=posts, labels="u8", lut=lut, masks=True)
            got = eng.predict_chain(img, binary=b, out_shape=osh, post_ops=posts, labels="u8", lut=lut, masks="png", png_level=1)
            assert np.array_equal(got["labels"], want["labels"])
            assert len(got["masks"]) == 4 and all(isinstance(m, bytes) for m in got["masks"])
            for png, arr in zip(got["masks"], want["masks"]):
                assert np.array_equal(strict_decode(png, arr.shape), arr), (posts, osh)
            l0 = eng.predict_chain(img, binary=b, out_shape=osh, post_ops=posts, labels="u8", lut=lut, masks="png")
            assert sum(map(len, got["masks"])) < sum(map(len, l0["masks"]))
    finally:
        eng.close()


@pytest.mark.parametrize("posts,high_res", [(["cc_majority"], False), (["cc_majority", "bounding_boxes"], True)])
def test_write_masks_and_output_data_level1(gpu, oracle_mod, tmp_path, posts, high_res):
    import dataclasses
    from PIL import Image
    from ocr4all_pixel_classifier.lib import output
    pred, data, cm = _predictor(gpu, oracle_mod, (96, 64), posts, high_res, tmp_path / "a")
    m = pred.predict_masks(data)
    want = (m.color, m.overlay, m.inverted_overlay)
    assert output.DEVICE_PNG_LEVEL == 0
    paths0 = pred.write_masks(data, str(tmp_path / "l0"))
    paths = pred.write_masks(data, level=1)                        # the argument, the module value at 0
    blobs = [open(p, "rb").read() for p in paths]
    for p, blob, arr in zip(paths, blobs, want):
        assert np.array_equal(strict_decode(blob, arr.shape), arr)
        assert np.array_equal(np.asarray(Image.open(p)), arr)
    assert sum(map(len, blobs)) < sum(os.path.getsize(p) for p in paths0)
    d2, _, lab = pred._labels(data)
    arrays = dict(zip(("color", "overlay", "inverted"), gpu.masks(lab, np.asarray(d2.binary).astype(np.uint8), cm.lut())[:3]))
    streams = gpu.masks_png(lab, np.asarray(d2.binary).astype(np.uint8), cm.lut(), level=1)
    try:
        output.DEVICE_PNG_LEVEL = 1
        paths_b = pred.write_masks(data, str(tmp_path / "b"))      # None -> the module value
        assert [open(p, "rb").read() for p in paths_b] == blobs
        root = tmp_path / "o"
        for sub in ("color", "overlay", "inverted"):
            os.makedirs(root / sub)
        output.output_data(str(root), lab, dataclasses.replace(d2, output_path="page.png"), cm)
        for sub in ("color", "overlay", "inverted"):
            blob = open(root / sub / "page.png", "rb").read()
            assert blob == streams[sub]
            assert np.array_equal(strict_decode(blob, arrays[sub].shape), arrays[sub])
            assert np.array_equal(np.asarray(Image.open(root / sub / "page.png")), arrays[sub])
    finally:
        output.DEVICE_PNG_LEVEL = 0


# ---- 9: errors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, -1])
def test_bad_level(gpu, oracle_mod, tmp_path, level):
    a = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(gpu.PsegError):
        gpu.png_bound(4, 5, 3, 0, level=level)
    with pytest.raises(gpu.PsegError):
        gpu.png_encode(a, level=level)
    with pytest.raises(gpu.PsegError):
        gpu.masks_png(np.zeros((4, 5), np.int64), np.zeros((4, 5), np.uint8), np.zeros((3, 3), np.uint8), level=level)
    pred, data, _ = _predictor(gpu, oracle_mod, (96, 64), ["cc_majority"], False, tmp_path)
    with pytest.raises(gpu.PsegError):
        pred.write_masks(data, level=level)
    from pseg_amd import synth
    img, binary, _ = synth.synth_page(4, 96, 64, 3)
    e = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_F32_EXACT)
    e.set_weights(oracle_mod.init_weights("fcn_skip", 3, seed=42, gain=1.5, bias_scale=0.05))
    try:
        with pytest.raises(gpu.PsegError):
            e.predict_chain(img, binary=binary, post_ops=["cc_vote"], labels="u8", lut=np.zeros((3, 3), np.uint8), masks="png", png_level=level)
    finally:
        e.close()


# ---- 10: level 0 is what it was -------------------------------------------------------------------------------------------
def test_level0_unchanged(gpu):
    golden = json.load(open(GOLDEN))
    cases = level0_cases(gpu)
    assert sorted(golden) == sorted(k for k, _ in cases)
    for key, fn in cases:
        assert hashlib.sha256(fn()).hexdigest() == golden[key], key
        assert hashlib.sha256(fn(level=0)).hexdigest() == golden[key], key + " with level=0"
