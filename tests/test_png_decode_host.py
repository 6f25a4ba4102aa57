"""The PNG reader without a device: pseg_png_probe and pseg_png_decode_gray_host -- the shared core (csrc/pseg_pngdec.h) the
kernels are compiled from, run serially -- against PIL on files written by tests/pngdec_cases.py."""
import numpy as np
import pytest

import pngdec_cases as C


def _host(files):
    import pseg_amd
    return pseg_amd.png_decode_gray(files, host=True)


def _check_list(cases, got):
    assert len(got) == len(cases)
    for (name, _, want), (arr, st) in zip(cases, got):
        assert st == C.OK, (name, st)
        assert arr.dtype == np.uint8 and arr.shape == want.shape, name
        assert np.array_equal(arr, want), name


def test_the_synthetic_page_meets_every_block_type():
    page = [(n, d) for n, d, _ in C.matrix() if n.startswith("300x330")]
    assert len(page) == 7
    types = {n.rsplit("-", 1)[1]: C.block_types(C.idat_payload(d)) for n, d in page}
    assert types == {"l0": 0, "l1": 2, "l6": 2, "l9": 2, "huff": 2, "rle": 2, "fixed": 1}
    raw_len = 300 * (1 + 330 * 3)
    assert raw_len > 65535                        # level 0 spans more than one stored block
    parts = [n.split("-") for n, _, _ in C.matrix()]
    assert len(parts) == 63
    assert {p[0] for p in parts} == {"%dx%d" % s for s in C.SHAPES} and {p[1] for p in parts} == {"gray", "rgb"}
    assert {p[2] for p in parts} == {"f%s" % m for m in C.FILTER_MODES} and {p[3] for p in parts} == {z[0] for z in C.ZLIB_SETTINGS}


def test_matrix_equals_pil():
    cases = C.matrix()
    _check_list(cases, _host([d for _, d, _ in cases]))


def test_matrix_one_file_at_a_time_and_probe():
    import pseg_amd
    for name, data, want in C.matrix()[::4]:
        assert pseg_amd.png_probe(data)[:3] == (C.OK, want.shape[0], want.shape[1]), name
        (arr, st), = _host([data])
        assert st == C.OK and np.array_equal(arr, want), name


def test_idat_splits_and_pil_files():
    cases = C.splits()
    _check_list(cases, _host([d for _, d, _ in cases]))
    import pseg_amd
    for name, data, want in cases:
        st, H, W, ch = pseg_amd.png_probe(data)
        assert (st, H, W) == (C.OK, want.shape[0], want.shape[1]) and ch in (1, 3), name


def test_hand_assembled_fixed_streams():
    cases = C.hand_streams()
    assert [n for n, _, _ in cases] == ["far", "run", "overlap", "empty-stored"]
    for name, data, want in cases:
        assert np.array_equal(C.pil_gray(data), want), name
    _check_list(cases, _host([d for _, d, _ in cases]))


def test_refusals_leave_output_and_neighbours_alone():
    import ctypes
    import pseg_amd
    good = C.matrix()[3]
    files = [good[1]] + [d for _, d in C.refusals()] + [good[1]]
    got = _host(files)
    assert np.array_equal(got[0][0], good[2]) and np.array_equal(got[-1][0], good[2])
    for (name, data), (arr, st) in zip(C.refusals(), got[1:-1]):
        assert st == C.EUNSUPPORTED and arr is None, (name, st)
        assert pseg_amd.png_probe(data)[0] == C.EUNSUPPORTED, name
        assert C.container_ok(data) and C.pil_gray(data).shape == (20, 30), name          # a sound PNG, PIL reads it
    # the output bytes of a refused file are untouched (the C entry, with a buffer of its own)
    L = pseg_amd.lib()
    for name, data in C.refusals()[:2] + [(n, d) for n, d, *_ in C.corrupt()[5:8]]:
        out = np.full(20 * 30 * 8, 0xA5, np.uint8)
        st = (ctypes.c_int * 1)(7)
        rc = L.pseg_png_decode_gray_host(1, (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)),
                                         (ctypes.c_size_t * 1)(len(data)), (ctypes.c_void_p * 1)(out.ctypes.data), st)
        assert rc == 0 and st[0] in (C.EUNSUPPORTED, C.EINVAL) and (out == 0xA5).all(), name


def test_corrupt_corpus_is_refused_with_einval():
    import pseg_amd
    cases = C.corrupt()
    assert len(cases) == 15
    for name, data, W, H, bpp in cases:
        assert C.is_corrupt(data, W, H, bpp), name                     # established without the decoder under test
    good = C.matrix()[3]
    got = _host([good[1]] + [d for _, d, *_ in cases] + [good[1]])
    assert np.array_equal(got[0][0], good[2]) and np.array_equal(got[-1][0], good[2])
    for (name, data, *_), (arr, st) in zip(cases, got[1:-1]):
        assert st == C.EINVAL and arr is None, (name, st)
    for name, data, *_ in cases:
        st = pseg_amd.png_probe(data)[0]
        assert st == (C.OK if C.container_ok(data) else C.EINVAL), name   # the container alone: the stream's faults show in the decode


def test_probe_values_and_the_empty_list():
    import pseg_amd
    assert pseg_amd.png_decode_gray([], host=True) == []
    assert pseg_amd.png_decode_gray([]) == []                          # n == 0: before a device is touched
    assert pseg_amd.png_probe(b"")[0] == C.EINVAL and pseg_amd.png_probe(b"not a png at all")[0] == C.EINVAL
    rgb = [c for c in C.matrix() if "-rgb-" in c[0]][0]
    assert pseg_amd.png_probe(rgb[1]) == (C.OK,) + rgb[2].shape + (3,)
    assert pseg_amd.png_probe(dict(C.refusals())["rgba"]) == (C.EUNSUPPORTED, 20, 30, 4)
    unknown = C.assemble(30, 20, 0, C.deflate(bytes(20 * 31)), before=(C.chunk(b"XYZa", b"?"),))
    assert pseg_amd.png_probe(unknown)[0] == C.EUNSUPPORTED            # a critical chunk the reader does not know
    late = C.SIG + C.chunk(b"pHYs", bytes(9)) + C.ihdr(3, 3) + C.chunk(b"IDAT", C.deflate(bytes(12))) + C.chunk(b"IEND")
    assert pseg_amd.png_probe(late)[0] == C.EINVAL                     # IHDR is not first
    s = C.deflate(bytes(12))
    gap = C.SIG + C.ihdr(3, 3) + C.chunk(b"IDAT", s[:4]) + C.chunk(b"tEXt", b"a\0b") + C.chunk(b"IDAT", s[4:]) + C.chunk(b"IEND")
    assert pseg_amd.png_probe(gap)[0] == C.EINVAL                      # IDAT chunks are consecutive


def test_gray_conversion_is_pils():
    r = np.random.RandomState(5)
    a = r.randint(0, 256, (40, 50, 3)).astype(np.uint8)
    data = C.make_png(a, 0, 1)
    (arr, st), = _host([data])
    want = ((a[..., 0].astype(np.uint32) * 19595 + a[..., 1].astype(np.uint32) * 38470 + a[..., 2].astype(np.uint32) * 7471 + 0x8000) >> 16).astype(np.uint8)
    assert st == C.OK and np.array_equal(arr, want) and np.array_equal(C.pil_gray(data), want)


@pytest.mark.gpu
def test_round_trip_with_the_device_encoder(gpu):
    r = np.random.RandomState(9)
    for level in (0, 1):
        for a in (C.synth(70, 50, False, 1), C.synth(65, 130, True, 2), r.randint(0, 256, (33, 17)).astype(np.uint8)):
            data = gpu.png_encode(a, level=level)
            want = a if a.ndim == 2 else ((a[..., 0].astype(np.uint32) * 19595 + a[..., 1].astype(np.uint32) * 38470 + a[..., 2].astype(np.uint32) * 7471 + 0x8000) >> 16).astype(np.uint8)
            assert np.array_equal(C.pil_gray(data), want)
            for host in (True, False):
                (arr, st), = gpu.png_decode_gray([data], host=host)
                assert st == C.OK and np.array_equal(arr, want), (level, a.shape, host)
