"""The two-set pipeline that pseg_predict_batch and the page chain share (run_pipeline, csrc/pseg_common.h), where the other chain
tests do not reach: page-locked caller arrays (the direct-DMA branch of upload, alone and beside pageable pages of the same unit), one
engine through every list entry with its staging growing, trimmed and growing again, and the empty and the single-page list.  Every
comparison is for equal bytes: against the same call with pageable arrays, against a fresh engine, against the page-by-page chain."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("color", "overlay", "inverted", "fg_color")
LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
SHAPES = [(96, 64)] * 3 + [(70, 50)] * 2 + [(160, 224)]
OUT = [None, (120, 80), None, None, (141, 91), None]
# the three smallest scans of test_chain_scans_gpu.py's list, built as there
SCAN_SHAPES = [(150, 110), (180, 150), (240, 130)]
SCAN_SEEDS = [40, 41, 43]
SCALES = [0.9, 0.5, 0.4]


def _engine(gpu, mode):
    from pseg_amd import synth
    eng = gpu.Engine("fcn_skip", 3, mode=mode)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return eng


@pytest.fixture(scope="module")
def engines(gpu):
    engs = {"f32": _engine(gpu, gpu.MODE_F32_EXACT), "bf16": _engine(gpu, gpu.MODE_BF16)}
    yield engs
    for e in engs.values():
        e.close()


@pytest.fixture(scope="module")
def pages(gpu):
    """Per page: image, binarisation at the final shape."""
    from pseg_amd import synth
    out = []
    for k, s in enumerate(SHAPES):
        img, binary, _ = synth.synth_page(60 + k, s[0], s[1], 3)
        if OUT[k] is not None:
            binary = (np.random.default_rng(60 + k).random(OUT[k]) < 0.2).astype(np.uint8)
        out.append((img, binary))
    return out


@pytest.fixture(scope="module")
def scans(gpu):
    from pseg_amd import synth
    return [(255 - synth.synth_page(k, s[0], s[1], 3)[0]).astype(np.uint8) for k, s in zip(SCAN_SEEDS, SCAN_SHAPES)]


def _same(got, want, at):
    assert len(got) == len(want), at
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["labels"] is None) == (w["labels"] is None), at + (k,)
        if w["labels"] is not None:
            assert g["labels"].shape == w["labels"].shape and g["labels"].tobytes() == w["labels"].tobytes(), at + (k,)
        assert sorted(g["masks"]) == sorted(w["masks"]), at + (k,)
        for name in w["masks"]:
            assert g["masks"][name] == w["masks"][name], at + (k, name)


def _chain(eng, imgs, bins, level, mixed):
    return eng.predict_chain_pages(imgs, binaries=bins, out_shapes=OUT, post_ops=["cc_vote"], lut=LUT, labels=True, png_level=level,
                                   unit_cap=2, mixed=mixed)


@pytest.mark.parametrize("mode_name", ["f32", "bf16"])
@pytest.mark.parametrize("level", [0, 1])
def test_page_locked_inputs(gpu, engines, pages, scans, mode_name, level):
    from pseg_amd import engine as E
    eng = engines[mode_name]
    imgs, bins = [p[0] for p in pages], [p[1] for p in pages]
    # with pages 0 and 3 alone page-locked, a unit of the mixed planner holds both kinds
    order, units = E.chain_units_mixed(SHAPES, cap=2)
    assert any(0 < sum(order[f + k] in (0, 3) for k in range(c)) < c for f, c in units), units
    all_locked = ([E.pinned_copy(a) for a in imgs], [E.pinned_copy(b) for b in bins])
    some = ([E.pinned_copy(a) if k in (0, 3) else a for k, a in enumerate(imgs)],
            [E.pinned_copy(b) if k in (0, 3) else b for k, b in enumerate(bins)])
    for mixed in (False, True):
        want = _chain(eng, imgs, bins, level, mixed)
        assert all(len(w["masks"]) == 3 and w["labels"] is not None for w in want)
        _same(_chain(eng, all_locked[0], all_locked[1], level, mixed), want, ("all page-locked", mixed))
        _same(_chain(eng, some[0], some[1], level, mixed), want, ("pages 0 and 3 page-locked", mixed))
    kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, png_level=level, unit_cap=2)
    want = eng.predict_chain_scans(scans, SCALES, **kw)
    _same(eng.predict_chain_scans([E.pinned_copy(s) for s in scans], SCALES, **kw), want, ("scans page-locked",))
    _same(eng.predict_chain_scans([E.pinned_copy(scans[0])] + scans[1:], SCALES, **kw), want, ("scan 0 page-locked",))


def test_one_engine_through_every_entry(gpu, pages, scans):
    """predict_batch, the three list entries, growth, trim and the small lists again on ONE engine: each result is what a fresh
    engine gives for that call alone; a sink that raises in the middle of a call leaves the next call intact."""
    small = [pages[0][0], pages[1][0], pages[2][0]] * 2                          # 6 pages of 96x64
    small_bins = [pages[0][1], pages[0][1], pages[2][1]] * 2                     # (page 1's own binarisation has its out-shape)
    large = [pages[5][0]] * 3                                                    # 3 pages of 160x224
    imgs, bins = [p[0] for p in pages], [p[1] for p in pages]
    kw = dict(post_ops=["cc_vote"], lut=LUT, labels=True, unit_cap=2)
    calls = {
        "batch": lambda e: [{"labels": lab, "masks": {}} for lab in e.predict_batch(small, dtype=np.uint8)],
        "pages": lambda e: e.predict_chain_pages(small, binaries=small_bins, **kw),
        "mixed": lambda e: e.predict_chain_pages(imgs, binaries=bins, out_shapes=OUT, mixed=True, **kw),
        "scans": lambda e: e.predict_chain_scans(scans, SCALES, **kw),
        "large": lambda e: e.predict_chain_pages(large, binaries=[pages[5][1]] * 3, **kw),
    }
    want = {}
    for name, call in calls.items():
        fresh = _engine(gpu, gpu.MODE_BF16)
        want[name] = call(fresh)
        fresh.close()
    eng = _engine(gpu, gpu.MODE_BF16)

    class Stop(Exception):
        pass

    def raising(page, name, data):
        if page == 3:
            raise Stop("page 3")

    for step, name in enumerate(["batch", "pages", "mixed", "raise", "scans", "large", "trim", "pages", "batch"]):
        if name == "raise":
            with pytest.raises(Stop, match="page 3"):
                eng.predict_chain_pages(imgs, binaries=bins, out_shapes=OUT, mixed=True, sink=raising, **{k: v for k, v in kw.items() if k != "labels"})
        elif name == "trim":
            eng.trim()
        else:
            _same(calls[name](eng), want[name], (step, name))
    eng.close()


def test_empty_and_single(gpu, pages, scans):
    eng = _engine(gpu, gpu.MODE_BF16)
    # an empty list is answered in front of any device work: on an engine that has run nothing, and behind a call
    for _ in range(2):
        assert eng.predict_chain_pages([], lut=LUT) == []
        assert eng.predict_chain_pages([], lut=LUT, mixed=True) == []
        assert eng.predict_chain_scans([], [], lut=LUT) == []
        img, binary = pages[3]
        one = eng.predict_chain(img, binary=binary, post_ops=["cc_vote"], labels="u8", lut=LUT, masks="png")
        want = [{"labels": np.array(one["labels"]), "masks": dict(zip(NAMES[:3], one["masks"]))}]
        for mixed in (False, True):
            got = eng.predict_chain_pages([img], binaries=[binary], post_ops=["cc_vote"], lut=LUT, labels=True, mixed=mixed)
            _same(got, want, ("one page", mixed))
    eng.close()
