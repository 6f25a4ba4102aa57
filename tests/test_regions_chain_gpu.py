"""The text regions as a stage of the page chain (pseg_predict_chain_pages_regions_png / pseg_predict_chain_scans_regions_png): every
page's "regions" -- found and traced on the device from the unit's final label maps, where they lie -- equals the host twin
(pseg_text_regions_poly_host) applied to that call's own "labels".  Everything is integer: array_equal throughout.  Same-shape and
mixed units, unit caps, the vote, the resize, regions alone, the call without the keyword, a page whose vertices overflow, and the
scan chain against the page chain on the prepared pages."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(64, 96), (70, 50), (160, 96), (130, 67), (64, 96), (160, 96), (130, 67), (64, 96)]
LABEL, KERNELS = 1, (3, 1, 2)
LUT = np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0]], np.uint8)
from pseg_amd.engine import PSEG_ENOMEM as ENOMEM, PSEG_EUNSUPPORTED as EUNSUPPORTED  # noqa: E402
RG = dict(max_regions=4096)                       # (random weights make ragged maps: a page here can have more than the default 256 regions)


def _pages():
    from pseg_amd import synth
    pages = [synth.synth_page(40 + k, H, W, 3) for k, (H, W) in enumerate(SHAPES)]
    return [p[0] for p in pages], [p[1] for p in pages]


def _engine(gpu, mode):
    from pseg_amd import synth
    eng = gpu.Engine("fcn_skip", 3, mode=mode)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return eng


@pytest.fixture(scope="module", params=["f32", "bf16"])
def eng(request, gpu):
    e = _engine(gpu, gpu.MODE_F32_EXACT if request.param == "f32" else gpu.MODE_BF16)
    yield e
    e.close()


def _how(gpu):
    return gpu.TextRegions(LABEL, kernels=KERNELS)


def _twin(gpu, labels, how=None):
    return gpu.text_regions(labels, how or _how(gpu), host=True, polygons=True, masks=False)


def _same_record(got, want, at):
    assert got["status"] == 0, (at, got["status"])
    for k in ("boxes", "areas", "seeds"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (at, k)
    assert len(got["polygons"]) == len(want["polygons"]), at
    for r, (p, q) in enumerate(zip(got["polygons"], want["polygons"])):
        assert p.dtype == np.int32 and np.array_equal(p, q), (at, r)


def _check(gpu, res, at, how=None):
    """Every page's regions against the host twin on that page's own label map -> the (regions, vertices) of the list."""
    want = _twin(gpu, [r["labels"] for r in res], how)
    for i, (r, w) in enumerate(zip(res, want)):
        _same_record(r["regions"], w, (at, i))
    return sum(len(w["polygons"]) for w in want), sum(len(p) for w in want for p in w["polygons"])


def test_regions_equal_the_host_twin_on_the_calls_own_labels(gpu, eng):
    imgs, bins = _pages()
    how = _how(gpu)
    for mixed in (False, True):
        for cap in (0, 2):
            res = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=mixed, unit_cap=cap, regions=how, **RG)
            assert all(set(r) == {"labels", "masks", "regions"} for r in res)
            _check(gpu, res, ("plain", mixed, cap))
    # the comparison is not empty: at least 8 regions of at least 8 vertices in the list
    want = _twin(gpu, [r["labels"] for r in res])
    assert sum(len(p) >= 8 for w in want for p in w["polygons"]) >= 8
    # with the vote and the masks beside it; one TextRegions per page
    res = eng.predict_chain_pages(imgs, binaries=bins, post_ops=("cc_vote",), lut=LUT, which=("color",), labels=True, mixed=True,
                                  regions=[how] * len(imgs), **RG)
    _check(gpu, res, "vote")
    plain = eng.predict_chain_pages(imgs, binaries=bins, post_ops=("cc_vote",), lut=LUT, which=("color",), labels=True, mixed=True)
    for a, b in zip(res, plain):                   # the stage changes nothing else
        assert np.array_equal(a["labels"], b["labels"]) and a["masks"] == b["masks"]
    # with the resize: the regions are those of the resized map
    outs = [(H * 2 - 3, W + 5) for H, W in SHAPES]
    for mixed in (False, True):
        res = eng.predict_chain_pages(imgs, out_shapes=outs, which=(), labels=True, mixed=mixed, regions=how, **RG)
        assert all(r["labels"].shape == o for r, o in zip(res, outs))
        _check(gpu, res, ("resize", mixed))
    # the resize and the box filling: the final map is the second of the ping-pong pair
    res = eng.predict_chain_pages(imgs, out_shapes=outs, post_ops=("bbox",), which=(), labels=True, mixed=True, regions=how, **RG)
    _check(gpu, res, "resize + bbox")


def test_regions_alone_and_the_call_without_the_keyword(gpu, eng):
    imgs, _ = _pages()
    how = _how(gpu)
    for mixed in (False, True):
        full = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=mixed, regions=how, **RG)
        alone = eng.predict_chain_pages(imgs, which=(), labels=False, mixed=mixed, regions=how, **RG)
        for i, (a, b) in enumerate(zip(alone, full)):
            assert a["labels"] is None and a["masks"] == {}
            _same_record(a["regions"], b["regions"], ("alone", mixed, i))
        none = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=mixed, regions=None)
        bare = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=mixed)
        for a, b, c in zip(none, bare, full):
            assert set(a) == set(b) == {"labels", "masks"} and a["masks"] == b["masks"] == {}
            assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["labels"], c["labels"])
    seen = []
    assert eng.predict_chain_pages(imgs[:3], which=(), labels=True, regions=how, **RG, sink=lambda page, name, item: seen.append((page, name))) is None
    assert seen == [(0, "labels"), (0, "regions"), (1, "labels"), (1, "regions"), (2, "labels"), (2, "regions")]
    with pytest.raises(gpu.PsegError):
        eng.predict_chain_pages(imgs, which=(), regions=[how])
    with pytest.raises(gpu.PsegError):
        eng.predict_chain_pages(imgs, which=(), regions=how, max_regions=0)


def test_a_page_whose_vertices_or_regions_overflow(gpu, eng):
    imgs, _ = _pages()
    how = _how(gpu)
    full = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=True, regions=how, **RG)
    totals = [sum(len(p) for p in r["regions"]["polygons"]) for r in full]
    counts = [len(r["regions"]["polygons"]) for r in full]
    top = max(totals)
    assert top > min(totals)
    res = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=True, regions=how, **RG, max_vertices=top - 1)
    for i, (r, f) in enumerate(zip(res, full)):
        if totals[i] == top:
            assert r["regions"]["status"] == ENOMEM and r["regions"]["polygons"] is None
            for k in ("boxes", "areas", "seeds"):
                assert np.array_equal(r["regions"][k], f["regions"][k]), (i, k)
        else:
            _same_record(r["regions"], f["regions"], ("neighbour", i))
    most = max(counts)
    assert most > min(counts)
    res = eng.predict_chain_pages(imgs, which=(), labels=True, mixed=True, regions=how, max_regions=most - 1)
    for i, (r, f) in enumerate(zip(res, full)):
        if counts[i] == most:
            assert r["regions"]["status"] == EUNSUPPORTED and r["regions"]["polygons"] is None and len(r["regions"]["boxes"]) == 0
        else:
            _same_record(r["regions"], f["regions"], ("neighbour", i))


def test_scan_chain_equals_the_page_chain_on_the_prepared_pages(gpu, eng):
    from pseg_amd import engine as E
    from pseg_amd import synth
    scans = [(255 - synth.synth_page(60 + k, H, W, 3)[0]).astype(np.uint8) for k, (H, W) in enumerate([(128, 192), (140, 100), (200, 134), (128, 192)])]
    scales = [0.5, 0.6, 0.75, 0.5]
    how = _how(gpu)
    prep = E.prepare_scans(scans, scales)
    pages = eng.predict_chain_pages([p[0] for p in prep], which=(), labels=True, mixed=True, regions=how, **RG)
    got = eng.predict_chain_scans(scans, scales, which=(), labels=True, regions=how, **RG)
    assert sum(len(r["regions"]["polygons"]) for r in pages) > 0
    for i, (a, b) in enumerate(zip(got, pages)):
        assert np.array_equal(a["labels"], b["labels"])
        _same_record(a["regions"], b["regions"], ("scans", i))
    _check(gpu, got, "scans")
    bare = eng.predict_chain_scans(scans, scales, which=(), labels=True)
    assert all(set(r) == {"labels", "masks"} and np.array_equal(r["labels"], g["labels"]) for r, g in zip(bare, got))


def test_predict_regions_chain_route_equals_the_list_route(gpu, oracle_mod):
    """Polygon by polygon, with a page that only the fallback can take among them (a page the list chain refuses)."""
    from test_eval_pages_gpu import _predictor_and_dataset
    total = 0
    for posts, high_res in (([], False), (["cc_majority"], True)):
        pred, ds = _predictor_and_dataset(gpu, oracle_mod, posts, high_res)
        for k, d in enumerate(ds.data):
            d.line_height_px = 4 + k
        refused = np.shape(ds.data[1].image)[:2]
        takes = pred._list_takes
        pred._list_takes = lambda shape: tuple(shape[:2]) != tuple(refused) and takes(shape)
        assert any(not pred._list_takes(np.shape(d.image)[:2]) for d in ds.data)
        for chunk in (64, 2):
            want = pred.predict_regions(ds, 1, chunk=chunk, route="list")
            got = pred.predict_regions(ds, 1, chunk=chunk, route="chain")
            assert len(got) == len(want) == len(ds.data)
            for a, b in zip(got, want):
                assert len(a) == len(b)
                for r, q in zip(a, b):
                    assert np.array_equal(r.polygon, q.polygon) and r.box == q.box and r.area == q.area and r.seed == q.seed
                total += len(a)
        assert [len(a) for a in pred.predict_regions(ds, 1)] == [len(a) for a in want]          # the default route
        with pytest.raises(Exception):
            pred.predict_regions(ds, 1, route="other")
    assert total > 0


@pytest.mark.parametrize("high_res", [False, True])
def test_write_masks_scans_with_regions(gpu, tmp_path, high_res):
    """The mask files are byte-equal to the call without `regions`; the regions equal predict_regions on the loaded entries: entries
    with a line height, one measured in the call, and one on the fallback route."""
    import dataclasses
    import test_chain_scans_gpu as S
    from ocr4all_pixel_classifier.lib.dataset import Dataset, DatasetLoader
    from pseg_amd import engine as E
    scans = [(S._text_scan(40 + k, s[0], s[1]),) for k, s in enumerate(S.SCAN_SHAPES)]
    pred, cm = S._predictor(gpu, ["cc_majority"], high_res)
    loader = DatasetLoader(S.TARGET_LINE_HEIGHT, cm, prediction=True)
    entries = S._entries(tmp_path, scans)
    measured = E.char_heights([scans[2][0]], inverse=False)[0][0]
    if measured is not None:
        entries[2] = dataclasses.replace(entries[2], line_height_px=None)       # measured in the call
    entries[4] = dataclasses.replace(entries[4], output_path="fifth.jpg")         # not a PNG target: the fallback route
    plain = list(pred.write_masks_scans([dataclasses.replace(e) for e in entries], loader, str(tmp_path / "plain"), level=0))
    seen = []
    mine = [dataclasses.replace(e) for e in entries]
    got = list(pred.write_masks_scans(mine, loader, str(tmp_path / "regions"), level=0, chunk_pages=4, regions=cm,
                                      on_regions=lambda k, regs: seen.append((k, regs))))
    assert S._rel(got, tmp_path / "regions") == S._rel(plain, tmp_path / "plain") and S._files(got) == S._files(plain)
    assert [k for k, _ in seen] == list(range(len(entries)))
    if measured is not None:
        assert mine[2].line_height_px == measured
    loaded = [loader.load_images(dataclasses.replace(e, line_height_px=m.line_height_px)) for e, m in zip(entries, mine)]
    want = pred.predict_regions(Dataset(loaded, cm), cm, route="list")
    total = 0
    for (k, regs), w in zip(seen, want):
        assert len(regs) == len(w), k
        for r, q in zip(regs, w):
            assert np.array_equal(r.polygon, q.polygon) and r.box == q.box and r.area == q.area and r.seed == q.seed, k
        total += len(regs)
    assert total > 0
    with pytest.raises(Exception):
        list(pred.write_masks_scans(mine, loader, str(tmp_path / "bad"), regions=1))
