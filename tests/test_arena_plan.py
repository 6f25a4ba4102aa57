"""The compact address map of the bf16 engine (pseg_plan_arena: host arithmetic, no GPU): a tensor takes the bytes of tensors whose
last reader has run, and never anything else's."""
import itertools

import pytest

import pseg_amd

ARCHS = ("fcn_skip", "fcn", "unet", "res_unet")
SHAPES = ((64, 96), (2048, 1536))
MB = 1e6


def _plan(arch, shape, classes, plan=None):
    rows, arena, full = pseg_amd.plan_arena(arch, shape[0], shape[1], n_classes=classes, plan=plan)
    assert len(rows) >= 1 and arena > 0 and full > 0
    return rows, arena, full


def _check(rows, arena, full):
    for r in rows:
        assert r["offset"] % 256 == 0, r
        assert r["bytes"] > 0 and r["offset"] >= 0 and r["offset"] + r["bytes"] <= arena, r
        assert 0 <= r["producer"] <= r["last_reader"], r
    # live range = producer launch .. last reader launch, both included
    for a, b in itertools.combinations(rows, 2):
        live = a["producer"] <= b["last_reader"] and b["producer"] <= a["last_reader"]
        bytes_ = a["offset"] < b["offset"] + b["bytes"] and b["offset"] < a["offset"] + a["bytes"]
        assert not (live and bytes_), (a, b)
        if bytes_:                                   # only tensors written whole by their producers share bytes
            assert a["shared"] and b["shared"], (a, b)
    assert arena <= full
    assert len({r["name"] for r in rows}) == len(rows)


@pytest.mark.parametrize("classes", [3, 6])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("arch", ARCHS)
def test_live_tensors_never_overlap(arch, shape, classes):
    _check(*_plan(arch, shape, classes))


def test_fcn_skip_page_fits_the_infinity_cache():
    """2048x1536, three classes: the whole arena, skip-logits plane included, stays under 240 MB (the page and the label map are the
    caller's) -- the full map is 0.96 GB."""
    rows, arena, full = _plan("fcn_skip", (2048, 1536), 3)
    assert arena <= 240 * MB, arena
    assert full >= 900 * MB
    by = {r["name"]: r for r in rows}
    assert by["skip_logits"]["bytes"] == 2048 * 1536 * 16
    assert by["skip_logits"]["producer_name"] == "conv2d_1" and by["skip_logits"]["last_reader_name"] == "conv2d_transpose_4"
    # the tensors that live inside fused kernels have no row: conv1, conv2, conv4, deconv1, deconv4, deconv5, the input
    assert not {"input", "conv2d", "conv2d_1", "conv2d_3", "conv2d_transpose", "conv2d_transpose_3", "conv2d_transpose_4"} & set(by)
    # pooled conv2 is dead after conv3: pooled conv4 and conv5 sit in its bytes
    p2 = by["max_pooling2d"]
    for name in ("max_pooling2d_1", "conv2d_4"):
        assert p2["offset"] <= by[name]["offset"] and by[name]["offset"] + by[name]["bytes"] <= p2["offset"] + p2["bytes"], name


@pytest.mark.parametrize("plan", ["PSEG_NO_DQ=1", "PSEG_NO_SKIPLOG=1", "PSEG_NO_TAIL_FUSION=1", "PSEG_NO_CONV1_FUSION=1", "PSEG_NO_POOL_ONLY=1"])
def test_plan_follows_the_fusion_switches(plan):
    """A fusion that is switched off turns a tensor that lived inside a kernel into one a launch writes and another reads."""
    base = {r["name"] for r in _plan("fcn_skip", (96, 160), 3)[0]}
    rows, arena, full = _plan("fcn_skip", (96, 160), 3, plan=plan)
    _check(rows, arena, full)
    names = {r["name"] for r in rows}
    assert names != base
    if plan == "PSEG_NO_DQ=1":
        # the stand-alone Conv2DTranspose k2 s2 stores 60 of deconv2's 64 storage channels: private, once-zeroed bytes
        d2 = [r for r in rows if r["name"] == "conv2d_transpose_1"][0]
        assert not d2["shared"] and "conv2d_transpose" in names
    if plan == "PSEG_NO_SKIPLOG=1":
        assert "skip_logits" not in names and "conv2d_1" in names


def test_three_channel_input_is_staged():
    rows, arena, full = pseg_amd.plan_arena("fcn_skip", 64, 96, n_classes=3, in_channels=3)
    _check(rows, arena, full)
    inp = [r for r in rows if r["name"] == "input"][0]
    assert inp["producer"] == 0 and inp["producer_name"] == "preprocess"


def test_bad_arguments():
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.plan_arena("fcn_skip", 0, 96)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.plan_arena(99, 64, 96)
