"""The bf16 engine's two address maps (DESIGN.md section 3 "Two address maps"): the entries that return label maps alone run on one
arena per page slot in which a tensor takes the bytes of dead tensors; pseg_predict and calls that ask for logits keep one buffer
per tensor.  Every kernel gets the same operands at other addresses, so the label maps must be the same bits -- also when the arena
is full of NaN bytes before every run (PSEG_COMPACT_POISON=1: a tensor wrongly planned as "written whole by its producer" would
show), and when real data of another page and another canvas lies in it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 70 x 50: ragged edge tiles; 33 x 37: one tile at every scale, a smaller canvas than the run before it; 96 x 160: several tiles
# and the narrow tile of the 1/8-resolution layers, a larger canvas than the run before it.
SHAPES = ((70, 50), (33, 37), (96, 160))
ARCHS = ("fcn_skip", "fcn", "unet", "res_unet")


def _page(shape, seed):
    from pseg_amd import synth
    if min(shape) >= 64:
        return synth.synth_page(seed, shape[0], shape[1], 3)[0]
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _engine(gpu, arch, classes, plan):
    from pseg_amd import synth
    e = gpu.Engine(arch, classes, mode=gpu.MODE_BF16, plan=plan)
    e.set_weights(synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return e


def _device_labels(eng, img):
    """pseg_predict_device, labels alone: (uint8 map, int64 map)"""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    H, W = img.shape
    d = torch.from_numpy(img).to(dev)
    u8 = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
    i64 = torch.full((H, W), -1, dtype=torch.int64, device=dev)
    eng.predict_device(d.data_ptr(), H, W, d_labels=i64.data_ptr(), d_labels_u8=u8.data_ptr(), stream=st)
    torch.cuda.synchronize()
    eng.status()
    return u8.cpu().numpy(), i64.cpu().numpy()


@pytest.mark.parametrize("classes", [3, 6])
@pytest.mark.parametrize("arch", ARCHS)
def test_compact_map_gives_the_same_label_maps(gpu, arch, classes):
    """Default (compact) plan, the same with the arena poisoned before every run, and PSEG_NO_COMPACT=1, one engine each, over pages
    of a shrinking and then growing canvas: stale bytes of real data are in place from the second page on."""
    engs = {"compact": _engine(gpu, arch, classes, ""), "poison": _engine(gpu, arch, classes, "PSEG_COMPACT_POISON=1"),
            "full": _engine(gpu, arch, classes, "PSEG_NO_COMPACT=1")}
    try:
        seen = set()
        for i, shape in enumerate(SHAPES):
            img = _page(shape, 11 + i)
            want = engs["full"].predict(img, want_logits=False, want_probs=False)[2]
            assert want.shape == shape and 0 <= want.min() and want.max() < classes
            for name, eng in engs.items():
                u8, i64 = _device_labels(eng, img)
                assert np.array_equal(i64, want), (name, shape)
                assert np.array_equal(u8, want.astype(np.uint8)), (name, shape)
            # the compact engines' own pseg_predict (the full map of the same engine) agrees too
            assert np.array_equal(engs["compact"].predict(img, want_logits=False, want_probs=False)[2], want)
            seen.add(want.tobytes())
        assert len(seen) == len(SHAPES)
    finally:
        for e in engs.values():
            e.close()


@pytest.mark.parametrize("plan", ["", "PSEG_COMPACT_POISON=1"])
def test_page_unit_on_the_compact_map(gpu, monkeypatch, plan):
    """Three 70 x 50 pages as one unit (pseg_predict_pages_device: a slot of the arena per page, the low-resolution layers over all
    slots in one launch) against the pages one by one through pseg_predict."""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    H, W, n = 70, 50, 3
    pages = np.stack([_page((H, W), 21 + i) for i in range(n)])
    monkeypatch.setenv("PSEG_BATCH_PAGES", "3")
    for arch in ("fcn_skip", "unet"):
        eng = _engine(gpu, arch, 3, plan)
        d = torch.from_numpy(pages).to(dev)
        out8 = torch.full((n, H, W), 255, dtype=torch.uint8, device=dev)
        out64 = torch.full((n, H, W), -1, dtype=torch.int64, device=dev)
        for _ in range(2):                                   # (the second unit finds the first one's bytes in every slot)
            eng.predict_pages_device(d.data_ptr(), n, H, W, d_labels=out64.data_ptr(), d_labels_u8=out8.data_ptr(), stream=st)
        torch.cuda.synchronize()
        eng.status()
        one = [eng.predict(pages[i], want_logits=False, want_probs=False)[2] for i in range(n)]
        eng.close()
        got8, got64 = out8.cpu().numpy(), out64.cpu().numpy()
        for i in range(n):
            assert np.array_equal(got64[i], one[i]) and np.array_equal(got8[i], one[i].astype(np.uint8)), (arch, i)
        assert len({p.tobytes() for p in got8}) > 1


def test_compact_map_is_the_default_and_has_a_switch(gpu, monkeypatch, capfd):
    """The plan log prints the arena table when a labels-only call lays out its canvas -- by default, not under PSEG_NO_COMPACT=1,
    and not for pseg_predict; its total is pseg_plan_arena's."""
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")
    img = _page((70, 50), 41)
    _, arena, _ = gpu.plan_arena("fcn_skip", 70, 50)
    for plan, entry, logged in (("", "device", True), ("PSEG_NO_COMPACT=1", "device", False), ("", "predict", False)):
        e = _engine(gpu, "fcn_skip", 3, plan)
        capfd.readouterr()
        if entry == "device":
            _device_labels(e, img)
        else:
            e.predict(img, want_logits=False, want_probs=False)
        err = capfd.readouterr().err
        e.close()
        assert ("[pseg] arena plan 96x64: 10 tensors, arena %d bytes" % arena in err) == logged, (plan, entry, err[-2000:])
        if logged:
            assert "skip_logits" in err and "shared" in err


def test_activations_come_from_the_full_map(gpu):
    """pseg_get_activation answers from the last run on the full map: equal to the PSEG_NO_COMPACT engine's after predict, refused
    with the documented message while only labels-only entries have run, and untouched by a predict_device that follows a predict."""
    names = ("max_pooling2d", "conv2d_2", "conv2d_4", "conv2d_transpose_2")
    img, other = _page((70, 50), 31), _page((96, 160), 32)
    a, b = _engine(gpu, "fcn_skip", 3, ""), _engine(gpu, "fcn_skip", 3, "PSEG_NO_COMPACT=1")
    try:
        _device_labels(a, img)
        with pytest.raises(gpu.PsegError, match="labels-only entries do not materialise activations"):
            a.activation("conv2d_2")
        za, _, la = a.predict(img, want_probs=False)
        zb, _, lb = b.predict(img, want_probs=False)
        assert np.array_equal(za, zb) and np.array_equal(la, lb)
        acts = {n: a.activation(n) for n in names}
        for n in names:
            assert np.abs(acts[n]).max() > 0 and np.array_equal(acts[n], b.activation(n)), n
        _device_labels(a, other)                               # another page, another canvas, on the compact map
        _device_labels(a, img)
        for n in names:
            assert np.array_equal(a.activation(n), acts[n]), n   # still the predict run's tensors
        a.trim()
        with pytest.raises(gpu.PsegError):
            a.activation("conv2d_2")
    finally:
        a.close()
        b.close()
