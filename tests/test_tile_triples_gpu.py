"""Tile triples (conv5, conv6, deconv3 of fcn / fcn_skip on conv_mfma_kernel): one 768-thread workgroup runs three consecutive
8 x 32 tiles as three four-wave teams that share ONE weight ring in the CU's pooled LDS.  A team is the one-tile workgroup on its
own tile -- same table, k order, start value and epilogue -- so the forced plan (PSEG_TRIPLE=1: any page size) and the plan with
PSEG_NO_TRIPLE=1 (one workgroup per tile) must give the same bits.  PSEG_NO_SP=1 in both arms keeps conv_sp_kernel from taking
these page sizes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("conv2d_4", "conv2d_5", "max_pooling2d_2", "conv2d_transpose_2")


def _page(shape, seed=11):
    from pseg_amd import synth
    if min(shape) >= 64:
        return synth.synth_page(seed, shape[0], shape[1], 3)[0]
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _engine(gpu, arch):
    from pseg_amd import synth
    e = gpu.Engine(arch, 3, mode=gpu.MODE_BF16)
    e.set_weights(synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return e


def _run(gpu, arch, img):
    e = _engine(gpu, arch)
    z, _, l = e.predict(img, want_probs=False)
    acts = [z, l]
    for name in NAMES:
        try:
            acts.append(e.activation(name))
        except Exception:
            acts.append(None)                 # (fused away or absent in this graph: the same in both arms)
    e.close()
    return acts


# page -> tiles at 1/4 resolution: 1 (two idle teams), 2 (one idle team), 3 (one full triple), 1 ragged in both directions (edge
# masking), 8 ragged in x (a last triple with one idle team), 32 (several weight groups per block, two and four channel blocks)
@pytest.mark.parametrize("arch", ["fcn_skip", "fcn"])
@pytest.mark.parametrize("shape", [(32, 128), (64, 128), (96, 128), (70, 50), (128, 160), (256, 416)])
def test_triples_are_bit_identical(gpu, monkeypatch, arch, shape):
    monkeypatch.setenv("PSEG_NO_SP", "1")
    img = _page(shape)
    monkeypatch.setenv("PSEG_TRIPLE", "1")
    on = _run(gpu, arch, img)
    monkeypatch.delenv("PSEG_TRIPLE")
    monkeypatch.setenv("PSEG_NO_TRIPLE", "1")
    off = _run(gpu, arch, img)
    for a, b in zip(on, off):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b)
    # (fcn reads conv6 only through its max-pool, so conv2d_5 is not stored there: the pool, the logits and the labels carry it)
    must_have = NAMES if arch == "fcn_skip" else ("conv2d_4", "max_pooling2d_2", "conv2d_transpose_2")
    for name in must_have:
        act = on[2 + NAMES.index(name)]
        assert act is not None and np.abs(act).max() > 0, name


def test_triples_page_unit_equals_page_by_page(gpu, monkeypatch):
    """A unit of three (128, 160) pages in one launch per layer (blockIdx.z = the page slot; eight tiles per page: the last
    triple of every slot has an idle team) against the same pages one by one."""
    import torch
    monkeypatch.setenv("PSEG_NO_SP", "1")
    monkeypatch.setenv("PSEG_TRIPLE", "1")
    monkeypatch.setenv("PSEG_BATCH_PAGES", "3")
    eng = _engine(gpu, "fcn_skip")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    H, W, n = 128, 160, 3
    pages = np.stack([_page((H, W), seed=11 + i) for i in range(n)])

    def one(p):
        d = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
        lab = torch.empty(p.shape, dtype=torch.uint8, device=dev)
        eng.predict_device(d.data_ptr(), H, W, d_labels_u8=lab.data_ptr(), stream=st)
        torch.cuda.synchronize()
        return lab.cpu().numpy()
    want = [one(pages[i]) for i in range(n)]
    d = torch.from_numpy(pages).to(dev)
    out8 = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    eng.predict_pages_device(d.data_ptr(), n, H, W, d_labels_u8=out8.data_ptr(), stream=st)
    torch.cuda.synchronize()
    got = out8.cpu().numpy()
    eng.close()
    assert len({w.tobytes() for w in want}) > 1 and all(len(np.unique(w)) > 1 for w in want)     # (pages and labels that differ)
    assert all(np.array_equal(got[i], want[i]) for i in range(n))


def test_triple_switch_reaches_the_default_plan(gpu, monkeypatch, capfd):
    """The default plan marks conv5, conv6 and deconv3 for tile triples and PSEG_NO_TRIPLE=1 unmarks them: the plan log
    (PSEG_LOG_GENERIC) says which, with both ring layouts."""
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")

    def plan_log():
        capfd.readouterr()
        e = _engine(gpu, "fcn_skip")
        e.predict(_page((16, 64)), want_probs=False)     # (the weights are packed, and the plan decided, before the first page)
        e.close()
        return capfd.readouterr().err
    layers = ("conv2d_4", "conv2d_5", "conv2d_transpose_2")
    log = plan_log()
    for layer in layers:
        assert "[pseg] triple %s: 1 " % layer in log, log
    assert "triple launch" not in log, log               # (a one-tile page: the size predicate keeps the one-tile workgroups)
    # ... the forced plan launches them on this page too (what the bit-identity tests above rely on)
    monkeypatch.setenv("PSEG_NO_SP", "1")
    monkeypatch.setenv("PSEG_TRIPLE", "1")
    log = plan_log()
    for layer in layers:
        assert "[pseg] triple launch %s: tiles 1 triples 1 pages 1" % layer in log, log
    monkeypatch.delenv("PSEG_TRIPLE")
    monkeypatch.setenv("PSEG_NO_TRIPLE", "1")
    log = plan_log()
    for layer in layers:
        assert "[pseg] triple %s: 0 " % layer in log and "triple %s: 1" % layer not in log, log
    assert "triple launch" not in log, log
