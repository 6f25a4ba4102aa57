"""The paired third cout tile (MfmaPlan::pair8; DESIGN.md section 4 "Paired third tile"): a 40-channel k5 layer under row reuse
gives the eight left-over couts of a wave's two output rows ONE A fragment per tap.  Every output still meets its taps in the old
order and the added terms are zeros, so the default plan and the plan with PSEG_NO_ROWREUSE=pair (row reuse, no pairing) must
give the same bits."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("conv2d_2", "conv2d_transpose_2")
PAIRED = "[pseg] pp launch conv2d_2: "


def _page(shape, seed=11):
    from pseg_amd import synth
    if min(shape) >= 64:
        return synth.synth_page(seed, shape[0], shape[1], 3)[0]
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _engine(gpu, arch="fcn_skip", classes=3):
    from pseg_amd import synth
    e = gpu.Engine(arch, classes, mode=gpu.MODE_BF16)
    e.set_weights(synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    return e


def _run(gpu, arch, img, classes=3):
    e = _engine(gpu, arch, classes)
    z, _, l = e.predict(img, want_probs=False)
    acts = [z, l] + [e.activation(name) for name in NAMES]
    e.close()
    return acts


def _both_arms(gpu, monkeypatch, arch, shape, classes=3):
    img = _page(shape)
    on = _run(gpu, arch, img, classes)
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "pair")
    off = _run(gpu, arch, img, classes)
    monkeypatch.delenv("PSEG_NO_ROWREUSE")
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    for act in on[2:]:
        assert np.abs(act).max() > 0
    return on


# 16 x 64: one half-resolution tile.  18 x 64: nine half-resolution rows of page.  36 x 64: nine quarter-resolution rows (deconv3).
# 70 x 50, 33 x 1, 1 x 37: ragged.  1100 x 900 and 1098 x 900: a 1120 x 928 canvas, 1050 half-resolution tiles -- conv_pp_kernel
# runs (its paired instance in the default arm) and its workgroups walk four and five tiles: both teams, both buffers, the
# accumulators and carried fragments start over at every tile.  544 x 1056: 578 tiles, workgroups of two and three.
@pytest.mark.parametrize("shape", [(16, 64), (18, 64), (36, 64), (70, 50), (33, 1), (1, 37), (160, 224), (1100, 900), (1098, 900),
                                   (544, 1056)])
def test_pair8_is_bit_identical(gpu, monkeypatch, shape):
    _both_arms(gpu, monkeypatch, "fcn_skip", shape)


@pytest.mark.parametrize("shape", [(16, 64), (36, 64), (70, 50), (33, 1), (160, 224), (256, 416)])
def test_pair8_ring_instances_are_bit_identical(gpu, monkeypatch, shape):
    """conv3 and deconv3 on conv_mfma_kernel's row-reuse instance (PSEG_NO_SP=1 in both arms keeps conv_sp_kernel from taking
    deconv3 at these page sizes): one and four channel blocks, the paired entries inside the weight ring's groups, entries 25-29 in
    the padding of every block's last group, ragged tiles, several workgroups."""
    monkeypatch.setenv("PSEG_NO_SP", "1")
    _both_arms(gpu, monkeypatch, "fcn_skip", shape)


@pytest.mark.parametrize("shape", [(70, 50), (1098, 900)])
def test_pair8_is_bit_identical_fcn(gpu, monkeypatch, shape):
    """fcn: the same layers without the skip connection."""
    _both_arms(gpu, monkeypatch, "fcn", shape)


@pytest.mark.parametrize("shape", [(70, 50), (1100, 900)])
def test_pair8_six_classes(gpu, monkeypatch, shape):
    on = _both_arms(gpu, monkeypatch, "fcn_skip", shape, classes=6)
    assert on[0].shape[-1] == 6


def test_pair8_page_unit(gpu, monkeypatch):
    """A page unit of three 70 x 50 pages (pseg_predict_pages_device) in both arms, and against the pages one by one."""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    H, W, n = 70, 50, 3
    pages = np.stack([_page((H, W), seed=11 + i) for i in range(n)])
    monkeypatch.setenv("PSEG_BATCH_PAGES", "3")

    def unit():
        eng = _engine(gpu)
        d = torch.from_numpy(pages).to(dev)
        out8 = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
        eng.predict_pages_device(d.data_ptr(), n, H, W, d_labels_u8=out8.data_ptr(), stream=st)
        torch.cuda.synchronize()
        one = [eng.predict(pages[i], want_probs=False)[2] for i in range(n)]
        eng.close()
        return out8.cpu().numpy(), one
    on, one = unit()
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "pair")
    off, _ = unit()
    assert np.array_equal(on, off)
    assert all(np.array_equal(on[i], one[i]) for i in range(n))
    assert len({p.tobytes() for p in on}) > 1


def _plan_log(gpu, capfd, shape):
    capfd.readouterr()
    e = _engine(gpu)
    e.predict(_page(shape), want_probs=False)
    e.close()
    return capfd.readouterr().err


def test_pair8_runs_by_default_and_not_under_the_switch(gpu, monkeypatch, capfd):
    """The plan log (PSEG_LOG_GENERIC): the default plan packs conv3's paired table and conv_pp_kernel launches its paired instance
    on a page with enough tiles; PSEG_NO_ROWREUSE=pair keeps row reuse and launches the unpaired one; =1 takes both away."""
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")
    log = _plan_log(gpu, capfd, (1100, 900))
    assert "[pseg] rowreuse conv2d_2: 1" in log and "[pseg] pair8 conv2d_2: 1 " in log, log
    assert re.search(re.escape(PAIRED) + r"tiles \d+ rowreuse 1 pair8 1 ", log), log
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "pair")
    log = _plan_log(gpu, capfd, (1100, 900))
    assert "[pseg] rowreuse conv2d_2: 1" in log and "[pseg] pair8 conv2d_2: 0" in log and "pair8 conv2d_2: 1" not in log, log
    assert re.search(re.escape(PAIRED) + r"tiles \d+ rowreuse 1 pair8 0 ", log) and "pair8 1 " not in log, log
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "1")
    log = _plan_log(gpu, capfd, (1100, 900))
    assert "[pseg] rowreuse conv2d_2: 0" in log and "pair8 conv2d_2: 1" not in log and "pair8 1 " not in log, log


def test_pair8_ring_instance_runs_by_default_and_not_under_the_switch(gpu, monkeypatch, capfd):
    """conv_mfma_kernel's row-reuse instance: paired for conv3 (one channel block) and deconv3 (four) on the default plan, unpaired
    under PSEG_NO_ROWREUSE=pair."""
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")
    monkeypatch.setenv("PSEG_NO_SP", "1")
    log = _plan_log(gpu, capfd, (70, 50))
    assert "[pseg] pair8 conv2d_transpose_2: 1 (4 channel block(s) x 30 entries" in log, log
    for blocks in (1, 4):
        assert "[pseg] rowreuse launch: pair8 1 (Cout 40, %d channel blocks)" % blocks in log, log
    assert "rowreuse launch: pair8 0" not in log, log
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "pair")
    log = _plan_log(gpu, capfd, (70, 50))
    for blocks in (1, 4):
        assert "[pseg] rowreuse launch: pair8 0 (Cout 40, %d channel blocks)" % blocks in log, log
    assert "pair8 1 " not in log and "[pseg] pair8 conv2d_transpose_2: 0" in log, log


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _fnv1a(b):
    h = 2166136261
    for v in b:
        h = ((h ^ int(v)) * 16777619) & 0xFFFFFFFF
    return h


def test_pair8_table_is_the_restated_packing(gpu, monkeypatch, capfd):
    """The paired table the plan uploads (its FNV-1a hash in the plan log) against a NumPy restatement: entry e = (ky', kx), lane
    (row p16, k-group g), element j -> kernel[ky', kx, 8 g + j, 32 + p16] (input channels 30, 31: zero) in rows 0-7 (zero for ky' = 5) and
    kernel[ky' - 1, kx, 8 g + j, 32 + p16 - 8] in rows 8-15 (zero for ky' = 0), rounded to bf16."""
    from pseg_amd import synth
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")
    capfd.readouterr()
    e = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_BF16)
    wts = synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05)
    e.set_weights(wts)
    e.predict(_page((16, 64)), want_probs=False)
    e.close()
    log = capfd.readouterr().err
    m = re.search(r"\[pseg\] pair8 conv2d_2: 1 \(1 channel block\(s\) x 30 entries, (\d+) bytes, fnv1a ([0-9a-f]{8});", log)
    assert m, log
    k = wts["conv2d_2/kernel"]
    assert k.shape == (5, 5, 30, 40)                      # (30 input channels in 32 storage channels: two zero k elements)
    kp = np.zeros((7, 5, 32, 8), np.float32)              # row ky' + 1: taps of ky' = -1 and 5 are zero
    kp[1:6, :, :30] = k[:, :, :, 32:40]
    tab = np.zeros((30, 64, 8), np.float32)
    for en in range(30):
        ky, kx = divmod(en, 5)
        for lane in range(64):
            g, p16 = divmod(lane, 16)
            src = kp[ky + 1, kx] if p16 < 8 else kp[ky, kx]
            tab[en, lane] = src[8 * g:8 * g + 8, p16 & 7]
    want = _bf16(tab).astype("<u2").tobytes()
    assert int(m.group(1)) == len(want) == 30 * 1024
    assert int(m.group(2), 16) == _fnv1a(want)
