"""Row reuse in the k5 conv kernels (four chunks per pixel: conv3, deconv3, conv6 of fcn / fcn_skip): a wave keeps the pixel
fragments that its two output rows share in registers instead of reading them from LDS twice.  Same operands in the same order
for every accumulator, so the default plan and the plan with PSEG_NO_ROWREUSE=1 (the old loops) must give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ("conv2d_2", "max_pooling2d_1", "conv2d_transpose_2", "conv2d_5")


def _page(shape, seed=11):
    from pseg_amd import synth
    if min(shape) >= 64:
        return synth.synth_page(seed, shape[0], shape[1], 3)[0]
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _run(gpu, arch, img):
    from pseg_amd import synth
    e = gpu.Engine(arch, 3, mode=gpu.MODE_BF16)
    e.set_weights(synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    z, _, l = e.predict(img, want_probs=False)
    acts = [z, l]
    for name in NAMES:
        try:
            acts.append(e.activation(name))
        except Exception:
            acts.append(None)                 # (fused away or absent in this graph: the same in both arms)
    e.close()
    return acts


def _both_arms(gpu, monkeypatch, arch, shape, must_have):
    img = _page(shape)
    on = _run(gpu, arch, img)
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "1")
    off = _run(gpu, arch, img)
    monkeypatch.delenv("PSEG_NO_ROWREUSE")
    for a, b in zip(on, off):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b)
    for name in must_have:
        act = on[2 + NAMES.index(name)]
        assert act is not None and np.abs(act).max() > 0, name


@pytest.mark.parametrize("arch", ["fcn_skip", "fcn"])
@pytest.mark.parametrize("shape", [(16, 64), (33, 1), (70, 50), (160, 224), (544, 1056)])
def test_rowreuse_conv3_is_bit_identical(gpu, monkeypatch, arch, shape):
    """conv3 (conv2d_2): one tile, ragged edges, many one-tile workgroups, and 544 x 1056 -- 578 half-resolution tiles on 256 CUs,
    where conv_pp_kernel runs and its workgroups walk two and three tiles (both teams, both buffers, an odd count): the carried
    fragments start over at every tile."""
    _both_arms(gpu, monkeypatch, arch, shape, ("conv2d_2",))


@pytest.mark.parametrize("arch", ["fcn_skip", "fcn"])
@pytest.mark.parametrize("shape", [(70, 50), (160, 224), (256, 416)])
def test_rowreuse_deconv3_conv6_are_bit_identical(gpu, monkeypatch, arch, shape):
    """deconv3 (conv2d_transpose_2) and conv6 (conv2d_5) on the conv_mfma_kernel instances (PSEG_NO_SP=1 in both arms keeps
    conv_sp_kernel from taking these page sizes): four and two channel blocks, several weight groups, ragged tiles."""
    monkeypatch.setenv("PSEG_NO_SP", "1")
    # (fcn reads conv6 only through its max-pool, so conv2d_5 is not stored there: the logits and labels carry it)
    _both_arms(gpu, monkeypatch, arch, shape, ("conv2d_transpose_2", "conv2d_5") if arch == "fcn_skip" else ("conv2d_transpose_2",))


def test_rowreuse_switch_reaches_the_default_plan(gpu, monkeypatch, capfd):
    """The default plan marks conv3 for row reuse and PSEG_NO_ROWREUSE=1 unmarks it: the plan log (PSEG_LOG_GENERIC) says which."""
    from pseg_amd import synth
    monkeypatch.setenv("PSEG_LOG_GENERIC", "1")

    def plan_log():
        capfd.readouterr()
        e = gpu.Engine("fcn_skip", 3, mode=gpu.MODE_BF16)
        e.set_weights(synth.glorot_weights(e.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
        e.predict(_page((16, 64)), want_probs=False)     # (the weights are packed, and the plan decided, before the first page)
        e.close()
        return capfd.readouterr().err
    log = plan_log()
    assert "[pseg] rowreuse conv2d_2: 1" in log, log
    monkeypatch.setenv("PSEG_NO_ROWREUSE", "1")
    log = plan_log()
    assert "[pseg] rowreuse conv2d_2: 0" in log and "rowreuse conv2d_2: 1" not in log, log
