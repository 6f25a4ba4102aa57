"""unet and res_unet on pages large enough for their size-dependent plans.

Both engines pick kernels and grids from a page's tile count, so the plans these graphs run on real pages are not the ones the
small-page tests (tests/test_predict_gpu.py, tests/test_bf16_gpu.py, tests/test_train_arch_gpu.py) reach:
- bf16 engine: res_unet's first stride-2 layers (conv_block 1 and the shortcut of the first residual block, 32 -> 64) walk their
  4 x 32 tiles on 2 x CUs persistent workgroups once the grid holds more than twice that many tiles
  (conv_mfma_kernel<2, 4, 3, 2, 4, MODE_CONV, FL_PERSIST[ | FL_INRELU]>, mfma_launch_conv), in page units too (slot by slot).
- float32 engine: the cout tiles per workgroup (NT) of the blocked chain drop to 1 while tiles x cout blocks < 1024
  (launch_conv_exact_mfma), so every 3x3 layer of a small page runs conv_xb_kernel<*, 1, *>.
- train step: wgrad_blk_plan splits a 64 x 64 layer's rows into column groups only when the page is wide and tall enough.
Each test restates the plan arithmetic it relies on (the library has no plan introspection) and asserts that its page reaches
the plan -- from the device's CU count where the plan depends on it -- instead of skipping.  Bars are those of the small-page
tests: float32 bit for bit, bf16 logits within 3 % and activations within 2 % of the tensor's magnitude, gradients within
2e-4 (unet, routed max-pool referee) / 2e-3 (res_unet) of their scale."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 0.02            # bf16 activations (tests/test_bf16_gpu.py)
LOGIT_TOL = 0.03      # bf16 logits of the 19- and 23-conv graphs (tests/test_bf16_gpu.py)
LARGE = (1024, 768)   # (H, W): 1536 stride-2 tiles, three per persistent workgroup on 256 CUs
RAGGED = (1100, 1300)  # padded to 1120 x 1312: 2940 stride-2 tiles, an uneven last trip on 512 workgroups


def _cdiv(a, b):
    return -(-a // b)


def _pad32(n):
    return _cdiv(n, 32) * 32


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _s2_tiles(H, W):
    """bf16 engine: 4 x 32 output tiles of res_unet's first stride-2 layers (half resolution of the padded page)."""
    return _cdiv(_pad32(W) // 2, 32) * _cdiv(_pad32(H) // 2, 4)


def _persistent(H, W):
    """mfma_launch_conv: a k3 stride-2 single-block layer runs persistent when its grid exceeds 2 x slots, slots = 2 x CUs (the
    three-workgroup form wg3 is stride-1 only)."""
    return _s2_tiles(H, W) > 4 * _cus()


def _assert_persistent(H, W, want=True):
    t, cus = _s2_tiles(H, W), _cus()
    assert _persistent(H, W) == want, "%dx%d page: %d stride-2 tiles against 4 x %d CUs -- the persistent walk is %s" % (
        H, W, t, cus, "not reached" if want else "reached")


def _exact_plan(Hout, Wout, Cout, stride):
    """launch_conv_exact_mfma's blocked chain for a 3x3 layer -> (output rows per tile, cout tiles per workgroup NT, cout blocks):
    8-row tiles unless the halo slab exceeds 52 KB (stride 2), at most four cout tiles split evenly over the blocks, NT lowered
    while tiles x blocks < 1024, one block for 3 or 4 tiles on >= 512 tiles."""
    twh = 31 * stride + 3
    rows = 8 if (7 * stride + 3) * twh * 18 * 4 <= 52 * 1024 else 4
    tiles = _cdiv(Wout, 32) * _cdiv(Hout, rows)
    ntall = _cdiv(Cout, 16)
    nblk = _cdiv(ntall, 4)
    nt = _cdiv(ntall, nblk)
    while nt > 1 and tiles * nblk < 1024:
        nt -= 1
        nblk = _cdiv(ntall, nt)
    nt = _cdiv(ntall, nblk)
    if ntall in (3, 4) and nblk == 2 and tiles >= 512:
        nt, nblk = ntall, 1
    return rows, nt, nblk


def _exact_wide(arch, H, W):
    """The layer whose cout-tile instance a page of this size changes: res_unet's 32 -> 64 stride-2 conv (4-row tiles,
    conv_xb_kernel<2, NT>), unet's 64 -> 64 full-resolution conv (8-row tiles, conv_xb_kernel<4, NT>)."""
    Hp, Wp = _pad32(H), _pad32(W)
    return _exact_plan(Hp // 2, Wp // 2, 64, 2) if arch == "res_unet" else _exact_plan(Hp, Wp, 64, 1)


def _wgrad_blk_plan(Hy, Wy, cus):
    """wgrad_blk_plan for a 3x3 stride-1 layer with a 64-channel source and 64 output channels (the 64 x 64 instance, one
    workgroup per CU, one channel block) -> (column groups, row strips)."""
    cpr = _cdiv(Wy, 32)
    target = max(1, cus)
    cg = cpr
    while True:
        rows = _cdiv(Hy, max(1, target // cg))
        if rows >= 8 or cg == 1:
            break
        cg = _cdiv(cg, 2)
    cg = _cdiv(cpr, _cdiv(cpr, cg))
    return cg, _cdiv(Hy, rows)


def _check_labels(pred, logit, logit_o):
    """(flips outside the oracle's near-ties, all flips) -- tests/test_bf16_gpu.py"""
    pred_o = np.argmax(logit_o, -1)
    srt = np.sort(logit_o, -1)
    margin = srt[..., -1] - srt[..., -2]
    err = float(np.abs(logit - logit_o).max())
    bad = (pred != pred_o) & (margin > 2 * err + 1e-6)
    return int(bad.sum()), int((pred != pred_o).sum())


def _layers(Wt):
    """Conv layer names in graph order, the logits layer (not an activation) left out."""
    return [n for n in dict.fromkeys(k.split("/")[0] for k in Wt) if n != "logits"]


def _activation(eng, name):
    """The stored tensor, or None for one the plan never writes (raises "fused")."""
    import pseg_amd
    try:
        return eng.activation(name)
    except pseg_amd.PsegError as ex:
        assert "fused" in str(ex), ex
        return None


# ---------------------------------------------------------------------------------------------------------------------------
# A. float32 engine, bit for bit


@pytest.mark.parametrize("arch,shape", [("unet", LARGE), ("unet", RAGGED), ("res_unet", LARGE), ("res_unet", RAGGED),
                                        ("res_unet", (2048, 1536))],
                         ids=["unet-1024x768", "unet-1100x1300", "res_unet-1024x768", "res_unet-1100x1300", "res_unet-2048x1536"])
def test_exact_mode_large_page_bit_identical(gpu, oracle_mod, arch, shape):
    """The float32 engine (Network's default) against the oracle, bit for bit, on pages where the blocked chain keeps several
    cout tiles per workgroup: res_unet's 32 -> 64 stride-2 conv on 4-row tiles with NT = 4 (1536 / 2940 / 6144 tiles), its
    64 -> 128 stride-2 conv with NT = 3 over three blocks (3 + 3 + 2) at 1024x768, and its 256 -> 512 stride-2 conv with NT = 3
    over eleven blocks at 2048x1536; unet's 64-channel full-resolution convs with NT = 4 on 8-row tiles and its 256-channel
    quarter-resolution convs with NT = 3 over six blocks (3 x 5 + 1).  The small-page tests run conv_xb_kernel<*, 1, *> on
    every one of these layers.  1024x768: logits, labels and every activation; the ragged page (padded to 1120 x 1312) and
    2048x1536: logits and labels."""
    H, W = shape
    rows, nt, _ = _exact_wide(arch, H, W)
    assert rows == (4 if arch == "res_unet" else 8) and nt == 4, (arch, shape, rows, nt)
    if arch == "res_unet" and shape == LARGE:
        assert _exact_plan(H // 4, W // 4, 128, 2) == (4, 3, 3)
    if arch == "res_unet" and shape == (2048, 1536):
        assert _exact_plan(H // 16, W // 16, 512, 2) == (4, 3, 11)
    if arch == "unet" and shape == LARGE:
        assert _exact_plan(H // 4, W // 4, 256, 1) == (8, 3, 6)
    rng = np.random.default_rng(H + W)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    Wt = oracle_mod.init_weights(arch, 3, seed=23, gain=1.5, bias_scale=0.05)
    eng = gpu.Engine(arch, 3, mode=gpu.MODE_F32_EXACT)
    eng.set_weights(Wt)
    z, _, pred = eng.predict(img, want_probs=False)
    if shape == LARGE:
        z_o, acts = oracle_mod.forward(arch, Wt, img, "f32", return_acts=True)
        for name, a in acts.items():
            if name != "logits":
                assert np.array_equal(eng.activation(name), a), name
        del acts
    else:
        z_o = oracle_mod.forward(arch, Wt, img, "f32")
    eng.close()
    assert np.array_equal(z, z_o), "logits differ: max |d| = %g" % np.abs(z - z_o).max()
    assert np.array_equal(pred, np.argmax(z_o, -1))


# ---------------------------------------------------------------------------------------------------------------------------
# B. bf16 engine: res_unet's persistent stride-2 layers, unet on a large page

# Label flips against the bf16 oracle, all of them at near-ties (bad == 0 below): measured once on the MI355X (384 / 722 of
# 0.79 / 1.43 M pixels for res_unet, 4145 of 0.79 M for unet), recorded with 2x headroom.  The near-tie rule alone cannot catch
# a kernel that drifts: a flip only needs an oracle margin within twice the largest logit error, and that error is the bar.
_FLIPS = {("res_unet", LARGE): 768, ("res_unet", RAGGED): 1444, ("unet", LARGE): 8290}


@pytest.mark.parametrize("shape", [LARGE, RAGGED], ids=["1024x768", "1100x1300"])
def test_bf16_res_unet_persistent_stride2_layers(gpu, oracle_mod, shape):
    """res_unet's first residual block on a page over the persistence threshold: conv_block 1 (pre-activation ReLU) and the
    shortcut run conv_mfma_kernel<2, 4, 3, 2, 4, MODE_CONV, FL_INRELU | FL_PERSIST> / <..., FL_PERSIST>, 2 x CUs workgroups
    walking three tiles each (1024x768: 1536 tiles on 512 workgroups) or 5.74 (1100x1300: 2940 tiles, an uneven last trip).
    Against the same engine with PSEG_NO_PERSIST (one tile per workgroup): the same products in the same order, so the same bits
    in the logits, the labels and every stored tensor -- with the default plan and with PSEG_NO_RELU_FWD, which keeps conv_block
    1's own output (the default stores it ReLU'd for its only reader).  Against the bf16 oracle: logits within 3 %, stored
    activations within 2 % (1024x768; the ragged page's tensors stay on the device), labels = argmax of the returned logits and
    equal to the oracle's except at near-ties, a recorded cap on those."""
    from pseg_amd import synth
    H, W = shape
    _assert_persistent(H, W)
    img = synth.synth_page(40, H, W, 3)[0]
    Wt = oracle_mod.init_weights("res_unet", 3, seed=42, gain=1.5, bias_scale=0.05)
    if shape == LARGE:
        z_o, acts_o = oracle_mod.forward("res_unet", Wt, img, "bf16", return_acts=True)
    else:
        z_o, acts_o = oracle_mod.forward("res_unet", Wt, img, "bf16"), None
    for base in ({}, {"PSEG_NO_RELU_FWD": "1"}):
        engs, outs = [], []
        for plan in (base, dict(base, PSEG_NO_PERSIST="1")):
            e = gpu.Engine("res_unet", 3, mode=gpu.MODE_BF16, plan=plan)
            e.set_weights(Wt)
            outs.append(e.predict(img, want_probs=False))
            engs.append(e)
        (z, _, pred), (z_n, _, pred_n) = outs
        assert np.array_equal(z, z_n) and np.array_equal(pred, pred_n), base
        stored = []
        for name in _layers(Wt):
            a, a_n = _activation(engs[0], name), _activation(engs[1], name)
            assert (a is None) == (a_n is None), (base, name)
            if a is None:
                continue
            assert np.array_equal(a, a_n), (base, name)
            stored.append(name)
            if acts_o is not None:
                err = np.abs(a - acts_o[name]).max()
                assert err <= TOL * max(1.0, np.abs(acts_o[name]).max()), "%s: max err %g" % (name, err)
        for e in engs:
            e.close()
        # the first residual block: conv_block 1 (stored raw only under PSEG_NO_RELU_FWD), conv_block 2 (+ the shortcut), shortcut;
        # the default plan stores the 11 tensors read only through pre-activation ReLUs ReLU'd, both plans fuse d4's conv_block 2
        # into the logits layer
        assert {"conv2d_4", "conv2d_5"} <= set(stored) and ("conv2d_3" in stored) == bool(base), (base, stored)
        assert len(stored) >= len(_layers(Wt)) - (1 if base else 12), (base, stored)
        err = float(np.abs(z - z_o).max())
        assert err <= LOGIT_TOL * max(1.0, float(np.abs(z_o).max())), "logits off by %g" % err
        assert np.array_equal(pred, np.argmax(z, -1))
        bad, total = _check_labels(pred, z, z_o)
        assert bad == 0, "%d label mismatches outside near-ties (%d total)" % (bad, total)
        assert total <= _FLIPS[("res_unet", shape)], "%d label flips against the bf16 oracle" % total


def test_bf16_unet_large_page_vs_bf16_oracle(gpu, oracle_mod):
    """unet on the bf16 engine at 1024x768 (every 3x3 layer on a grid of hundreds to thousands of tiles, the quarter-resolution
    and deeper layers over the XCD-banded tile order of a many-workgroup grid) against the bf16 oracle: logits within 3 %, every
    stored activation within 2 %, labels = argmax of the returned logits, equal to the oracle's except at near-ties, and a
    recorded cap on those."""
    from pseg_amd import synth
    H, W = LARGE
    _assert_persistent(H, W)
    img = synth.synth_page(41, H, W, 3)[0]
    Wt = oracle_mod.init_weights("unet", 3, seed=42, gain=1.5, bias_scale=0.05)
    z_o, acts_o = oracle_mod.forward("unet", Wt, img, "bf16", return_acts=True)
    eng = gpu.Engine("unet", 3, mode=gpu.MODE_BF16)
    eng.set_weights(Wt)
    z, _, pred = eng.predict(img, want_probs=False)
    checked = 0
    for name in _layers(Wt):
        a = _activation(eng, name)
        if a is None:
            continue
        checked += 1
        err = np.abs(a - acts_o[name]).max()
        assert err <= TOL * max(1.0, np.abs(acts_o[name]).max()), "%s: max err %g" % (name, err)
    eng.close()
    assert checked >= len(acts_o) - 3
    err = float(np.abs(z - z_o).max())
    assert err <= LOGIT_TOL * max(1.0, float(np.abs(z_o).max())), "logits off by %g" % err
    assert np.array_equal(pred, np.argmax(z, -1))
    bad, total = _check_labels(pred, z, z_o)
    assert bad == 0, "%d label mismatches outside near-ties (%d total)" % (bad, total)
    assert total <= _FLIPS[("unet", LARGE)], "%d label flips against the bf16 oracle" % total


# ---------------------------------------------------------------------------------------------------------------------------
# C. train step with column groups
# (one plan of one wgrad_blk_kernel instance, through a whole step; test_wgrad_layers_gpu.py runs every instance of every
# weight-gradient kernel on its own, exactly, under every strip plan)


@pytest.mark.parametrize("arch", ["unet", "res_unet"])
def test_train_step_column_groups_match_float64_autograd(gpu, oracle_mod, arch):
    """A 256x384 train step, where wgrad_blk_plan splits the 64 x 64 layers (unet's conv2d_1, its last decoder level; res_unet's
    d4 conv_block 2) into 12 column groups x 20 row strips on 256 CUs (wgrad_blk_kernel with grid.y = 240: per-strip bias
    partials, the column walk starting at pc0 = cper x group); the tests at 64x96 and below run one column group.  Against
    torch autograd of the same graph in float64: loss within 1e-4 relative, every gradient within 2e-4 of its scale for unet
    and 2e-3 for res_unet.  unet runs two steps, so that the Dropout masks change; its referee takes the max-pool winners AND
    the ReLU decisions from the float32 forward of that step (Dropout included), which the engine reproduces bit for bit.  With
    the pools routed alone, pre-activations within rounding of zero decide differently in float64 and move whole pixel
    contributions of the 1/16-resolution layers (384 pixels here): 3.4e-3 on conv2d_10/kernel, and as much against a float32
    referee, while the column-group kernel agrees with the other weight-gradient kernels (PSEG_WGRAD_NO_BLK) to 6e-7."""
    from oracle.train_ref import graph_loss_and_grads
    from pseg_amd import synth
    H, W, C = 256, 384, 3
    cg, strips = _wgrad_blk_plan(H, W, _cus())
    assert cg > 1, "%dx%d on %d CUs: wgrad_blk_plan keeps one column group" % (H, W, _cus())
    Wt = oracle_mod.init_weights(arch, C, seed=11, gain=1.2, bias_scale=0.05)
    img, _, mask = synth.synth_page(3, H, W, C)
    eng = gpu.Engine(arch, C, mode=gpu.MODE_F32_EXACT)
    eng.set_weights(Wt)
    eng.train_init(clipnorm=1.0)

    def compare(g, g_o, bar):
        assert list(g.keys()) == list(g_o.keys())
        for k in g_o:
            scale = np.abs(g_o[k]).max() + 1e-12
            err = np.abs(g[k] - g_o[k]).max()
            assert err <= bar * scale + 1e-9, "%s: max err %g vs scale %g" % (k, err, scale)
    if arch == "unet":
        eng.train_set_dropout_seed(77)
        for step in range(2):
            acts = oracle_mod.forward(arch, Wt, img, "f32", return_acts=True, drop=(77, step))[1]
            loss_o, g_o, _ = graph_loss_and_grads(arch, Wt, img, mask, drop=(77, step), float64=True, route_acts=acts, route_relu=True)
            del acts
            loss = eng.train_forward_backward(img, mask)[0]
            assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (step, loss, loss_o)
            compare(eng.gradients(), g_o, 2e-4)
    else:
        loss_o, g_o, _ = graph_loss_and_grads(arch, Wt, img, mask, float64=True)
        loss = eng.train_forward_backward(img, mask)[0]
        assert abs(loss - loss_o) <= 1e-4 * abs(loss_o), (loss, loss_o)
        compare(eng.gradients(), g_o, 2e-3)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# D. one engine across the thresholds

SEQ_SHAPES = [(64, 96), LARGE, (70, 50), RAGGED]


@pytest.mark.parametrize("mode", ["bf16", "f32"])
@pytest.mark.parametrize("arch", ["unet", "res_unet"])
def test_call_sequences_across_plan_thresholds(gpu, oracle_mod, arch, mode):
    """One engine driven through a seeded random sequence of host / device / batch predicts and weight changes over pages on
    both sides of the size thresholds -- the bf16 engine's persistent stride-2 walk (res_unet) and grids, the float32 engine's
    cout tiles per workgroup (NT 1 on the small pages, 4 on the large ones) -- returns exactly what a fresh engine returns for
    each page (tests/test_predict_gpu.py::test_call_sequences_do_not_leak_state covers fcn_skip)."""
    import torch
    for s in SEQ_SHAPES:
        big = s[0] >= 1024
        _assert_persistent(*s, want=big)
        assert (_exact_wide(arch, *s)[1] > 1) == big, (arch, s, _exact_wide(arch, *s))
    m = gpu.MODE_BF16 if mode == "bf16" else gpu.MODE_F32_EXACT
    rng = np.random.default_rng(22)
    pages = {s: rng.integers(0, 256, s, dtype=np.uint8) for s in SEQ_SHAPES}
    weights = [oracle_mod.init_weights(arch, 3, seed=sd, gain=1.5, bias_scale=0.05) for sd in (1, 2)]
    want = {}
    for wi, Wt in enumerate(weights):
        for s in SEQ_SHAPES:
            f = gpu.Engine(arch, 3, mode=m)
            f.set_weights(Wt)
            want[(wi, s)] = f.predict(pages[s], want_probs=False)
            f.close()
    # twelve operations: every kind at least twice, each predict kind on both sides of the thresholds
    ops = [int(o) for o in rng.permutation([0, 0, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4])]
    seq = [(op, SEQ_SHAPES[int(rng.integers(0, len(SEQ_SHAPES)))]) for op in ops]
    for op in (1, 2, 3):
        assert {s[0] >= 1024 for o, s in seq if o == op} == {True, False}, seq
    eng = gpu.Engine(arch, 3, mode=m)
    wi = 0
    eng.set_weights(weights[wi])
    st = torch.cuda.current_stream().cuda_stream
    for step, (op, s) in enumerate(seq):
        if op == 0:                                              # change the weights
            wi = 1 - wi
            eng.set_weights(weights[wi])
        elif op == 1:                                            # host entry with logits
            z, _, l = eng.predict(pages[s], want_probs=False)
            assert np.array_equal(z, want[(wi, s)][0]) and np.array_equal(l, want[(wi, s)][2]), (step, s)
        elif op == 2:                                            # host entry, labels only
            l = eng.predict(pages[s], want_logits=False, want_probs=False)[2]
            assert np.array_equal(l, want[(wi, s)][2]), (step, s)
        elif op == 3:                                            # device entry on torch's stream, uint8 labels
            d_img = torch.from_numpy(pages[s]).cuda()
            d_u8 = torch.empty(s, dtype=torch.uint8, device="cuda")
            eng.predict_device(d_img.data_ptr(), s[0], s[1], d_labels_u8=d_u8.data_ptr(), stream=st)
            torch.cuda.synchronize()
            assert np.array_equal(d_u8.cpu().numpy(), want[(wi, s)][2]), (step, s)
        else:                                                    # batch of three ragged pages, one of each side at least
            ss = [SEQ_SHAPES[int(i)] for i in rng.permutation(len(SEQ_SHAPES))[:3]]
            out = eng.predict_batch([pages[q] for q in ss])
            for q, o in zip(ss, out):
                assert np.array_equal(o, want[(wi, q)][2]), (step, q)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------
# E. page units over the threshold


@pytest.mark.parametrize("arch", ["res_unet", "unet"])
def test_page_units_over_the_persistence_threshold(gpu, arch):
    """Two 1024x768 pages as one unit (pseg_predict_pages_device: every tensor holds a slot per page) against the pages one by
    one: the same products in the same order, so the label maps must be the same, uint8 and int64.  In the unit the quarter-
    resolution and deeper convs take both slots in one launch (blockIdx.z = slot, persistence off); the full- and half-
    resolution layers run slot by slot, so res_unet's first stride-2 layers take the persistent walk here as on a single page
    (a kernel trace of this test shows conv_mfma_kernel<2, 4, 3, 2, 4, 0, 64 | 68, 4> on 512 workgroups for each slot)."""
    import torch
    from pseg_amd import synth
    H, W = LARGE
    _assert_persistent(H, W)
    n = 2
    pages = np.stack([synth.synth_page(50 + i, H, W, 3)[0] for i in range(n)])
    eng = gpu.Engine(arch, 3, mode=gpu.MODE_BF16)
    eng.set_weights(synth.glorot_weights(eng.weight_specs(), seed=42, gain=1.5, bias_scale=0.05))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    want = []
    for i in range(n):
        d = torch.from_numpy(pages[i]).to(dev)
        lab = torch.empty((H, W), dtype=torch.uint8, device=dev)
        eng.predict_device(d.data_ptr(), H, W, d_labels_u8=lab.data_ptr(), stream=st)
        torch.cuda.synchronize()
        want.append(lab.cpu().numpy())
    assert not np.array_equal(want[0], want[1])
    d = torch.from_numpy(pages).to(dev)
    out8 = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    out64 = torch.zeros((n, H, W), dtype=torch.int64, device=dev)
    eng.predict_pages_device(d.data_ptr(), n, H, W, d_labels=out64.data_ptr(), d_labels_u8=out8.data_ptr(), stream=st)
    eng.status(st)
    for i in range(n):
        assert np.array_equal(out8[i].cpu().numpy(), want[i]), i
        assert np.array_equal(out64[i].cpu().numpy(), want[i]), i
    eng.close()
