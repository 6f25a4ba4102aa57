"""Training masks as label maps on the device: pseg_label_masks against the host entry and the restatement of
tests/labelmasks_cases.py over the same grid, integer array_equal throughout; lists of two groups in any order, each mask alone,
after the workspace was released, with and without counts; the byte rule of the group cut; every refusal."""
import numpy as np
import pytest

import labelmasks_cases as C

pytestmark = pytest.mark.gpu


def test_device_list_equals_host_entry_and_restatement(gpu):
    cases, want = C.grid()
    for n, ks in C.by_table(cases).items():
        sub = [cases[k] for k in ks]
        got = C.run(sub, n)
        C.assert_equal(sub, got, [want[k] for k in ks])
        C.assert_equal(sub, got, C.run(sub, n, host=True))
        plain = gpu.label_masks([c[1] for c in sub], [c[2] for c in sub], *C.table(n))
        assert all(a.dtype == np.uint8 and np.array_equal(a, b[0]) for a, b in zip(plain, got))


def test_seventy_masks_in_two_groups(gpu):
    cases = C.mixed_list()
    assert len(cases) == 70 and gpu.label_mask_groups([c[1] for c in cases]) == [0] * 64 + [1] * 6
    assert {c[1].ndim for c in cases} == {2, 3} and len({c[1].shape[:2] for c in cases}) > 40
    want = C.run(cases, 8, host=True)
    C.assert_equal(cases[:10], want[:10], [C.restate(c[1], c[2], *C.table(8)) for c in cases[:10]])
    first = C.run(cases, 8)
    C.assert_equal(cases, first, want)
    C.assert_equal(cases, C.run(cases, 8), want)                              # twice: the workspace and its counters are reused
    order = np.random.default_rng(9).permutation(len(cases))
    C.assert_equal([cases[k] for k in order], C.run([cases[k] for k in order], 8), [want[k] for k in order])
    for c, w in zip(cases, want):                                              # each alone
        C.assert_equal([c], C.run([c], 8), [w])
    assert gpu.lib().pseg_release_workspace(0) == 0
    C.assert_equal(cases, C.run(cases, 8), want)
    plain = gpu.label_masks([c[1] for c in cases], [c[2] for c in cases], *C.table(8))      # counts off: the other instance
    assert all(np.array_equal(a, w[0]) for a, w in zip(plain, want))
    C.assert_equal(cases, C.run(cases, 8), want)


def test_group_cut_by_bytes(gpu):
    """Three 4096x2048 RGB masks, 24 MiB each: two make a group, the third a second one."""
    rng = np.random.default_rng(4)
    colors, ids = C.table(8)
    small = rng.integers(0, 8, (3, 64, 32))
    masks = []
    for k in range(3):
        m = np.repeat(np.repeat(colors[small[k]], 64, axis=0), 64, axis=1)     # 64x64 blocks of one colour each
        m[k::97, (5 * k)::89] = (251, k, 1)                                     # a lattice of unknown pixels
        masks.append(m)
    assert masks[0].shape == (4096, 2048, 3) and gpu.label_mask_groups(masks) == [0, 0, 1]
    shapes = [(64, 32)] * 3
    got = gpu.label_masks(masks, shapes, colors, ids, counts=True)
    want = gpu.label_masks(masks, shapes, colors, ids, counts=True, host=True)
    for (lab, cnt), (hlab, hcnt) in zip(got, want):
        assert np.array_equal(lab, hlab) and np.array_equal(cnt, hcnt) and cnt[:256].sum() == 64 * 32
    rlab, rcnt = C.restate(masks[2], (64, 32), colors, ids)                    # the mask of the second group, by the reference
    assert np.array_equal(got[2][0], rlab) and np.array_equal(got[2][1], rcnt)
    assert len({g[0].tobytes() for g in got}) == 3


def test_refusals_leave_the_outputs_untouched(gpu):
    assert C.refusals(gpu.lib(), False)
    with pytest.raises(gpu.PsegError, match="device 99"):
        gpu.label_masks([np.zeros((3, 3), np.uint8)], [(2, 2)], [], [], device=99)
