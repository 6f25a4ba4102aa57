"""The C-ABI library loads without a GPU, exports every symbol include/pseg.h declares, and fails
loudly (no CPU fallback) when no HIP device is visible.  No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "pseg.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(pseg_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    import pseg_amd
    L = pseg_amd.lib()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for sym in declared:
        assert hasattr(L, sym), "libpseg.so does not export %s" % sym
    assert sorted(pseg_amd.EXPORTED_SYMBOLS) == declared
    assert L.pseg_abi_version() == 1


def test_rccl_entry_points_are_pinned_against_the_rccl_header():
    """pseg_dist.hip binds RCCL by dlopen and restates its ABI by hand (128-byte id, ncclFloat32 = 7, ncclSum = 0, five prototypes);
    where <rccl/rccl.h> exists at build time -- the ROCm image -- static_asserts compare every one of them with the header, and the
    library says whether they ran.  No GPU and no second rank needed: a mismatch is a build failure."""
    import pseg_amd
    L = pseg_amd.lib()
    pinned = L.pseg_rccl_abi_pinned()
    assert pinned == (1 if os.path.exists("/opt/rocm/include/rccl/rccl.h") else 0)


def test_release_library_reads_at_most_15_documented_environment_knobs():
    """The release library takes its environment knobs from ONE list (PSEG_ENV_KNOBS, pseg_env_knobs()): at most 15 names, every
    one documented in README.md, and no other getenv in the sources -- kernel / fusion plan switches reach an engine only through
    pseg_create_plan's string (the test harness builds it from os.environ: pseg_amd.engine.PLAN_FROM_ENV)."""
    import glob
    import re
    import pseg_amd
    names = pseg_amd.lib().pseg_env_knobs().decode().split("\n")
    assert 1 <= len(names) <= 15 and len(set(names)) == len(names), names
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert all(("`%s`" % n) in readme for n in names), [n for n in names if ("`%s`" % n) not in readme]
    csrc = os.path.join(ROOT, "page-segmentation_amd", "csrc")
    src = {fn: open(fn).read() for fn in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.h"))}
    # getenv: the snapshot (over the list) and the two macros of the diagnostic build, nothing else
    calls = [(os.path.basename(fn), ln.strip()) for fn, t in src.items() for ln in t.splitlines() if re.search(r"\bgetenv\(", ln)]
    assert len(calls) == 3 and sorted(c[0] for c in calls) == ["pseg_common.h", "pseg_common.h", "pseg_engine.hip"], calls
    # every name the sources look up is a listed environment knob or a plan switch; the total stays reviewable
    used = sorted({m for t in src.values() for m in re.findall(r'PSEG_KNOB\("(PSEG_[A-Z0-9_]+)"\)', t)})
    assert set(names) <= set(used), sorted(set(names) - set(used))          # no listed knob is dead
    assert len(used) <= 49, (len(used), used)


def test_plan_switches_do_not_come_from_the_environment(monkeypatch):
    """A plan switch in the process environment does not reach the snapshot an engine would take; a listed knob does (checked on
    the snapshot text the library reports -- no GPU needed)."""
    import pseg_amd
    from pseg_amd import engine as E
    assert E.PLAN_FROM_ENV                                                  # (tests/conftest.py: the harness translates for the tests)
    listed = pseg_amd.lib().pseg_env_knobs().decode().split("\n")
    assert "PSEG_NO_SP" in listed and "PSEG_NO_DQ" not in listed and "PSEG_NO_PAIRC2" not in listed


def test_oracle_library_is_separate_from_the_product():
    """Nothing of the oracle is linked into or imported by the product package."""
    import subprocess
    import pseg_amd
    out = subprocess.run(["nm", "-D", pseg_amd.lib_path()], capture_output=True, text=True).stdout
    assert "orc_" not in out
    pkg = os.path.join(ROOT, "page-segmentation_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dp, fn)).read()
                assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, fn


def test_fails_loudly_without_a_gpu():
    import pseg_amd
    if pseg_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(pseg_amd.PsegError) as ei:
        pseg_amd.Engine("fcn_skip", 3)
    assert "no CPU fallback" in str(ei.value) or "HIP" in str(ei.value)
    import numpy as np
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.cc_vote(np.zeros((4, 4), np.int64), np.ones((4, 4), np.uint8), 3)
    with pytest.raises(pseg_amd.PsegError):
        pseg_amd.masks(np.zeros((4, 4), np.int64), np.ones((4, 4), np.uint8), np.zeros((3, 3), np.uint8))
    L = pseg_amd.lib()
    h = ctypes.c_void_p()
    assert L.pseg_create(0, 3, 1, 0, 1, ctypes.byref(h)) != 0
    assert L.pseg_create(99, 3, 1, 0, 1, ctypes.byref(h)) != 0
    assert len(L.pseg_last_error()) > 0


def test_library_links_no_vendor_gemm():
    """Every GEMM on the hot path is a hand-written MFMA kernel: libpseg.so must not pull in hipBLASLt / rocBLAS / MIOpen."""
    import subprocess
    import pseg_amd
    out = subprocess.run(["ldd", pseg_amd.lib_path()], capture_output=True, text=True).stdout.lower()
    assert not any(k in out for k in ("hipblas", "rocblas", "miopen")), out


def test_release_library_has_no_wrong_result_switches():
    """Timing ablations that produce wrong results (PSEG_DBG, PSEG_XM_DBG, PSEG_PP_NODMA, PSEG_PP_NOEPI, the in-kernel
    trace stamps) are compiled into the diagnostic build only (PSEG_DIAG_KNOB is a constant nullptr in the release
    library): the release .so does not even contain their names, so no environment can switch them on."""
    import pseg_amd
    blob = open(pseg_amd.lib_path(), "rb").read()
    for name in (b"PSEG_PP_NODMA", b"PSEG_PP_NOEPI", b"PSEG_XM_DBG", b"PSEG_DBG\0", b"PSEG_WS_TRACE", b"PSEG_TRACE\0"):
        assert name not in blob, name
    src = open(os.path.join(ROOT, "page-segmentation_amd", "csrc", "pseg_common.h")).read()
    assert "#define PSEG_DIAG_KNOB(name) ((const char*)nullptr)" in src


def test_reciprocal_pixel_index_is_exact_for_every_channel_count():
    """conv1x1_exact_kernel splits a flat element index e < 256*C into (pixel, channel) with a reciprocal multiply,
    floor(e * (2^32 // C + 1) / 2^32); exact for every per-source channel count the launch gate admits (<= 127).  (A
    20-bit reciprocal was wrong for C in 73..127 -- ADVICE round 2.)  conv_exact_mfma_kernel's staging keeps the 20-bit
    form under its own gate: C < 64 and e < 67 * 64."""
    import numpy as np
    for C in range(1, 128):
        e = np.arange(256 * C, dtype=np.uint64)
        inv = np.uint64((1 << 32) // C + 1)
        assert np.array_equal((e * inv) >> np.uint64(32), e // np.uint64(C)), C
    for C in range(1, 64):
        e = np.arange(67 * 64, dtype=np.uint64)
        inv = np.uint64((1 << 20) // C + 1)
        assert np.array_equal((e * inv) >> np.uint64(20), e // np.uint64(C)), C
