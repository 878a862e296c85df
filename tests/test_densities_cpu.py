"""CPU checks of the several-densities entries (sctl_amd_eval_densities_*): argument errors before any device work, the planner's
invariants, the device assembly of the multi-density kernels (no scratch, at least two waves per SIMD) and the C++ host surface."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

OK, UNKNOWN, BAD, NODEV, BADCTX = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
GB2 = 2 << 30


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_argument_errors_before_any_device_work():
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = _p(z)
    for fn, last in ((L.sctl_amd_eval_densities_host, 0), (L.sctl_amd_eval_densities_device, None)):
        assert fn(0, 0, -1, 1, 1, p, p, None, p, p, -1, None, 0, last) == BAD                    # nd < 0
        assert b"densities" in L.sctl_amd_last_error()
        assert fn(0, 0, 2, 1, 1, p, p, None, None, p, -1, None, 0, last) == BAD                  # null v_src
        assert fn(0, 0, 2, 1, 1, p, p, None, p, None, -1, None, 0, last) == BAD                  # null v_trg
        assert fn(99, 0, 2, 1, 1, p, p, None, p, p, -1, None, 0, last) == UNKNOWN                # unknown kernel
        assert fn(0, 7, 2, 1, 1, p, p, None, p, p, -1, None, 0, last) == BAD                     # bad precision tag
        assert fn(0, 0, 2, -1, 1, p, p, None, p, p, -1, None, 0, last) == BAD                    # negative size
        assert fn(1, 0, 2, 1, 1, p, p, None, p, p, -1, None, 0, last) == BAD                     # Laplace3D-DxU without normals
        assert b"normals" in L.sctl_amd_last_error()
        assert fn(9, 0, 2, 1, 1, p, p, None, p, p, -1, None, 0, last) == BADCTX                  # Helmholtz without its wavenumber
        assert fn(9, 0, 2, 1, 1, p, p, None, p, p, -1, p, 8, last) == BADCTX                     # ... or with a blob of the wrong size
        if sctl_amd.device_count() == 0:
            assert fn(0, 0, 2, 1, 1, p, p, None, p, p, -1, None, 0, last) == NODEV               # good arguments: no CPU fallback
            assert fn(0, 0, 1, 1, 1, p, p, None, p, p, -1, None, 0, last) == NODEV               # nd == 1: the single-density entry's answer
    assert L.sctl_amd_op_eval_densities(None, 2, p, p, 0, -1, None, 0) == BAD
    i, i64 = ctypes.c_int(), ctypes.c_int64()
    args = [ctypes.byref(i)] * 4 + [ctypes.byref(i64)] * 2
    assert L.sctl_amd_eval_densities_plan(0, 0, -1, 10, 10, -1, *args) == BAD
    assert L.sctl_amd_eval_densities_plan(99, 0, 2, 10, 10, -1, *args) == UNKNOWN
    assert L.sctl_amd_eval_densities_plan(0, 3, 2, 10, 10, -1, *args) == BAD
    assert L.sctl_amd_eval_densities_plan(0, 0, 2, -10, 10, -1, *args) == BAD


def test_python_wrappers_check_shapes():
    x = np.zeros(30)
    with pytest.raises(sctl_amd.api.SctlAmdError):
        sctl_amd.eval_densities_host("Laplace3D-FxU", x, x, None, np.zeros(10))              # V_src must be (nd, Ns*SrcDim)
    with pytest.raises(sctl_amd.api.SctlAmdError):
        sctl_amd.eval_densities_host("Stokes3D-FxU", x, x, None, np.zeros((2, 10)))


def _l2_splits(info, real, M, Nt, Ns):
    """the L2 rule of the single-density planner with M densities in a split's source bytes"""
    if Nt * Ns < 2 ** 34:
        return 1
    rs = 8 if real == 0 else 4
    s = -(-Ns * (3 + info["nd"] + M * info["k0"]) * rs // (2 << 20))
    return min(64, -(-s // 8) * 8, -(-Ns // 256))


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_planner_invariants(name):
    info = sctl_amd.kernel_info(name)
    for real in (0, 1):
        m_max = sctl_amd.plan_densities(name, real, 64, 1 << 14, 1 << 14)["densities_per_pass"]
        assert m_max in (4, 8)
        for nd in (1, 2, 3, 8, 11, 33):
            for N in (300, 1 << 14, 1 << 18, 1 << 20, 1 << 23):
                pl = sctl_amd.plan_densities(name, real, nd, N, N)
                if nd == 1:
                    single = sctl_amd.plan(name, real, N, N)
                    assert pl == dict(densities_per_pass=1, passes=1, **{k: single[k] for k in ("trg_per_lane", "src_splits", "workgroups", "workspace_bytes")})
                    continue
                M = pl["densities_per_pass"]
                assert M in (2, 4, 8) and M <= m_max
                assert pl["passes"] == math.ceil(nd / m_max) and M * pl["passes"] >= nd, (name, real, nd, N, pl)
                assert M == (m_max if nd >= m_max else min(m for m in (2, 4, 8) if m >= nd))
                assert 0 <= pl["workspace_bytes"] <= GB2, (name, real, nd, N, pl)
                s = pl["src_splits"]
                assert s >= 1 and (s < 8 or s % 8 == 0), (name, real, nd, N, pl)
                assert s >= _l2_splits(info, real, M, N, N), (name, real, nd, N, pl)
                assert pl["trg_per_lane"] in (1, 2)
                assert pl["workgroups"] >= -(-N // (256 * pl["trg_per_lane"])) * s


def test_planner_cuts_the_targets_when_the_partial_sums_would_pass_2gb():
    """Stokes3D-FxT fp32, 8 densities at 2^20 x 2^20: the L2 rule asks for 32 splits of four densities' records, whose partial sums over all
    targets would be 4.5 GB; the plan keeps the 32 splits and cuts the targets instead (the workgroups still cover every target once per split)."""
    info = sctl_amd.kernel_info("Stokes3D-FxT")
    N = 1 << 20
    pl = sctl_amd.plan_densities("Stokes3D-FxT", 1, 8, N, N)
    M, s = pl["densities_per_pass"], pl["src_splits"]
    assert pl["passes"] * M >= 8
    assert s >= _l2_splits(info, 1, M, N, N) >= 32, pl
    assert M * s * N * info["k1"] * 4 > GB2, pl                 # the whole target set would not fit ...
    assert 0 < pl["workspace_bytes"] <= GB2, pl                   # ... so one launch holds a part of it
    assert pl["workgroups"] == -(-N // (256 * pl["trg_per_lane"])) * s


# (kernel, real, nd, Nt, Ns, forward plan, transposed plan) with a plan as (rows per pass, passes, owners per lane, splits, workgroups, workspace bytes): what the
# two separate planners (make_plan_multi, make_plan_multi_t) returned before they became one (make_plan_rows), SCTL_AMD_TRANSPOSE_WORKSPACE unset, 256 CUs.
# Among them Stokes3D-FSxU fp64 with 8 rows at 2^22 x 2^22 in both directions, Stokes3D-FxT (widest form 4, owner cuts) and kernels with a source normal at
# sizes where the forward L2 rule counts it (Laplace3D-DxU fp64, 4 rows, 2^20 x 2^20: 40 splits forward, 32 transposed).
PLANS_BEFORE_THE_MERGE = (
    ("Stokes3D-FSxU", 0, 8, 1 << 22, 1 << 22, (4, 2, 1, 64, 1048576, 1074266112), (8, 1, 1, 64, 1048576, 2147483648)),
    ("Stokes3D-FxT", 0, 8, 1 << 20, 1 << 20, (4, 2, 1, 64, 262144, 1075838976), (4, 2, 1, 64, 262144, 1074266112)),
    ("Stokes3D-FxT", 1, 8, 1 << 20, 1 << 20, (4, 2, 1, 32, 131072, 1611399168), (4, 2, 1, 64, 262144, 1610612736)),
    ("Laplace3D-DxU", 0, 4, 1 << 20, 1 << 20, (4, 1, 2, 40, 81920, 1342177280), (4, 1, 2, 32, 65536, 1073741824)),
    ("Stokes3D-DxU", 1, 8, 1 << 22, 1 << 22, (8, 1, 1, 64, 1048576, 1074266112), (8, 1, 1, 64, 1048576, 1074266112)),
    ("Helmholtz3D-FxU", 0, 33, 1 << 22, 1 << 22, (8, 5, 1, 64, 1048576, 2147483648), (8, 5, 1, 64, 1048576, 2147483648)),
    ("Laplace3D-FxU", 0, 2, 1, 1, (2, 1, 2, 1, 1, 0), (2, 1, 2, 1, 1, 0)),
    ("Laplace3D-FxU", 1, 5, 1 << 12, 64, (8, 1, 2, 1, 8, 0), (8, 1, 2, 16, 16, 32768)),
    ("Laplace3D-FxU", 0, 33, 1 << 20, 1 << 20, (8, 5, 2, 48, 98304, 1610612736), (8, 5, 2, 48, 98304, 1610612736)),
    ("Laplace3D-FxU", 1, 4, 1 << 14, 1 << 23, (4, 1, 2, 64, 2048, 16777216), (4, 1, 2, 8, 131072, 1073741824)),
    ("Laplace3D-FxU", 0, 11, 1000, 513, (8, 2, 2, 3, 6, 192000), (8, 2, 2, 4, 8, 131328)),
    ("Laplace3D-FxU", 1, 3, 1 << 18, 1 << 18, (4, 1, 2, 8, 4096, 33554432), (4, 1, 2, 8, 4096, 33554432)),
    ("Laplace3D-DxU", 1, 4, 1 << 22, 1 << 22, (4, 1, 2, 64, 524288, 2147483648), (4, 1, 2, 56, 458752, 1879048192)),
    ("Laplace3D-DxU", 0, 11, 1, 1, (8, 2, 2, 1, 1, 0), (8, 2, 2, 1, 1, 0)),
    ("Laplace3D-DxU", 1, 3, 1 << 12, 64, (4, 1, 2, 1, 8, 0), (4, 1, 2, 16, 16, 16384)),
    ("Laplace3D-DxU", 0, 8, 1 << 20, 1 << 20, (8, 1, 2, 56, 114688, 1879048192), (8, 1, 2, 48, 98304, 1610612736)),
    ("Laplace3D-DxU", 1, 2, 1 << 14, 1 << 23, (2, 1, 2, 64, 2048, 8388608), (2, 1, 2, 8, 131072, 536870912)),
    ("Laplace3D-DxU", 0, 5, 1000, 513, (8, 1, 2, 3, 6, 192000), (8, 1, 2, 4, 8, 131328)),
    ("Laplace3D-FxdU", 0, 8, 1 << 14, 1 << 14, (8, 1, 1, 16, 1024, 50331648), (8, 1, 1, 16, 1024, 16777216)),
    ("Laplace3D-FxdU", 1, 2, 1 << 22, 1 << 22, (2, 1, 2, 40, 327680, 2013265920), (2, 1, 2, 64, 524288, 2147483648)),
    ("Laplace3D-FxdU", 0, 5, 1, 1, (8, 1, 1, 1, 1, 0), (8, 1, 1, 1, 1, 0)),
    ("Laplace3D-FxdU", 1, 33, 1 << 12, 64, (8, 5, 1, 1, 16, 0), (8, 5, 1, 16, 16, 32768)),
    ("Laplace3D-FxdU", 0, 4, 1 << 20, 1 << 20, (4, 1, 1, 32, 131072, 1610612736), (4, 1, 1, 64, 262144, 2147483648)),
    ("Laplace3D-FxdU", 1, 11, 1 << 14, 1 << 23, (8, 2, 1, 64, 4096, 100663296), (8, 2, 1, 8, 262144, 2147483648)),
    ("Stokes3D-FxU", 1, 33, 300, 300, (8, 5, 1, 2, 4, 57600), (8, 5, 1, 2, 4, 57600)),
    ("Stokes3D-FxU", 0, 4, 1 << 14, 1 << 14, (4, 1, 1, 16, 1024, 25165824), (4, 1, 1, 16, 1024, 25165824)),
    ("Stokes3D-FxU", 1, 11, 1 << 22, 1 << 22, (8, 2, 1, 64, 1048576, 1074266112), (8, 2, 1, 64, 1048576, 1074266112)),
    ("Stokes3D-FxU", 0, 3, 1, 1, (4, 1, 1, 1, 1, 0), (4, 1, 1, 1, 1, 0)),
    ("Stokes3D-FxU", 1, 8, 1 << 12, 64, (8, 1, 1, 1, 16, 0), (8, 1, 1, 16, 16, 98304)),
    ("Stokes3D-FxU", 0, 2, 1 << 20, 1 << 20, (2, 1, 2, 40, 81920, 2013265920), (2, 1, 2, 40, 81920, 2013265920)),
    ("Stokes3D-DxU", 0, 3, 1 << 23, 1 << 14, (4, 1, 1, 8, 262144, 1073872896), (4, 1, 1, 64, 4096, 100663296)),
    ("Stokes3D-DxU", 1, 8, 300, 300, (8, 1, 1, 2, 4, 57600), (8, 1, 1, 2, 4, 57600)),
    ("Stokes3D-DxU", 0, 2, 1 << 14, 1 << 14, (2, 1, 2, 32, 1024, 25165824), (2, 1, 2, 32, 1024, 25165824)),
    ("Stokes3D-DxU", 1, 5, 1 << 22, 1 << 22, (8, 1, 1, 64, 1048576, 1074266112), (8, 1, 1, 64, 1048576, 1074266112)),
    ("Stokes3D-DxU", 0, 33, 1, 1, (8, 5, 1, 1, 1, 0), (8, 5, 1, 1, 1, 0)),
    ("Stokes3D-DxU", 1, 4, 1 << 12, 64, (4, 1, 1, 1, 16, 0), (4, 1, 1, 16, 16, 49152)),
    ("Stokes3D-FxT", 1, 5, 1 << 18, 1 << 18, (4, 2, 1, 8, 8192, 301989888), (4, 2, 1, 24, 24576, 301989888)),
    ("Stokes3D-FxT", 0, 33, 1 << 23, 1 << 14, (4, 9, 1, 8, 262144, 1932853248), (4, 9, 1, 64, 4096, 100663296)),
    ("Stokes3D-FxT", 1, 4, 300, 300, (4, 1, 1, 2, 4, 86400), (4, 1, 1, 2, 4, 28800)),
    ("Stokes3D-FxT", 0, 11, 1 << 14, 1 << 14, (4, 3, 1, 16, 1024, 75497472), (4, 3, 1, 16, 1024, 25165824)),
    ("Stokes3D-FxT", 1, 3, 1 << 22, 1 << 22, (4, 1, 1, 64, 1048576, 1075838976), (4, 1, 1, 64, 1048576, 1074266112)),
    ("Stokes3D-FxT", 0, 8, 1, 1, (4, 2, 1, 1, 1, 0), (4, 2, 1, 1, 1, 0)),
    ("Stokes3D-FSxU", 0, 11, 1000, 513, (4, 3, 1, 3, 12, 288000), (8, 2, 1, 4, 12, 525312)),
    ("Stokes3D-FSxU", 1, 3, 1 << 18, 1 << 18, (4, 1, 1, 16, 16384, 201326592), (4, 1, 1, 8, 8192, 134217728)),
    ("Stokes3D-FSxU", 0, 8, 1 << 23, 1 << 14, (4, 2, 1, 8, 262144, 1073872896), (8, 1, 1, 64, 4096, 268435456)),
    ("Stokes3D-FSxU", 1, 2, 300, 300, (2, 1, 2, 2, 2, 14400), (2, 1, 2, 2, 2, 19200)),
    ("Stokes3D-FSxU", 0, 5, 1 << 14, 1 << 14, (4, 2, 1, 16, 1024, 25165824), (8, 1, 1, 16, 1024, 67108864)),
    ("Stokes3D-FSxU", 1, 33, 1 << 22, 1 << 22, (4, 9, 1, 64, 1048576, 1074266112), (8, 5, 1, 64, 1048576, 2147483648)),
    ("Stokes3D-FxUP", 1, 2, 1 << 14, 1 << 23, (2, 1, 2, 64, 2048, 33554432), (2, 1, 2, 8, 131072, 1610612736)),
    ("Stokes3D-FxUP", 0, 5, 1000, 513, (4, 2, 1, 3, 12, 384000), (8, 1, 1, 4, 12, 393984)),
    ("Stokes3D-FxUP", 1, 33, 1 << 18, 1 << 18, (4, 9, 1, 8, 8192, 134217728), (8, 5, 1, 24, 24576, 603979776)),
    ("Stokes3D-FxUP", 0, 4, 1 << 23, 1 << 14, (4, 1, 1, 8, 262144, 2147483648), (4, 1, 1, 64, 4096, 100663296)),
    ("Stokes3D-FxUP", 1, 11, 300, 300, (4, 3, 1, 2, 4, 38400), (8, 2, 1, 2, 4, 57600)),
    ("Stokes3D-FxUP", 0, 3, 1 << 14, 1 << 14, (4, 1, 1, 16, 1024, 33554432), (4, 1, 1, 16, 1024, 25165824)),
    ("Laplace3D-FDxUdU", 0, 4, 1 << 20, 1 << 20, (4, 1, 1, 56, 229376, 1879048192), (4, 1, 1, 64, 262144, 2147483648)),
    ("Laplace3D-FDxUdU", 1, 11, 1 << 14, 1 << 23, (4, 3, 1, 64, 4096, 67108864), (8, 2, 1, 8, 262144, 2147483648)),
    ("Laplace3D-FDxUdU", 0, 3, 1000, 513, (4, 1, 1, 3, 12, 384000), (4, 1, 1, 4, 12, 131328)),
    ("Laplace3D-FDxUdU", 1, 8, 1 << 18, 1 << 18, (4, 2, 1, 8, 8192, 134217728), (8, 1, 1, 24, 24576, 402653184)),
    ("Laplace3D-FDxUdU", 0, 2, 1 << 23, 1 << 14, (2, 1, 2, 8, 131072, 2147483648), (2, 1, 2, 64, 2048, 33554432)),
    ("Laplace3D-FDxUdU", 1, 5, 300, 300, (4, 2, 1, 2, 4, 38400), (8, 1, 1, 2, 4, 38400)),
    ("Helmholtz3D-FxU", 1, 8, 1 << 12, 64, (8, 1, 1, 1, 16, 0), (8, 1, 1, 16, 16, 65536)),
    ("Helmholtz3D-FxU", 0, 2, 1 << 20, 1 << 20, (2, 1, 2, 32, 65536, 1073741824), (2, 1, 2, 32, 65536, 1073741824)),
    ("Helmholtz3D-FxU", 1, 5, 1 << 14, 1 << 23, (8, 1, 1, 64, 4096, 67108864), (8, 1, 1, 8, 262144, 2147483648)),
    ("Helmholtz3D-FxU", 0, 33, 1000, 513, (8, 5, 1, 3, 12, 384000), (8, 5, 1, 4, 12, 262656)),
    ("Helmholtz3D-FxU", 1, 4, 1 << 18, 1 << 18, (4, 1, 1, 8, 8192, 67108864), (4, 1, 1, 8, 8192, 67108864)),
    ("Helmholtz3D-FxU", 0, 11, 1 << 23, 1 << 14, (8, 2, 1, 8, 262144, 2147483648), (8, 2, 1, 64, 4096, 134217728)),
)


def test_one_planner_returns_the_plans_of_the_two_it_replaced(monkeypatch):
    monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE", raising=False)
    assert len(PLANS_BEFORE_THE_MERGE) >= 60
    for name, real, nd, Nt, Ns, fwd, trans in PLANS_BEFORE_THE_MERGE:
        f = sctl_amd.plan_densities(name, real, nd, Nt, Ns)
        t = sctl_amd.plan_transpose_densities(name, real, nd, Nt, Ns)
        assert tuple(f[k] for k in ("densities_per_pass", "passes", "trg_per_lane", "src_splits", "workgroups", "workspace_bytes")) == fwd, (name, real, nd, Nt, Ns, f)
        assert tuple(t[k] for k in ("vectors_per_pass", "passes", "src_per_lane", "splits", "workgroups", "workspace_bytes")) == trans, (name, real, nd, Nt, Ns, t)


def test_transpose_workspace_variable_leaves_the_forward_plan_alone(monkeypatch):
    """The forward bound is a fixed 2 GB: SCTL_AMD_TRANSPOSE_WORKSPACE, which lowers the transposed one, must not reach it through the shared planner."""
    N = 1 << 22
    monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE", raising=False)
    unset = sctl_amd.plan_densities("Stokes3D-FSxU", 0, 8, N, N)
    t_unset = sctl_amd.plan_transpose_densities("Stokes3D-FSxU", 0, 8, N, N)
    for v in ("1", str(1 << 20)):
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", v)
        assert sctl_amd.plan_densities("Stokes3D-FSxU", 0, 8, N, N) == unset, v
        assert sctl_amd.plan_transpose_densities("Stokes3D-FSxU", 0, 8, N, N) != t_unset, v   # (the variable is read: it does lower the transposed bound)


def _unit_asm(tmp_path, unit):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    extra = subprocess.run(["make", "-s", "-C", CSRC, "print-unit-flags", "UNIT=" + unit], capture_output=True, text=True, check=True).stdout.split()
    out = str(tmp_path / (unit + ".s"))
    return subprocess.Popen(["/opt/rocm/bin/hipcc"] + flags + extra + ["--offload-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE), out


def test_multi_density_kernels_have_no_scratch_and_two_waves_per_simd(tmp_path):
    """Every eval_multi_kernel instantiation of every multi_*.hip unit, compiled to gfx950 assembly with the Makefile's flags: ScratchSize 0 and at most 256
    allocated vector registers (two waves per SIMD), f64 modes 0/1/2 and f32 modes 0/1 for each form of 2, 4 (and 8) densities."""
    units = sorted(f[:-4] for f in os.listdir(CSRC) if f.startswith("multi_") and f.endswith(".hip"))
    assert len(units) == 10
    jobs = []
    for i in range(0, len(units), 5):                            # five compiles at a time
        batch = [_unit_asm(tmp_path, u) for u in units[i:i + 5]]
        for proc, out in batch:
            _, err = proc.communicate(timeout=900)
            assert proc.returncode == 0, err[-2000:]
        jobs += [out for _, out in batch]
    for out in jobs:
        txt = open(out).read()
        kernels = re.findall(r"\.amdhsa_kernel (\S*eval_multi_kernel\S*)\n(.*?)\.end_amdhsa_kernel", txt, re.S)
        assert len(kernels) in (10, 15), (out, len(kernels))    # forms of 2 and 4 (and 8) densities x 5 precision/accuracy modes
        for name, body in kernels:
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
            assert scratch == 0, (out, name)
            assert vgpr <= 256, (out, name, vgpr)


def test_host_header_eval_densities_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "densities_driver")
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "densities_driver.cpp"),
                    "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    if sctl_amd.device_count() > 0:
        pytest.skip("a GPU is present: the no-device abort cannot be observed")
    p = subprocess.run([exe, "50", "3", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert p.returncode != 0
    assert "sctl_amd_eval_densities_host" in p.stderr and "no CPU fallback" in p.stderr
