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
