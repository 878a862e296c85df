"""Several weight vectors through the transposed kernel sum (sctl_amd_eval_transpose_densities_*): what can be checked without a GPU.  Argument errors before
any device work and the refusal of work without a device, the planner's invariants including the 2 GB cut of the owners, the Python wrappers' shape checks,
the device assembly of the ten tmulti_*.hip units (no scratch, at most 256 vector registers: two waves per SIMD) and the C++ host surface."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

OK, UNKNOWN, BAD, NODEV, BADCTX = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
GB2 = 2 << 30
SYMS = ("sctl_amd_eval_transpose_densities_device", "sctl_amd_eval_transpose_densities_host", "sctl_amd_eval_transpose_densities_plan")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    for f in ("eval_transpose_densities_host", "eval_transpose_densities_device", "plan_transpose_densities"):
        assert callable(getattr(sctl_amd, f))
    assert callable(sctl_amd.GenericKernel.EvalTransposeDensities)
    from sctl_amd import autograd
    assert callable(autograd.kernel_sum_densities)
    assert "EvalTransposeDensities" in open(os.path.join(ROOT, "include", "sctl_amd", "generic-kernel.hpp")).read()


def test_argument_errors_before_any_device_work():
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = _p(z)
    host = lambda k, real, nd, Nt, Ns, xt, xs, xn, w, g, ctx=None, cb=0: L.sctl_amd_eval_transpose_densities_host(k, real, nd, Nt, Ns, xt, xs, xn, w, g, 1, -1, ctx, cb, 0)
    dev = lambda k, real, nd, Nt, Ns, xt, xs, xn, w, g, ctx=None, cb=0: L.sctl_amd_eval_transpose_densities_device(k, real, nd, Nt, Ns, xt, xs, xn, w, g, -1, ctx, cb, None)
    for fn in (host, dev):
        assert fn(0, 0, -1, 1, 1, p, p, None, p, p) == BAD and b"weight vectors" in L.sctl_amd_last_error()      # nd < 0
        assert fn(0, 0, 2, 1, 1, p, p, None, None, p) == BAD and b"null weight or result" in L.sctl_amd_last_error()   # null W
        assert fn(0, 0, 2, 1, 1, p, p, None, p, None) == BAD and b"null weight or result" in L.sctl_amd_last_error()   # null G
        assert fn(99, 0, 2, 1, 1, p, p, None, p, p) == UNKNOWN                                                       # unknown kernel
        assert fn(0, 7, 2, 1, 1, p, p, None, p, p) == BAD and b"real must be" in L.sctl_amd_last_error()             # bad precision tag
        assert fn(0, 0, 2, -1, 1, p, p, None, p, p) == BAD and b"negative size" in L.sctl_amd_last_error()           # negative size
        assert fn(0, 0, 2, 1, 1, None, p, None, p, p) == BAD and b"null coordinate" in L.sctl_amd_last_error()
        assert fn(1, 0, 2, 1, 1, p, p, None, p, p) == BAD and b"needs source normals" in L.sctl_amd_last_error()     # Laplace3D-DxU without normals
        assert fn(9, 0, 2, 1, 1, p, p, None, p, p) == BADCTX and b"context blob of 16 bytes" in L.sctl_amd_last_error()   # Helmholtz without its wavenumber
        assert fn(9, 0, 2, 1, 1, p, p, None, p, p, p, 8) == BADCTX                                                   # ... or with a blob of the wrong size
        if sctl_amd.device_count() == 0:
            assert fn(0, 0, 2, 1, 1, p, p, None, p, p) == NODEV and b"no HIP device" in L.sctl_amd_last_error()      # good arguments: no CPU fallback
            assert fn(0, 0, 1, 1, 1, p, p, None, p, p) == NODEV                                                      # nd == 1: the single entry's answer
            assert fn(9, 0, 3, 1, 1, p, p, None, p, p, p, 16) == NODEV
    assert not z.any()
    i, i64 = ctypes.c_int(), ctypes.c_int64()
    args = [ctypes.byref(i)] * 4 + [ctypes.byref(i64)] * 2
    plan = L.sctl_amd_eval_transpose_densities_plan
    assert plan(0, 0, -1, 10, 10, -1, *args) == BAD and b"weight vectors" in L.sctl_amd_last_error()
    assert plan(99, 0, 2, 10, 10, -1, *args) == UNKNOWN
    assert plan(0, 3, 2, 10, 10, -1, *args) == BAD
    assert plan(0, 0, 2, -10, 10, -1, *args) == BAD
    assert plan(0, 0, 2, 10, 10, -1, *([None] * 6)) == OK                                                            # every output is optional


def test_python_wrappers_check_shapes():
    x = np.zeros(30)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="W_trg must have shape"):
        sctl_amd.eval_transpose_densities_host("Laplace3D-FxU", x, x, None, np.zeros(10))              # W_trg must be (nd, Nt*TrgDim)
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"W_trg must have shape \(nd, 40\)"):
        sctl_amd.eval_transpose_densities_host("Stokes3D-FxUP", x, x, None, np.zeros((2, 30)))         # TrgDim 4: 40 weights per row
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        sctl_amd.eval_transpose_densities_host("Helmholtz3D-FxU", x, x, None, np.zeros((2, 20)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="float64 array"):
        sctl_amd.eval_transpose_densities_host("Laplace3D-FxU", x, x, None, np.zeros((2, 10), dtype=np.float32))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="W_trg must have shape"):
        sctl_amd.GenericKernel("Laplace3D-FxU").EvalTransposeDensities(None, x, x, None, np.zeros((2, 11)))


def _l2_splits(info, real, M, Nt, Ns):
    """the L2 rule of the single transposed planner with M weight vectors in a split's streamed bytes"""
    if Nt * Ns < 2 ** 34:
        return 1
    rs = 8 if real == 0 else 4
    s = -(-Nt * (3 + M * info["k1"]) * rs // (2 << 20))
    return min(64, -(-s // 8) * 8, -(-Nt // 256))


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_planner_invariants(name):
    info = sctl_amd.kernel_info(name)
    for real in (0, 1):
        rs = 8 if real == 0 else 4
        m_max = sctl_amd.plan_transpose_densities(name, real, 64, 1 << 14, 1 << 14)["vectors_per_pass"]
        assert m_max == (4 if name == "Stokes3D-FxT" else 8)
        for nd in (1, 2, 3, 8, 11, 33):
            for N in (300, 1 << 14, 1 << 18, 1 << 20, 1 << 23):
                pl = sctl_amd.plan_transpose_densities(name, real, nd, N, N)
                if nd == 1:
                    single = sctl_amd.plan_transpose(name, real, N, N)
                    assert pl["vectors_per_pass"] == 1 and pl["passes"] == 1 and all(pl[k] == single[k] for k in single), (pl, single)
                    assert pl["workgroups"] >= -(-N // (256 * pl["src_per_lane"])) * pl["splits"]
                    continue
                M = pl["vectors_per_pass"]
                assert M in (2, 4, 8) and M <= m_max
                assert pl["passes"] == math.ceil(nd / m_max) and M * pl["passes"] >= nd, (name, real, nd, N, pl)
                assert M == (m_max if nd >= m_max else min(m for m in (2, 4, 8) if m >= nd))
                assert 0 <= pl["workspace_bytes"] <= GB2, (name, real, nd, N, pl)
                s = pl["splits"]
                assert s >= 1 and (s < 8 or s % 8 == 0), (name, real, nd, N, pl)
                assert s >= _l2_splits(info, real, M, N, N), (name, real, nd, N, pl)
                assert pl["src_per_lane"] in (1, 2)
                assert pl["workgroups"] >= -(-N // (256 * pl["src_per_lane"])) * s
                if s == 1 and pl["passes"] == 1:
                    assert pl["workspace_bytes"] == 0
                elif pl["passes"] == 1:                           # whole workgroups' owners, [M][splits][owners * K0] (the largest of any pass: one pass here)
                    per = M * s * info["k0"] * rs
                    assert pl["workspace_bytes"] % per == 0 and (pl["workspace_bytes"] // per == N or (pl["workspace_bytes"] // per) % (256 * pl["src_per_lane"]) == 0)
        for Nt, Ns in ((0, 0), (0, 10), (10, 0), (1, 1), (1 << 23, 1 << 14), (1 << 14, 1 << 23)):
            pl = sctl_amd.plan_transpose_densities(name, real, 5, Nt, Ns)
            assert pl["splits"] >= 1 and 0 <= pl["workspace_bytes"] <= GB2 and pl["passes"] == (2 if m_max == 4 else 1), (name, real, Nt, Ns, pl)


def test_planner_cuts_the_owners_when_the_partial_sums_would_pass_2gb():
    """Stokes3D-FSxU fp64, 8 weight vectors at 2^22 x 2^22: the L2 rule asks for 64 splits (the cap) of records of 27 reals, whose partial sums over
    all owners would be 64 GB; the plan keeps the 64 splits and cuts the owners into launches of 2^31 / (8 * 64 * 32 B) = 2^17 instead (the
    workgroups still cover every owner once per split)."""
    info = sctl_amd.kernel_info("Stokes3D-FSxU")
    N = 1 << 22
    pl = sctl_amd.plan_transpose_densities("Stokes3D-FSxU", 0, 8, N, N)
    M, s = pl["vectors_per_pass"], pl["splits"]
    assert M == 8 and s == 64 == _l2_splits(info, 0, M, N, N), pl
    assert M * s * N * info["k0"] * 8 > GB2                        # the whole source set would not fit ...
    assert pl["workspace_bytes"] == GB2 == M * s * (1 << 17) * info["k0"] * 8, pl    # ... so one launch holds 2^17 owners
    assert pl["workgroups"] == -(-N // (256 * pl["src_per_lane"])) * s


def test_workspace_bound_can_be_lowered_but_not_raised(monkeypatch):
    """SCTL_AMD_TRANSPOSE_WORKSPACE lowers the 2 GB bound as it does for the single transposed plan, never raises it; a launch always holds one whole
    workgroup's owners, and the splits never drop below the L2 rule's (fewer owners per launch ask for more, to fill the chip)"""
    P = lambda: sctl_amd.plan_transpose_densities("Stokes3D-FSxU", 0, 8, 1 << 22, 1 << 22)
    default = P()
    assert default["splits"] == 64 and default["workspace_bytes"] == GB2
    T = default["src_per_lane"]
    for value in ("1", str(1 << 20)):
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", value)
        pl = P()
        assert pl["splits"] >= 64 and pl["splits"] % 8 == 0 and pl["workspace_bytes"] == 8 * pl["splits"] * 256 * T * 4 * 8, (value, pl)
    for value in (str(1 << 40), "-5", "x", ""):
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", value)
        assert P() == default, value
    monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
    assert P() == default


def _unit_asm(tmp_path, unit):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    extra = subprocess.run(["make", "-s", "-C", CSRC, "print-unit-flags", "UNIT=" + unit], capture_output=True, text=True, check=True).stdout.split()
    assert "-fno-slp-vectorize" in extra, (unit, extra)
    out = str(tmp_path / (unit + ".s"))
    return subprocess.Popen(["/opt/rocm/bin/hipcc"] + flags + extra + ["--offload-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE), out


def test_multi_transpose_kernels_have_no_scratch_and_two_waves_per_simd(tmp_path):
    """Every eval_multi_transpose_kernel instantiation of every tmulti_*.hip unit, compiled to gfx950 assembly with the Makefile's flags: no private
    segment and at most 256 allocated vector registers (two waves per SIMD), f64 modes 0/1/2 and f32 modes 0/1 for each form of 2, 4 (and 8) weight
    vectors; and an LDS allocation of which two workgroups fit a CU."""
    units = sorted(f[:-4] for f in os.listdir(CSRC) if f.startswith("tmulti_") and f.endswith(".hip"))
    assert units == sorted("tmulti_" + n.replace("-", "_") for n in sctl_amd.KERNEL_NAMES)
    jobs = []
    for i in range(0, len(units), 5):                            # five compiles at a time
        batch = [_unit_asm(tmp_path, u) for u in units[i:i + 5]]
        for proc, out in batch:
            _, err = proc.communicate(timeout=900)
            assert proc.returncode == 0, err[-2000:]
        jobs += [out for _, out in batch]
    for out in jobs:
        txt = open(out).read()
        kernels = re.findall(r"\.amdhsa_kernel (\S*eval_multi_transpose_kernel\S*)\n(.*?)\.end_amdhsa_kernel", txt, re.S)
        assert len(kernels) == (10 if "Stokes3D_FxT" in out else 15), (out, len(kernels))    # forms of 2 and 4 (and 8) x 5 precision/accuracy modes
        for name, body in kernels:
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
            print("%s: %d VGPRs, %d B LDS" % (name, field("next_free_vgpr"), field("group_segment_fixed_size")))
            assert field("private_segment_fixed_size") == 0, (out, name)
            assert field("next_free_vgpr") <= 256, (out, name, field("next_free_vgpr"))
            assert (160 * 1024) // ((field("group_segment_fixed_size") + 1279) // 1280 * 1280) >= 2, (out, name)


def test_host_header_eval_transpose_densities_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "transpose_densities_driver")
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "transpose_densities_driver.cpp"),
                    "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    if sctl_amd.device_count() > 0:
        pytest.skip("a GPU is present: the no-device abort cannot be observed")
    p = subprocess.run([exe, "50", "40", "3", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert p.returncode != 0
    assert "sctl_amd_eval_transpose_densities_host" in p.stderr and "no CPU fallback" in p.stderr
