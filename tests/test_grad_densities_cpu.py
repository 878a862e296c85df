"""Geometry gradients for several density / weight rows (sctl_amd_eval_grad_densities_*): what can be checked without a GPU.  The symbols, argument errors
before any device work and the refusal of work without a device, the Python wrappers' shape checks, the planner's arithmetic including the lowered
workspace bound in a fresh process, and the device assembly of the ten gmulti_*.hip units (no scratch, at most 256 vector registers, LDS for two
workgroups per CU, no atomic)."""
import ctypes
import math
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

OK, UNKNOWN, BAD, NODEV, BADCTX = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
GB2 = 2 << 30
SYMS = ("sctl_amd_eval_grad_densities_device", "sctl_amd_eval_grad_densities_host", "sctl_amd_eval_grad_densities_plan")
UNITS = ["gmulti_" + n.replace("-", "_") for n in sctl_amd.KERNEL_NAMES]
M_MAX = {n: (4 if n == "Stokes3D-FxT" else 8) for n in sctl_amd.KERNEL_NAMES}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    for f in ("eval_grad_densities_host", "eval_grad_densities_device", "plan_grad_densities"):
        assert callable(getattr(sctl_amd, f))
    assert callable(sctl_amd.GenericKernel.EvalGradDensities)
    from sctl_amd import autograd
    assert callable(autograd.kernel_sum_densities_geometry)
    assert "EvalGradDensities" in open(os.path.join(ROOT, "include", "sctl_amd", "generic-kernel.hpp")).read()


def test_argument_errors_before_any_device_work():
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = _p(z)
    host = lambda k, real, nd, Nt, Ns, xt, xs, xn, f, w, gn=None, ctx=None, cb=0: L.sctl_amd_eval_grad_densities_host(k, real, nd, Nt, Ns, xt, xs, xn, f, w, p, p, gn, 1, -1, ctx, cb, 0)
    dev = lambda k, real, nd, Nt, Ns, xt, xs, xn, f, w, gn=None, ctx=None, cb=0: L.sctl_amd_eval_grad_densities_device(k, real, nd, Nt, Ns, xt, xs, xn, f, w, p, p, gn, -1, ctx, cb, None)
    for fn in (host, dev):
        assert fn(0, 0, -1, 1, 1, p, p, None, p, p) == BAD and b"rows" in L.sctl_amd_last_error()                    # nd < 0
        assert fn(99, 0, -1, 1, 1, p, p, None, p, p) == BAD                                                          # ... before anything else
        assert fn(0, 0, 2, 1, 1, p, p, None, p, p, p) == BAD and b"g_nrm must be null" in L.sctl_amd_last_error()    # g_nrm for a kernel without a normal
        assert fn(1, 0, 2, 1, 1, p, p, None, p, p) == BAD and b"needs source normals" in L.sctl_amd_last_error()     # a missing normal
        assert fn(0, 0, 2, 1, 1, p, p, None, None, p) == BAD and b"null density or weight" in L.sctl_amd_last_error()
        assert fn(0, 0, 2, 1, 1, p, p, None, p, None) == BAD and b"null density or weight" in L.sctl_amd_last_error()
        assert fn(99, 0, 2, 1, 1, p, p, None, p, p) == UNKNOWN
        assert fn(0, 7, 2, 1, 1, p, p, None, p, p) == BAD and b"real must be" in L.sctl_amd_last_error()
        assert fn(0, 0, 2, -1, 1, p, p, None, p, p) == BAD and b"negative size" in L.sctl_amd_last_error()
        assert fn(0, 0, 2, 1, 1, None, p, None, p, p) == BAD and b"null coordinate" in L.sctl_amd_last_error()
        assert fn(9, 0, 2, 1, 1, p, p, None, p, p) == BADCTX                                                         # Helmholtz without its wavenumber
        if sctl_amd.device_count() == 0:
            assert fn(0, 0, 2, 1, 1, p, p, None, p, p) == NODEV and b"no HIP device" in L.sctl_amd_last_error()      # good arguments: no CPU fallback
            assert fn(0, 0, 1, 1, 1, p, p, None, p, p) == NODEV                                                      # nd == 1: the single entry's answer
            assert fn(4, 0, 3, 1, 1, p, p, p, p, p, p) == NODEV
            assert fn(9, 0, 3, 1, 1, p, p, None, p, p, None, p, 16) == NODEV
    assert not z.any()
    i, i64 = ctypes.c_int(), ctypes.c_int64()
    args = [ctypes.byref(i)] * 3 + [ctypes.byref(i64), ctypes.byref(i), ctypes.byref(i64)]
    plan = L.sctl_amd_eval_grad_densities_plan
    assert plan(0, 0, -1, 10, 10, -1, *args) == BAD and b"rows" in L.sctl_amd_last_error()
    assert plan(99, 0, 2, 10, 10, -1, *args) == UNKNOWN
    assert plan(0, 3, 2, 10, 10, -1, *args) == BAD
    assert plan(0, 0, 2, -10, 10, -1, *args) == BAD
    assert plan(0, 0, 2, 10, 10, -1, *([None] * 6)) == OK                                                            # every output is optional


def test_python_wrappers_check_shapes():
    x = np.zeros(30)
    E = sctl_amd.api.SctlAmdError
    with pytest.raises(E, match=r"V_src must have shape \(nd, 10\)"):
        sctl_amd.eval_grad_densities_host("Laplace3D-FxU", x, x, None, np.zeros(10), np.zeros((1, 10)))
    with pytest.raises(E, match=r"V_src must have shape \(nd, 40\)"):
        sctl_amd.eval_grad_densities_host("Stokes3D-FSxU", x, x, None, np.zeros((2, 30)), np.zeros((2, 30)))        # SrcDim 4
    with pytest.raises(E, match=r"W_trg must have shape \(nd, 40\)"):
        sctl_amd.eval_grad_densities_host("Stokes3D-FxUP", x, x, None, np.zeros((2, 30)), np.zeros((2, 30)))        # TrgDim 4
    with pytest.raises(E, match="same number of rows, not 2 and 3"):
        sctl_amd.eval_grad_densities_host("Laplace3D-FxU", x, x, None, np.zeros((2, 10)), np.zeros((3, 10)))
    with pytest.raises(E, match="want holds"):
        sctl_amd.eval_grad_densities_host("Laplace3D-FxU", x, x, None, np.zeros((2, 10)), np.zeros((2, 10)), want=("density",))
    with pytest.raises(E, match="n_src must be a contiguous float64 array of 30 values"):
        sctl_amd.eval_grad_densities_host("Laplace3D-DxU", x, x, None, np.zeros((2, 10)), np.zeros((2, 10)))        # a missing normal
    with pytest.raises(E, match="status -2.*g_nrm must be null"):
        sctl_amd.eval_grad_densities_host("Laplace3D-FxU", x, x, None, np.zeros((2, 10)), np.zeros((2, 10)), want=("nrm",))
    with pytest.raises(E, match="needs a context"):
        sctl_amd.eval_grad_densities_host("Helmholtz3D-FxU", x, x, None, np.zeros((2, 20)), np.zeros((2, 20)))
    with pytest.raises(E, match="W_trg must have shape"):
        sctl_amd.GenericKernel("Laplace3D-FxU").EvalGradDensities(x, x, None, np.zeros((2, 10)), np.zeros((2, 11)))


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_planner_arithmetic(name):
    """nd == 1 is plan_grad; passes = ceil(nd / rows_per_pass of a full pass); the form of a short call is the narrowest that holds it; splits come in
    eights from 8 on; the workspace is [splits][owners of a launch * 3 (6)] without a factor nd or M, the same for every nd that runs the same widest
    form, and at most 2 GB."""
    info = sctl_amd.kernel_info(name)
    m_max = M_MAX[name]
    for real in (0, 1):
        rs = 8 if real == 0 else 4
        assert sctl_amd.plan_grad_densities(name, real, 64, 1 << 14, 1 << 14)["rows_per_pass"] == m_max
        for N in (300, 1 << 14, 1 << 18, 1 << 20, 1 << 23):
            single = sctl_amd.plan_grad(name, real, N, N)
            pl = sctl_amd.plan_grad_densities(name, real, 1, N, N)
            assert pl["rows_per_pass"] == 1 and pl["passes"] == 1
            assert all(pl[side][k] == single[side][k] for side in ("trg", "src") for k in ("splits", "workspace_bytes")), (pl, single)
            assert sctl_amd.plan_grad_densities(name, real, 0, N, N)["passes"] == 0
            full = sctl_amd.plan_grad_densities(name, real, m_max, N, N)
            for nd in (2, 3, m_max, m_max + 1, 2 * m_max, 33):
                pl = sctl_amd.plan_grad_densities(name, real, nd, N, N)
                M = pl["rows_per_pass"]
                assert M == (m_max if nd >= m_max else min(m for m in (2, 4, 8) if m >= nd)), (name, nd, pl)
                assert pl["passes"] == math.ceil(nd / m_max), (name, real, nd, N, pl)
                for side, width in (("trg", 3), ("src", 6 if info["nd"] else 3)):
                    s, ws = pl[side]["splits"], pl[side]["workspace_bytes"]
                    assert s >= 1 and (s < 8 or s % 8 == 0), (name, real, nd, N, pl)
                    assert 0 <= ws <= GB2, (name, real, nd, N, pl)
                    if nd >= m_max:                                   # the same widest form: the same plan, however many rows
                        assert pl[side] == full[side], (name, real, nd, N, pl, full)
                    if pl["passes"] == 1:
                        if s == 1:
                            assert ws == 0
                        else:                                         # whole workgroups' owners (or all of them), `width` sums each: no factor nd or M
                            per = s * width * rs
                            assert ws % per == 0 and (ws // per == N or (ws // per) % 256 == 0), (name, real, nd, N, pl)
        for Nt, Ns in ((0, 0), (0, 10), (10, 0), (1, 1), (1 << 23, 1 << 14), (1 << 14, 1 << 23)):
            pl = sctl_amd.plan_grad_densities(name, real, 5, Nt, Ns)
            assert pl["passes"] == (2 if m_max == 4 else 1) and all(pl[s]["splits"] >= 1 and 0 <= pl[s]["workspace_bytes"] <= GB2 for s in ("trg", "src"))


def test_l2_rule_counts_all_rows():
    """2^20 x 2^20 Stokes3D-FxU fp64: a split's streamed bytes, all 8 rows of a record with them, stay within 2 MB up to the cap of 64 splits, which
    the single gradient's records of 6 reals do not reach"""
    N = 1 << 20
    one = sctl_amd.plan_grad("Stokes3D-FxU", 0, N, N)
    pl = sctl_amd.plan_grad_densities("Stokes3D-FxU", 0, 8, N, N)
    want = lambda reals: min(64, -(-(-(-N * reals * 8 // (2 << 20))) // 8) * 8)
    assert one["trg"]["splits"] == want(6) == 24 and pl["trg"]["splits"] == want(3 + 8 * 3) == 64, (one, pl)
    assert pl["src"]["splits"] == 64 and pl["trg"]["workspace_bytes"] == 64 * N * 3 * 8


_CHILD = r"""
import json, sys
import sctl_amd
print(json.dumps([sctl_amd.plan_grad_densities(sys.argv[1], 0, int(sys.argv[2]), 1 << 22, 1 << 22), sctl_amd.plan_grad(sys.argv[1], 0, 1 << 22, 1 << 22)]))
"""


def test_workspace_bound_follows_the_lowered_variable_in_a_fresh_process():
    """Stokes3D-DxU fp64, 8 rows at 2^22 x 2^22: 64 splits of 6 sums per source would be 12 GB, so a launch holds 2^31 / (64 * 48 B) owners in whole
    workgroups; SCTL_AMD_TRANSPOSE_WORKSPACE lowers that bound (here to one workgroup per launch), as it does for the single gradient, never raises it"""
    import json
    def run(value):
        env = dict(os.environ)
        env.pop("SCTL_AMD_TRANSPOSE_WORKSPACE", None)
        if value is not None:
            env["SCTL_AMD_TRANSPOSE_WORKSPACE"] = value
        p = subprocess.run([sys.executable, "-c", _CHILD, "Stokes3D-DxU", "8"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert p.returncode == 0, p.stderr
        return json.loads(p.stdout.strip().splitlines()[-1])
    default, single = run(None)
    assert default["src"]["splits"] == 64 and default["src"]["workspace_bytes"] == 64 * 48 * ((GB2 // (64 * 48)) // 256 * 256) <= GB2, default
    assert default["trg"]["workspace_bytes"] == 64 * 24 * ((GB2 // (64 * 24)) // 256 * 256) <= GB2
    assert single["src"]["workspace_bytes"] <= GB2
    low, low_single = run("1")
    assert low["src"]["splits"] % 8 == 0 and low["src"]["workspace_bytes"] == low["src"]["splits"] * 256 * 48, low
    assert low["trg"]["workspace_bytes"] == low["trg"]["splits"] * 256 * 24, low
    assert low_single["src"]["workspace_bytes"] == low_single["src"]["splits"] * 256 * 48, low_single
    assert run(str(1 << 40)) == [default, single]


# ---- the device assembly of the gmulti_*.hip units ------------------------------------------------------------------------------------------
def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten gmulti_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("gmulti_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = []
    for u in UNITS:
        extra = mk("print-unit-flags", "UNIT=" + u)
        assert "-fno-slp-vectorize" in extra, (u, extra)
        jobs.append((u, flags + extra, str(td / (u + ".s"))))
    with ThreadPoolExecutor(max_workers=5) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_units_are_the_ten_kernels_and_in_the_makefile():
    assert sorted(f[:-4] for f in os.listdir(CSRC) if f.startswith("gmulti_") and f.endswith(".hip")) == sorted(UNITS)
    assert "gmulti_%.o" in open(os.path.join(CSRC, "Makefile")).read()


def test_shipped_forms_have_no_scratch_two_waves_per_simd_and_no_atomic(unit_asm):
    """Every eval_multi_grad_kernel<Ker, R, MODE, SIDE, 1, M> the library launches: ScratchSize 0, at most 256 vector registers (two waves per SIMD),
    an LDS allocation of which two 256-lane workgroups fit a CU (160 KB), and no atomic instruction in the unit.  Per kernel: fp64 modes 0-2 and fp32
    modes 0-1, both sides, the forms of 2, 4 (and 8) rows."""
    for name, unit in zip(sctl_amd.KERNEL_NAMES, UNITS):
        src = open(unit_asm[unit]).read()
        seen = set()
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*eval_multi_grad_kernelINS_\d*(\w+?)E([df])Li(\d)ELi(\d)ELi1ELi(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, side, M, body = m.groups()
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
            vgpr, lds = field("next_free_vgpr"), field("group_segment_fixed_size")
            print("%s %s mode %s side %s M %s: %d VGPRs, %d B LDS" % (ker, real, mode, side, M, vgpr, lds))
            assert ker == name.replace("-", "_")
            assert field("private_segment_fixed_size") == 0, sym
            assert vgpr <= 256, (sym, vgpr)
            assert (160 * 1024) // ((lds + 1279) // 1280 * 1280) >= 2, (sym, lds)
            seen.add((real, int(mode), int(side), int(M)))
        forms = [m for m in (2, 4, 8) if m <= M_MAX[name]]
        assert seen == {(r, mode, side, m) for r, modes in (("d", 3), ("f", 2)) for mode in range(modes) for side in (0, 1) for m in forms}, (unit, sorted(seen))
        assert not re.search(r"^\s+\w*atomic\w*\s", src, re.M), unit


def test_new_units_pass_the_isa_rules(unit_asm):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa_rules.py")] + sorted(unit_asm.values()), capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" 0 finding(s)") == len(UNITS)


def test_host_header_eval_grad_densities_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "grad_densities_driver")
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "grad_densities_driver.cpp"),
                    "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    if sctl_amd.device_count() > 0:
        return                      # with a GPU the driver runs in tests/test_gpu_grad_densities.py
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode != 0
    assert "no CPU fallback" in p.stderr
