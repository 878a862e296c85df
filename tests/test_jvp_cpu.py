"""The tangent of a kernel sum along a perturbation of the geometry (sctl_amd_eval_jvp_*): what can be checked without a GPU.  The three symbols in
the library, the header and the binding, the argument checks (before any device work, through C and through Python) and the refusal of work without
a device and of plugin kernels, the planner's arithmetic including the cut of the targets, the device assembly of the ten inst_j_*.hip units (no
scratch; the register counts are printed), and a C++ driver that type-checks GenericKernel::EvalJvp."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

OK, UNKNOWN_KERNEL, BAD_ARGUMENT, NO_DEVICE, BAD_CONTEXT = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
SYMS = ("sctl_amd_eval_jvp_device", "sctl_amd_eval_jvp_host", "sctl_amd_eval_jvp_plan")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    assert set(re.findall(r"\bint (sctl_amd_eval_jvp_\w+)\(", hdr)) == set(SYMS)
    assert int(re.search(r"#define SCTL_AMD_DEVICE_ABI (\d+)", hdr).group(1)) == 4        # the plugin ABI did not move
    for f in ("eval_jvp_host", "eval_jvp_device", "plan_jvp"):
        assert callable(getattr(sctl_amd, f)) and f in sctl_amd.__all__
    assert callable(sctl_amd.GenericKernel.EvalJvp)
    from sctl_amd.autograd import _KernelSumGeometry
    assert callable(_KernelSumGeometry.jvp) and callable(_KernelSumGeometry.backward)


def test_bad_arguments_are_refused_before_anything_else():
    L = sctl_amd.lib()
    z = np.zeros(64)
    dev = lambda *a: L.sctl_amd_eval_jvp_device(*a)
    host = lambda *a: L.sctl_amd_eval_jvp_host(*a)
    err = lambda: L.sctl_amd_last_error()
    # (kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, dv_trg, [accumulate,] digits, ctx, ctx_bytes, stream | device)
    assert dev(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), -1, None, 0, None) == UNKNOWN_KERNEL
    assert host(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), 1, -1, None, 0, 0) == UNKNOWN_KERNEL
    assert dev(0, 7, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"real must be" in err()
    assert dev(0, 0, -1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"negative size" in err()
    assert host(0, 0, 1, 1, None, _p(z), None, _p(z), _p(z), _p(z), None, _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null coordinate" in err()
    assert host(0, 0, 1, 1, _p(z), _p(z), None, None, _p(z), _p(z), None, _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null density or tangent result" in err()
    assert dev(0, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, None, -1, None, 0, None) == BAD_ARGUMENT and b"null density or tangent result" in err()
    assert host(1, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"needs source normals" in err()
    assert host(9, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), None, _p(z), 1, -1, None, 0, 0) == BAD_CONTEXT and b"context blob of 16 bytes" in err()
    # d_nrm for a kernel without a normal, on both entries, whatever other tangents there are
    for k in (0, 2, 3, 5, 6, 7):
        assert host(k, 0, 1, 1, _p(z), _p(z), None, _p(z), None, None, _p(z), _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"d_nrm must be null" in err()
        assert dev(k, 1, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"d_nrm must be null" in err()
    assert L.sctl_amd_eval_jvp_plan(99, 0, 10, 10, -1, None, None, None) == UNKNOWN_KERNEL
    assert L.sctl_amd_eval_jvp_plan(0, 3, 10, 10, -1, None, None, None) == BAD_ARGUMENT
    assert L.sctl_amd_eval_jvp_plan(0, 0, -10, 10, -1, None, None, None) == BAD_ARGUMENT
    assert L.sctl_amd_eval_jvp_plan(0, 0, 10, 10, -1, None, None, None) == OK          # every output of the plan is optional
    # ... and through Python
    x = np.zeros(30)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="d_nrm must be null"):
        sctl_amd.eval_jvp_host("Laplace3D-FxU", x, x, None, np.zeros(10), d_trg=x, d_nrm=np.zeros(30))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="d_trg must be"):
        sctl_amd.eval_jvp_host("Laplace3D-FxU", x, x, None, np.zeros(10), d_trg=np.zeros(10))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="d_src must be"):
        sctl_amd.eval_jvp_host("Laplace3D-FxU", x, x, None, np.zeros(10), d_src=np.zeros(30, dtype=np.float32))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="d_nrm must be"):
        sctl_amd.eval_jvp_host("Laplace3D-DxU", x, x, x, np.zeros(10), d_nrm=np.zeros(10))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="v_src must be"):
        sctl_amd.eval_jvp_host("Stokes3D-FxU", x, x, None, np.zeros(10), d_trg=x)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        sctl_amd.eval_jvp_host("Helmholtz3D-FxU", x, x, None, np.zeros(20), d_trg=x)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2"):
        sctl_amd.plan_jvp("Laplace3D-FxU", 0, -1, 10)


def test_work_without_a_device_is_refused():
    L = sctl_amd.lib()
    x = np.random.default_rng(0).random(30)
    f, du = np.ones(10), np.zeros(10)
    rc_h = L.sctl_amd_eval_jvp_host(0, 0, 10, 10, _p(x), _p(x + 1.0), None, _p(f), _p(x), None, None, _p(du), 1, -1, None, 0, 0)
    if sctl_amd.device_count() == 0:      # there is no CPU path
        assert rc_h == NO_DEVICE and b"no HIP device" in L.sctl_amd_last_error()
        assert L.sctl_amd_eval_jvp_device(0, 0, 10, 10, _p(x), _p(x), None, _p(f), _p(x), None, None, _p(du), -1, None, 0, None) == NO_DEVICE
        assert L.sctl_amd_eval_jvp_host(0, 0, 0, 10, None, _p(x), None, _p(f), None, _p(x), None, None, 1, -1, None, 0, 0) == NO_DEVICE   # as the forward entry: before the no-op
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
            sctl_amd.eval_jvp_host("Laplace3D-FxU", x, x, None, f, d_trg=x)
        assert not du.any()
    else:
        assert rc_h == OK and du.all()


PLUGIN_NAME = "Yukawa3D-FxU-J"
PLUGIN = r"""
// The screened Coulomb (Yukawa) functor, forward form only, under a name of its own: e^{-lambda r} / (4 pi r)
#include <sctl_amd/device/kernel_plugin.hpp>
struct Yukawa3D_FxU_J {
  static constexpr int ID = -1, K0 = 1, K1 = 1, ND = 0, NREC = 4, FLOPS = 10;
  static constexpr const char* NAME = "Yukawa3D-FxU-J";
  template <class R> using Consts = sctl_amd::DefaultConsts<R>;
  static constexpr double scale() { return 1 / (4 * sctl_amd::kPi); }
  static constexpr double acc_factor(int) { return 1; }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) { rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; }
  template <class R, int MODE, bool MASKED>
  static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const sctl_amd::KerCtx& ctx, const Consts<R>& K) {
    const R r2 = sctl_amd::len2(d);
    const R rinv = sctl_amd::rsqrt_masked<MODE, MASKED>(r2, K.rsq);
    acc[0] = sctl_amd::fma_(rec[3], rinv * exp_(-R(ctx.v[0]) * (r2 * rinv)), acc[0]);
  }
  static __device__ __forceinline__ double exp_(double x) { return ::exp(x); }
  static __device__ __forceinline__ float exp_(float x) { return ::expf(x); }
};
SCTL_AMD_REGISTER_KERNEL(Yukawa3D_FxU_J, /*context: lambda*/ 8)
"""


@pytest.fixture(scope="module")
def plugin(tmp_path_factory):
    try:
        return sctl_amd.kernel_id(PLUGIN_NAME)
    except KeyError:
        td = tmp_path_factory.mktemp("jvp_plugin")
        src, so, libdir = str(td / "yukawa_j_kernel.hip"), str(td / "libyukawa_j_kernel.so"), os.path.join(ROOT, "sctl_amd")
        open(src, "w").write(PLUGIN)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), src, "-o", so,
                        "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir], check=True)
        assert sctl_amd.load_plugin(so) == [PLUGIN_NAME]
        return sctl_amd.kernel_id(PLUGIN_NAME)


def test_plugin_kernels_are_refused_by_the_new_entries_only(plugin):
    """a registered kernel has no tangent form: SCTL_AMD_ERR_UNKNOWN_KERNEL from the three new entries, after the other argument checks, while its forward plan
    still answers"""
    L = sctl_amd.lib()
    kid = sctl_amd.kernel_id(PLUGIN_NAME)
    z, lam = np.zeros(64), np.array([2.5])
    assert L.sctl_amd_eval_jvp_plan(kid, 0, 10, 10, -1, None, None, None) == UNKNOWN_KERNEL and b"no tangent form" in L.sctl_amd_last_error()
    assert L.sctl_amd_eval_jvp_host(kid, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), None, None, _p(z), 1, -1, _p(lam), 8, 0) == UNKNOWN_KERNEL
    assert L.sctl_amd_eval_jvp_device(kid, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), None, None, _p(z), -1, _p(lam), 8, None) == UNKNOWN_KERNEL
    assert L.sctl_amd_eval_jvp_host(kid, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), None, None, _p(z), 1, -1, None, 0, 0) == BAD_CONTEXT
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*no tangent form"):
        sctl_amd.plan_jvp(PLUGIN_NAME, 0, 10, 10)
    assert sctl_amd.plan(PLUGIN_NAME, 0, 1000, 1000)["path"] == "exact"


def test_planner_arithmetic(monkeypatch):
    """plan_owned with the targets as owners of TrgDim sums each (256 CUs when planning without a device, the MI355X's count): one target per lane, the
    sources split in whole 256-record tiles, the workspace splits x owners x TrgDim x itemsize, and the targets cut into launches where that would pass
    the bound"""
    P = sctl_amd.plan_jvp
    for name in sctl_amd.KERNEL_NAMES:
        k1 = sctl_amd.kernel_info(name)["k1"]
        for real, item in ((0, 8), (1, 4)):
            pl = P(name, real, 300, 2000)
            assert pl["per_lane"] == 1 and pl["splits"] > 1 and pl["workspace_bytes"] == pl["splits"] * 300 * k1 * item, (name, real, pl)
            monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", "1")          # the bound lowered to one workgroup's 256 owners
            low = P(name, real, 300, 2000)
            monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
            assert low["splits"] == pl["splits"] and low["workspace_bytes"] == pl["splits"] * 256 * k1 * item, (name, real, low)
            for Nt, Ns in ((0, 0), (0, 10), (10, 0), (1, 1), (1 << 20, 1 << 20), (1 << 23, 1 << 14), (1 << 14, 1 << 23)):
                q = P(name, real, Nt, Ns)
                assert q["per_lane"] == 1 and 1 <= q["splits"] <= 1024 and 0 <= q["workspace_bytes"] <= 1 << 31, (name, real, Nt, Ns, q)
    # what follows are the figures of a 256-CU device; what stands above holds on any
    if sctl_amd.device_count() > 0:
        import torch
        if torch.cuda.get_device_properties(0).multi_processor_count != 256:
            pytest.skip("the figures below are those of a 256-CU device")
    # 300 targets: 2 workgroups, 1024 wanted -> 512 splits wanted, 8 tiles of sources: one per split
    assert P("Laplace3D-FxU", 0, 300, 2000) == dict(per_lane=1, splits=8, workspace_bytes=8 * 300 * 8)
    assert P("Stokes3D-FxT", 1, 100, 200) == dict(per_lane=1, splits=1, workspace_bytes=0)          # one tile: no partial sums
    # 20000 targets, one per lane: 79 workgroups, ceil(1024 / 79) = 13 splits wanted, 118 tiles -> 10 per split -> 12 splits
    assert P("Stokes3D-FxUP", 0, 20000, 30000) == dict(per_lane=1, splits=12, workspace_bytes=12 * 20000 * 4 * 8)
    # 2^18 x 2^18 (2^36 pairs): 1024 workgroups, 2048 wanted -> 2; the 2 MB rule: Stokeslet sources {x, dx, f} 72 B x 2^18 = 18 MB -> 9 -> 16 splits
    assert P("Stokes3D-FxU", 0, 1 << 18, 1 << 18) == dict(per_lane=1, splits=16, workspace_bytes=16 * (1 << 18) * 3 * 8)
    # the 2 GB bound at its real size: 2^22 x 2^22 traction kernel, fp64: 64 splits (the cap) x 9 sums x 8 B: 2^31 / 4608 = 466033 -> 465920 targets per launch
    assert P("Stokes3D-FxT", 0, 1 << 22, 1 << 22) == dict(per_lane=1, splits=64, workspace_bytes=64 * 465920 * 72)


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "inst_j_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten inst_j_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("inst_j_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=inst_j_" + u), str(td / ("inst_j_%s.s" % u))) for u in UNITS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_shipped_forms_have_no_scratch(unit_asm):
    """Every eval_jvp_kernel<Ker, R, MODE, T> the library launches, 50 in all, from its metadata (register counts and scratch size only): ScratchSize
    0, and an LDS allocation of which two 256-lane workgroups fit a CU (160 KB).  Per kernel: fp64 modes 0-2 and fp32 modes 0-1, one target per lane.
    The register counts are printed (DESIGN.md §4.18 quotes them)."""
    total = 0
    for unit, path in unit_asm.items():
        src = open(path).read()
        seen = set()
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*eval_jvp_kernelINS_\d+(\w+?)E([df])Li(\d)ELi(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, T, meta = m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5)), m.group(6)
            assert ker == unit, (unit, sym)
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta).group(1))
            tail = src[src.index("\n" + sym + ":"):]
            scratch, vgprs = int(re.search(r"; ScratchSize: (\d+)", tail).group(1)), int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
            lds = field("group_segment_fixed_size")
            print("%-17s %s mode %d T %d: %3d VGPRs, %5d B LDS, scratch %d" % (unit, real, mode, T, vgprs, lds, scratch))
            assert scratch == 0 and field("private_segment_fixed_size") == 0, sym
            assert vgprs <= 512, (sym, vgprs)
            assert (160 * 1024) // ((lds + 1279) // 1280 * 1280) >= 2, (sym, lds)
            seen.add((real, mode, T))
        assert seen == {(r, m, 1) for r, modes in (("d", (0, 1, 2)), ("f", (0, 1))) for m in modes}, (unit, sorted(seen))
        total += len(seen)
    assert total == 50


def test_cpp_driver_type_checks_eval_jvp(tmp_path):
    """tests/cpp/jvp_driver.cpp: GenericKernel<Stokes3D_DxU>::EvalJvp compiles under g++ -Wall -Werror against the installed headers; without a GPU it
    fails loudly, with one tests/test_gpu_jvp.py runs it"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "jvp_driver")
    if sctl_amd.device_count() == 0:
        p = subprocess.run([exe, str(tmp_path / "o.bin")], capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "no HIP device" in p.stderr
