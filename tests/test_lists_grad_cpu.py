"""Geometry gradients over P2P lists (sctl_amd_lists_eval_grad_*, include/sctl_amd/device/lists_grad_kernel.hpp): what can be checked without a GPU.
The symbols and names, the argument checks that need no device, and the device assembly of the ten inst_lg_*.hip units: every lists_grad_kernel
(fp64 modes 0-2, fp32 modes 0-1, both sides) without scratch and within 256 vector registers — read from the kernel metadata —, and the rules of
tools/check_isa_rules.py."""
import ctypes
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

BAD_ARGUMENT = -2
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
SYMS = ("sctl_amd_lists_eval_grad_device", "sctl_amd_lists_eval_grad_host", "sctl_amd_eval_lists_grad_host")


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    assert int(re.search(r"#define SCTL_AMD_DEVICE_ABI (\d+)", hdr).group(1)) == 4      # KernelEntry and the plugin ABI stay as they are
    assert callable(sctl_amd.eval_lists_grad_host) and callable(sctl_amd.GenericKernel.EvalListsGrad)
    for f in ("eval_grad_host", "eval_grad_device"):
        assert callable(getattr(sctl_amd.ListsPlan, f))
    assert "void EvalListsGrad(" in open(os.path.join(ROOT, "include", "sctl_amd", "generic-kernel.hpp")).read()
    from sctl_amd.autograd import lists_sum_geometry
    assert callable(lists_sum_geometry)


def test_checks_that_need_no_device():
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    empty = [np.zeros(0, dtype=np.int64)] * 4
    assert L.sctl_amd_lists_eval_grad_host(None, p(z), p(z), None, p(z), p(z), p(z), None, None, -1, None, 0) == BAD_ARGUMENT and b"null handle" in L.sctl_amd_last_error()
    fwd = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *empty, 10, 10)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2.*TRANSPOSE"):
        fwd.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10))
    assert fwd.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10), want=["trg"])[1] is None
    tr = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *empty, 10, 10, directions="transpose")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2.*FORWARD"):
        tr.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10))
    both = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *empty, 10, 10, directions="both")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2.*no source normal"):
        both.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10), want=["nrm"])
    # a plan without work: nothing is launched, the outputs keep their values
    g0 = np.arange(30.0)
    g = both.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10), g_trg=g0.copy(), g_src=g0.copy())
    assert np.array_equal(g[0], g0) and np.array_equal(g[1], g0) and g[2] is None
    h = sctl_amd.ListsPlan("Helmholtz3D-FxU", np.float64, *empty, 10, 10, directions="both")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        h.eval_grad_host(np.zeros(30), np.zeros(30), None, np.zeros(20), np.zeros(20))
    from sctl_amd.autograd import lists_sum_geometry
    for q in (fwd, tr):
        with pytest.raises(sctl_amd.api.SctlAmdError, match='directions="both"'):
            lists_sum_geometry(q, None, None, None, None)


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "inst_lg_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten inst_lg_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("inst_lg_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=inst_lg_" + u), str(td / ("inst_lg_%s.s" % u))) for u in UNITS]
    assert all("-fno-slp-vectorize" in j[1] for j in jobs)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_every_form_has_no_scratch_and_two_waves_per_simd(unit_asm):
    """Every lists_grad_kernel<Ker, R, MODE, SIDE> the library launches (all seven item shapes are branches of the one kernel), from the kernel
    metadata (amdhsa.kernels): no private segment, no spilt vector register, at most 256 vector registers (two waves per SIMD)."""
    for unit, path in unit_asm.items():
        src = open(path).read()
        md = src[src.index("amdhsa.kernels:"):]
        seen = set()
        for block in re.split(r"\n  - (?=\.agpr_count:)", md)[1:]:
            field = lambda k: re.search(r"\.%s:\s+(\S+)" % k, block).group(1)
            m = re.search(r"lists_grad_kernelINS_\d+(\w+?)E([df])Li(\d)ELi(\d)E", field("name"))
            if not m:
                continue
            ker, real, mode, side = m.group(1), m.group(2), int(m.group(3)), int(m.group(4))
            assert ker == unit, (unit, field("name"))
            vgprs, lds = int(field("vgpr_count")), int(field("group_segment_fixed_size"))
            print("%-17s %s mode %d side %d: %3d VGPRs, %5d B LDS" % (unit, real, mode, side, vgprs, lds))
            assert int(field("private_segment_fixed_size")) == 0 and int(field("vgpr_spill_count")) == 0, field("name")
            assert vgprs <= 256, (field("name"), vgprs)
            seen.add((real, mode, side))
        assert seen == {(r, m, s) for r, modes in (("d", (0, 1, 2)), ("f", (0, 1))) for m in modes for s in (0, 1)}, (unit, sorted(seen))


def test_new_units_pass_the_isa_rules(unit_asm):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa_rules.py")] + sorted(unit_asm.values()), capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" 0 finding(s)") == len(UNITS)
