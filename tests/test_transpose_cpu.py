"""The transposed kernel sum (sctl_amd_eval_transpose_*): what can be checked without a GPU.  The three symbols, the argument checks and the
refusal of work without a device, the planner's arithmetic including the 2 GB cut of the owners, and the device assembly of the ten inst_t_*.hip
units: no scratch, registers and LDS that leave two or more waves per SIMD, and the rules of tools/check_isa_rules.py."""
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

OK, UNKNOWN_KERNEL, BAD_ARGUMENT, NO_DEVICE, BAD_CONTEXT = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
SYMS = ("sctl_amd_eval_transpose_device", "sctl_amd_eval_transpose_host", "sctl_amd_eval_transpose_plan")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    assert int(re.search(r"#define SCTL_AMD_DEVICE_ABI (\d+)", hdr).group(1)) == 4
    for f in ("eval_transpose_host", "eval_transpose_device", "plan_transpose"):
        assert callable(getattr(sctl_amd, f))
    assert callable(sctl_amd.GenericKernel.EvalTranspose)


def test_bad_arguments_are_refused_before_anything_else():
    L = sctl_amd.lib()
    z = np.zeros(64)
    dev = lambda *a: L.sctl_amd_eval_transpose_device(*a)
    host = lambda *a: L.sctl_amd_eval_transpose_host(*a)
    assert dev(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == UNKNOWN_KERNEL
    assert host(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), 1, -1, None, 0, 0) == UNKNOWN_KERNEL
    assert dev(0, 7, 1, 1, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"real must be" in L.sctl_amd_last_error()
    assert dev(0, 0, -1, 1, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"negative size" in L.sctl_amd_last_error()
    assert host(0, 0, 1, 1, None, _p(z), None, _p(z), _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null coordinate" in L.sctl_amd_last_error()
    assert host(0, 0, 1, 1, _p(z), _p(z), None, None, _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null weight or result" in L.sctl_amd_last_error()
    assert dev(0, 0, 1, 1, _p(z), _p(z), None, _p(z), None, -1, None, 0, None) == BAD_ARGUMENT and b"null weight or result" in L.sctl_amd_last_error()
    assert host(1, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"needs source normals" in L.sctl_amd_last_error()
    assert host(9, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), 1, -1, None, 0, 0) == BAD_CONTEXT and b"context blob of 16 bytes" in L.sctl_amd_last_error()
    assert dev(9, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), -1, _p(z), 8, None) == BAD_CONTEXT
    assert L.sctl_amd_eval_transpose_plan(99, 0, 10, 10, -1, None, None, None) == UNKNOWN_KERNEL
    assert L.sctl_amd_eval_transpose_plan(0, 3, 10, 10, -1, None, None, None) == BAD_ARGUMENT
    assert L.sctl_amd_eval_transpose_plan(0, 0, -10, 10, -1, None, None, None) == BAD_ARGUMENT
    with pytest.raises(sctl_amd.api.SctlAmdError, match="w_trg must be"):
        sctl_amd.eval_transpose_host("Stokes3D-FxUP", np.zeros(30), np.zeros(30), None, np.zeros(30))     # TrgDim 4: 40 weights
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        sctl_amd.eval_transpose_host("Helmholtz3D-FxU", np.zeros(30), np.zeros(30), None, np.zeros(20))


def test_work_without_a_device_is_refused():
    L = sctl_amd.lib()
    x = np.random.default_rng(0).random(30)
    w, g = np.ones(10), np.zeros(10)
    rc_h = L.sctl_amd_eval_transpose_host(0, 0, 10, 10, _p(x), _p(x), None, _p(w), _p(g), 1, -1, None, 0, 0)
    if sctl_amd.device_count() == 0:      # there is no CPU path
        assert rc_h == NO_DEVICE and b"no HIP device" in L.sctl_amd_last_error()
        assert L.sctl_amd_eval_transpose_device(0, 0, 10, 10, _p(x), _p(x), None, _p(w), _p(g), -1, None, 0, None) == NO_DEVICE
        assert L.sctl_amd_eval_transpose_host(0, 0, 0, 10, None, _p(x), None, None, _p(g), 1, -1, None, 0, 0) == NO_DEVICE   # as the forward entry: before the no-op
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
            sctl_amd.eval_transpose_host("Laplace3D-FxU", x, x, None, w)
        assert not g.any()
    else:
        assert rc_h == OK and g.all()


def test_planner_arithmetic():
    """make_plan with the roles exchanged (256 CUs when planning without a device, the MI355X's count): sources per lane from the source count,
    splits of the TARGET range in whole 256-record tiles, partial sums [splits][Ns * SrcDim]"""
    P = sctl_amd.plan_transpose
    if sctl_amd.device_count() > 0:
        import torch
        if torch.cuda.get_device_properties(0).multi_processor_count != 256:
            pytest.skip("the figures below are those of a 256-CU device")
    assert P("Laplace3D-FxU", 0, 1000, 300) == dict(src_per_lane=1, splits=4, workspace_bytes=4 * 300 * 8)       # 4 tiles, one per split
    assert P("Laplace3D-FxU", 0, 100, 300) == dict(src_per_lane=1, splits=1, workspace_bytes=0)                 # one tile: no partial sums
    assert P("Stokes3D-FxT", 1, 40000, 64) == dict(src_per_lane=1, splits=157, workspace_bytes=157 * 64 * 3 * 4)
    assert P("Stokes3D-FSxU", 0, 4096, 64) == dict(src_per_lane=1, splits=16, workspace_bytes=16 * 64 * 4 * 8)
    # 20000 sources, one per lane: 79 workgroups, ceil(1024 / 79) = 13 splits wanted, 118 tiles -> 10 per split -> 12 splits
    assert P("Laplace3D-DxU", 0, 30000, 20000) == dict(src_per_lane=1, splits=12, workspace_bytes=12 * 20000 * 8)
    # two sources per lane from 2^15 sources on; 2^18 x 2^18 (2^36 pairs): 2048 wanted / 512 workgroups = 4, the 2 MB rule asks for 8 MB / 2 MB = 4 -> 8
    assert P("Laplace3D-FxU", 0, 1 << 18, 1 << 18) == dict(src_per_lane=2, splits=8, workspace_bytes=8 * (1 << 18) * 8)
    assert P("Laplace3D-FxU", 0, 1 << 18, (1 << 15) - 1)["src_per_lane"] == 1
    # the 2 GB bound: 2^22 x 2^22, SrcDim 4, fp64: 96 x 2 MB of targets -> 64 splits (the cap); 64 * 2^22 * 32 B = 8 GB of partial sums for one launch,
    # so the sources go in launches of 2^31 / (64 * 32) = 2^20: the splits stay 64
    pl = P("Stokes3D-FSxU", 0, 1 << 22, 1 << 22)
    assert pl == dict(src_per_lane=2, splits=64, workspace_bytes=1 << 31)
    pl = P("Stokes3D-FxT", 0, 1 << 23, 3000000)          # SrcDim 3: 2^31 / (64 * 24) = 1398101 -> whole workgroups of 512 sources: 1397760
    assert pl["splits"] == 64 and pl["workspace_bytes"] == 64 * 1397760 * 24 <= 1 << 31
    for name in sctl_amd.KERNEL_NAMES:
        for real in (0, 1):
            for Nt, Ns in ((0, 0), (0, 10), (10, 0), (1, 1), (1 << 20, 1 << 20), (1 << 23, 1 << 14), (1 << 14, 1 << 23)):
                pl = P(name, real, Nt, Ns)
                assert pl["src_per_lane"] in (1, 2) and 1 <= pl["splits"] <= 1024 and 0 <= pl["workspace_bytes"] <= 1 << 31, (name, real, Nt, Ns, pl)


def test_workspace_bound_can_be_lowered_but_not_raised(monkeypatch):
    """SCTL_AMD_TRANSPOSE_WORKSPACE lowers the 2 GB bound (tests/test_gpu_transpose.py runs the cut of the owners on small shapes with it); a launch
    always holds one whole workgroup's owners, and a value above 2 GB or a malformed one leaves the bound where it is"""
    P = lambda: sctl_amd.plan_transpose("Stokes3D-FSxU", 0, 1 << 22, 1 << 22)
    assert P() == dict(src_per_lane=2, splits=64, workspace_bytes=1 << 31)
    for value, owners in (("1", 512), (str(64 * 32 * 1000), 512), (str(64 * 32 * 1024), 1024), (str(1 << 40), 1 << 20), ("-5", 1 << 20), ("x", 1 << 20), ("", 1 << 20)):
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", value)
        assert P() == dict(src_per_lane=2, splits=64, workspace_bytes=64 * owners * 32), value
    monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
    assert P()["workspace_bytes"] == 1 << 31


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "inst_t_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten inst_t_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("inst_t_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=inst_t_" + u), str(td / ("inst_t_%s.s" % u))) for u in UNITS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_shipped_forms_have_no_scratch_and_two_waves_per_simd(unit_asm):
    """Every eval_transpose_kernel<Ker, R, MODE, T> the library launches: ScratchSize 0, at most 256 vector registers (512 per SIMD lane: two
    waves), and an LDS allocation of which two 256-lane workgroups fit a CU (160 KB): each has one wave on every SIMD.  Per kernel: fp64 modes
    0-2 and fp32 modes 0-1, one and two sources per lane."""
    for unit, path in unit_asm.items():
        src = open(path).read()
        seen = set()
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*eval_transpose_kernelINS_\d+(\w+?)E([df])Li(\d)ELi(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, T, meta = m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5)), m.group(6)
            assert ker == unit, (unit, sym)
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta).group(1))
            tail = src[src.index("\n" + sym + ":"):]
            scratch, vgprs = int(re.search(r"; ScratchSize: (\d+)", tail).group(1)), int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
            lds = field("group_segment_fixed_size")
            print("%-17s %s mode %d T %d: %3d VGPRs, %5d B LDS, scratch %d" % (unit, real, mode, T, vgprs, lds, scratch))
            assert scratch == 0 and field("private_segment_fixed_size") == 0, sym
            assert 512 // vgprs >= 2, (sym, vgprs)
            assert (160 * 1024) // ((lds + 1279) // 1280 * 1280) >= 2, (sym, lds)
            seen.add((real, mode, T))
        assert seen == {(r, m, T) for r, modes in (("d", (0, 1, 2)), ("f", (0, 1))) for m in modes for T in (1, 2)}, (unit, sorted(seen))


def test_new_units_pass_the_isa_rules(unit_asm):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa_rules.py")] + sorted(unit_asm.values()), capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" 0 finding(s)") == len(UNITS)
