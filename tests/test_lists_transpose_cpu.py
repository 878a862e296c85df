"""The transposed list sum (sctl_amd_lists_create_directions, sctl_amd_lists_eval_transpose_*): what can be checked without a GPU.  The symbols,
the ownership rule of each direction and the other argument checks (none needs a device), the refusal of work without a device, and the device
assembly of the ten inst_lt_*.hip units: all five instantiations, no scratch, at most 256 vector registers, and the rules of
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

OK, UNKNOWN_KERNEL, BAD_ARGUMENT, NO_DEVICE, BAD_CONTEXT = 0, -1, -2, -3, -5
FORWARD, TRANSPOSE = 1, 2
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
SYMS = ("sctl_amd_lists_create_directions", "sctl_amd_lists_eval_transpose_device", "sctl_amd_lists_eval_transpose_host", "sctl_amd_lists_transpose_info",
        "sctl_amd_eval_lists_transpose_host")
i8 = lambda *v: np.array(v, dtype=np.int64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _create(lists, directions, Nt=10, Ns=10, kernel=0):
    h = ctypes.c_void_p()
    rc = sctl_amd.lib().sctl_amd_lists_create_directions(kernel, 0, 0, lists[0].size, _p(lists[0]), _p(lists[1]), _p(lists[2]), _p(lists[3]), Nt, Ns, directions,
                                                         ctypes.byref(h))
    return rc, h, sctl_amd.lib().sctl_amd_last_error().decode()


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    assert int(re.search(r"#define SCTL_AMD_DEVICE_ABI (\d+)", hdr).group(1)) == 4
    assert re.search(r"#define SCTL_AMD_LISTS_FORWARD 1\b", hdr) and re.search(r"#define SCTL_AMD_LISTS_TRANSPOSE 2\b", hdr)
    assert callable(sctl_amd.eval_lists_transpose_host)
    for f in ("eval_transpose_host", "eval_transpose_device", "transpose_info"):
        assert callable(getattr(sctl_amd.ListsPlan, f))
    assert "void EvalListsTranspose(" in open(os.path.join(ROOT, "include", "sctl_amd", "generic-kernel.hpp")).read()
    from sctl_amd.autograd import lists_sum
    assert callable(lists_sum)


def test_each_direction_checks_its_own_ownership_rule():
    # source ranges [0,4) and [2,6): overlapping, not identical; then the same start with another length
    for lists in ((i8(0, 5), i8(2, 2), i8(0, 2), i8(4, 4)), (i8(0, 5), i8(2, 2), i8(0, 0), i8(4, 3))):
        for d in (TRANSPOSE, FORWARD | TRANSPOSE):
            rc, h, msg = _create(lists, d)
            assert rc == BAD_ARGUMENT and "source ranges of lists" in msg and re.search(r"lists (0 and 1|1 and 0)\b", msg), msg
        rc, h, msg = _create(lists, FORWARD)
        assert rc != BAD_ARGUMENT                                  # FORWARD only: source ranges overlap freely, as ever (OK with a device, else "no HIP device")
        assert rc == (OK if sctl_amd.device_count() else NO_DEVICE)
        sctl_amd.lib().sctl_amd_lists_destroy(h)
    # target ranges [0,4) and [2,6) against disjoint source ranges: refused FORWARD (the existing message), legal TRANSPOSE
    lists = (i8(0, 2), i8(4, 4), i8(0, 5), i8(2, 2))
    rc, h, msg = _create(lists, FORWARD)
    assert rc == BAD_ARGUMENT and "target ranges of lists 0 and 1 overlap" in msg
    rc, h, msg = _create(lists, FORWARD | TRANSPOSE)
    assert rc == BAD_ARGUMENT and "target ranges of lists 0 and 1 overlap" in msg
    rc, h, msg = _create(lists, TRANSPOSE)
    assert rc == (OK if sctl_amd.device_count() else NO_DEVICE), msg
    sctl_amd.lib().sctl_amd_lists_destroy(h)


def test_directions_must_be_a_known_non_empty_bit_set():
    lists = (i8(0), i8(0), i8(0), i8(0))
    for d in (0, 4, 7, -1):
        rc, h, msg = _create(lists, d)
        assert rc == BAD_ARGUMENT and "directions" in msg, (d, msg)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="directions"):
        sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *lists, 10, 10, directions="backward")
    assert _create(lists, TRANSPOSE, kernel=99)[0] == UNKNOWN_KERNEL
    assert _create((i8(8), i8(4), i8(0), i8(1)), TRANSPOSE)[0] == BAD_ARGUMENT          # targets beyond Nt


def test_plan_without_work_needs_no_device_and_leaves_g_src_alone():
    mk = lambda d: sctl_amd.ListsPlan("Stokes3D-FxU", np.float64, i8(0, 5), i8(0, 3), i8(0, 0), i8(4, 0), 10, 10, directions=d)
    for d in ("transpose", "both"):
        p = mk(d)
        assert p.transpose_info() == dict(pairs=0, work_items=0, target_ranges=0)
        g0 = np.arange(30.0)
        g = p.eval_transpose_host(np.zeros(30), np.ones(30), None, np.ones(30), g_src=g0.copy())
        assert np.array_equal(g, g0)
        assert np.array_equal(p.eval_transpose_host(np.zeros(30), np.ones(30), None, np.ones(30)), np.zeros(30))
        p.close()
    assert np.array_equal(sctl_amd.eval_lists_transpose_host("Stokes3D-FxU", i8(0), i8(0), i8(0), i8(3), np.zeros(30), np.ones(30), None, np.ones(30)), np.zeros(30))


def test_a_direction_that_was_not_planned_is_refused():
    L = sctl_amd.lib()
    z = np.zeros(64)
    empty = (i8(0), i8(0), i8(0), i8(0))
    fwd = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *empty, 10, 10)
    assert fwd.transpose_info() == dict(pairs=0, work_items=0, target_ranges=0)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2.*TRANSPOSE"):
        fwd.eval_transpose_host(np.zeros(30), np.zeros(30), None, np.zeros(10))
    assert L.sctl_amd_lists_eval_transpose_device(fwd._h, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT
    tr = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *empty, 10, 10, directions="transpose")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -2.*FORWARD"):
        tr.eval_host(np.zeros(30), np.zeros(30), None, np.zeros(10))
    assert L.sctl_amd_lists_eval_device(tr._h, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT
    assert L.sctl_amd_lists_eval_densities_host(tr._h, 2, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT
    assert L.sctl_amd_lists_eval_transpose_host(None, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT and b"null handle" in L.sctl_amd_last_error()
    from sctl_amd.autograd import lists_sum
    for p in (fwd, tr):
        with pytest.raises(sctl_amd.api.SctlAmdError, match='directions="both"'):
            lists_sum(p, None, None, None, None)


def test_wrong_sizes_and_a_missing_context_are_errors():
    empty = (i8(0), i8(0), i8(0), i8(0))
    p = sctl_amd.ListsPlan("Stokes3D-FxUP", np.float64, *empty, 10, 10, directions="transpose")      # SrcDim 3, TrgDim 4
    with pytest.raises(sctl_amd.api.SctlAmdError, match="w_trg must be"):
        p.eval_transpose_host(np.zeros(30), np.zeros(30), None, np.zeros(30))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="g_src must be"):
        p.eval_transpose_host(np.zeros(30), np.zeros(30), None, np.zeros(40), g_src=np.zeros(40))
    h = sctl_amd.ListsPlan("Helmholtz3D-FxU", np.float64, *empty, 10, 10, directions="transpose")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        h.eval_transpose_host(np.zeros(30), np.zeros(30), None, np.zeros(20))
    z = np.zeros(64)
    L = sctl_amd.lib()
    assert L.sctl_amd_lists_eval_transpose_host(h._h, _p(z), _p(z), None, _p(z), _p(z), -1, _p(z), 8) == BAD_CONTEXT
    assert L.sctl_amd_lists_eval_transpose_device(h._h, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_CONTEXT


def test_work_without_a_device_is_refused():
    x = np.random.default_rng(0).random(30)
    lists = (i8(0), i8(4), i8(0), i8(4))
    g = np.zeros(10)
    if sctl_amd.device_count() == 0:      # there is no CPU path
        for d in ("transpose", "both"):
            with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
                sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *lists, 10, 10, directions=d)
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
            sctl_amd.eval_lists_transpose_host("Laplace3D-FxU", *lists, x, x, None, np.ones(10), g_src=g)
        assert not g.any()
    else:
        sctl_amd.eval_lists_transpose_host("Laplace3D-FxU", *lists, x, x, None, np.ones(10), g_src=g)
        assert g[:4].all() and not g[4:].any()


def test_cpp_driver_compiles_against_the_host_headers(tmp_path):
    """tests/cpp/lists_transpose_driver.cpp (GenericKernel::EvalListsTranspose) builds with g++ -Wall -Werror; tests/test_gpu_lists_transpose.py runs it"""
    from test_cpp_host import _build
    assert os.path.exists(_build(tmp_path, "lists_transpose_driver"))


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "inst_lt_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten inst_lt_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("inst_lt_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=inst_lt_" + u), str(td / ("inst_lt_%s.s" % u))) for u in UNITS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_shipped_forms_have_no_scratch_and_two_waves_per_simd(unit_asm):
    """Every lists_transpose_kernel<Ker, R, MODE> the library launches (all seven item shapes are branches of the one kernel): ScratchSize 0 and
    at most 256 vector registers (512 per SIMD lane: two waves); the LDS allocation is printed.  Per kernel: fp64 modes 0-2 and fp32 modes 0-1."""
    for unit, path in unit_asm.items():
        src = open(path).read()
        seen = set()
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*lists_transpose_kernelINS_\d+(\w+?)E([df])Li(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, meta = m.group(1), m.group(2), m.group(3), int(m.group(4)), m.group(5)
            assert ker == unit, (unit, sym)
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta).group(1))
            tail = src[src.index("\n" + sym + ":"):]
            scratch, vgprs = int(re.search(r"; ScratchSize: (\d+)", tail).group(1)), int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
            lds = field("group_segment_fixed_size")
            print("%-17s %s mode %d: %3d VGPRs, %5d B LDS, scratch %d" % (unit, real, mode, vgprs, lds, scratch))
            assert scratch == 0 and field("private_segment_fixed_size") == 0, sym
            assert vgprs <= 256, (sym, vgprs)
            seen.add((real, mode))
        assert seen == {(r, m) for r, modes in (("d", (0, 1, 2)), ("f", (0, 1))) for m in modes}, (unit, sorted(seen))


def test_new_units_pass_the_isa_rules(unit_asm):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa_rules.py")] + sorted(unit_asm.values()), capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(" 0 finding(s)") == len(UNITS)
