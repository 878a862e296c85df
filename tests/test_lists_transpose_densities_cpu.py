"""Several weight vectors through the transposed sum over the P2P lists (sctl_amd_lists_eval_transpose_densities_*,
sctl_amd_eval_lists_transpose_densities_host): what can be checked without a GPU.  The argument and context errors of the Python wrappers and
of the raw C ABI and their order, nd == 0, a plan without work, the refusal of real work without a device, and the ISA metadata of every
shipped (kernel, precision, M) form of lists_multi_transpose_kernel: no scratch, and registers and LDS that leave two or more waves per SIMD."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT

OK, BAD_ARGUMENT, BAD_CONTEXT = 0, -2, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
i8 = lambda *v: np.array(v, dtype=np.int64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _empty_plan(name="Laplace3D-FxU", ctx=None, directions="both"):
    """only empty lists: a legal plan without work, no GPU needed"""
    return sctl_amd.ListsPlan(name, np.float64, i8(0, 5), i8(0, 3), i8(0, 0), i8(4, 0), 10, 10, ctx=ctx, directions=directions)


def test_error_codes_agree_with_the_header():
    txt = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name, val in (("SCTL_AMD_ERR_BAD_ARGUMENT", BAD_ARGUMENT), ("SCTL_AMD_ERR_BAD_CONTEXT", BAD_CONTEXT)):
        assert int(re.search(name + r" = (-?\d+)", txt).group(1)) == val


def test_symbols_and_raw_abi_errors():
    L = sctl_amd.lib()
    for name in ("sctl_amd_lists_eval_transpose_densities_device", "sctl_amd_lists_eval_transpose_densities_host", "sctl_amd_eval_lists_transpose_densities_host"):
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name)
    z = np.zeros(30)
    for nd in (-1, 0, 2):                                                           # a null handle is refused whatever nd is
        assert L.sctl_amd_lists_eval_transpose_densities_host(None, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT
        assert b"null handle" in L.sctl_amd_last_error()
        assert L.sctl_amd_lists_eval_transpose_densities_device(None, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT
        assert b"null handle" in L.sctl_amd_last_error()
    p = _empty_plan()
    assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, -1, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT
    assert b"negative number of densities" in L.sctl_amd_last_error()
    assert L.sctl_amd_lists_eval_transpose_densities_device(p._h, -3, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT
    assert b"negative number of densities" in L.sctl_amd_last_error()
    a = [i8(0), i8(4), i8(0), i8(4)]
    assert L.sctl_amd_eval_lists_transpose_densities_host(0, 0, -1, 1, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), 10, 10, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0,
                                                          0) == BAD_ARGUMENT
    assert b"negative number of densities" in L.sctl_amd_last_error()              # before the plan: no "no HIP device" here
    p.close()


def test_a_forward_only_plan_is_refused():
    L = sctl_amd.lib()
    z = np.zeros(30)
    p = _empty_plan(directions="forward")
    for nd in (0, 1, 2, 5):
        assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT
        assert b"this plan was not made for the TRANSPOSE direction" in L.sctl_amd_last_error()
        assert L.sctl_amd_lists_eval_transpose_densities_device(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT
        assert b"this plan was not made for the TRANSPOSE direction" in L.sctl_amd_last_error()
    assert L.sctl_amd_lists_eval_transpose_host(p._h, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_ARGUMENT     # the single-vector entry's wording
    assert b"this plan was not made for the TRANSPOSE direction" in L.sctl_amd_last_error()
    with pytest.raises(sctl_amd.api.SctlAmdError, match="TRANSPOSE direction"):
        p.eval_transpose_densities_host(z, z, None, np.ones((2, 10)))
    p.close()


def test_bad_context_for_helmholtz_comes_before_anything_else():
    L = sctl_amd.lib()
    z = np.zeros(60)
    k = np.array([3.0, 0.2])
    p = _empty_plan("Helmholtz3D-FxU", ctx=k)
    for nd in (-1, 0, 1, 3):                                                        # ... a negative nd included
        assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_CONTEXT
        assert b"context blob of 16 bytes" in L.sctl_amd_last_error()
        assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, _p(k), 8) == BAD_CONTEXT
        assert L.sctl_amd_lists_eval_transpose_densities_device(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0, None) == BAD_CONTEXT
        if nd >= 0:
            assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, nd, _p(z), _p(z), None, _p(z), _p(z), -1, _p(k), 16) == OK     # (no work: nothing to do)
    p.close()
    fwd = _empty_plan("Helmholtz3D-FxU", ctx=k, directions="forward")             # ... and a plan of the wrong direction
    assert L.sctl_amd_lists_eval_transpose_densities_host(fwd._h, 2, _p(z), _p(z), None, _p(z), _p(z), -1, None, 0) == BAD_CONTEXT
    assert L.sctl_amd_lists_eval_transpose_densities_host(fwd._h, 2, _p(z), _p(z), None, _p(z), _p(z), -1, _p(k), 16) == BAD_ARGUMENT
    fwd.close()
    bad = sctl_amd.ListsPlan("Helmholtz3D-FxU", np.float64, i8(0), i8(0), i8(0), i8(0), 10, 10, ctx=None, directions="both")     # through Python
    with pytest.raises(sctl_amd.api.SctlAmdError, match="needs a context"):
        bad.eval_transpose_densities_host(np.zeros(30), np.ones(30), None, np.ones((3, 20)))
    bad.close()


def test_python_wrappers_check_shapes_before_the_library():
    p = _empty_plan()
    x = np.zeros(30)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        p.eval_transpose_densities_host(x, x, None, np.zeros(10))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        p.eval_transpose_densities_host(x, x, None, np.zeros((2, 9)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        sctl_amd.eval_lists_transpose_densities_host("Laplace3D-FxU", i8(0), i8(0), i8(0), i8(0), x, x, None, np.zeros((2, 9)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):                  # Stokeslet: TrgDim 3, a row has Nt*3 = 30 values
        sctl_amd.eval_lists_transpose_densities_host("Stokes3D-FxU", i8(0), i8(0), i8(0), i8(0), x, x, None, np.zeros((2, 10)))
    with pytest.raises(sctl_amd.api.SctlAmdError):
        p.eval_transpose_densities_host(x, x, None, np.zeros((2, 10), dtype=np.float32))
    with pytest.raises(sctl_amd.api.SctlAmdError):
        p.eval_transpose_densities_host(x, x, None, np.zeros((4, 10))[::2])        # rows that are not contiguous
    p.close()


def test_nd0_leaves_g_src_untouched():
    L = sctl_amd.lib()
    p = _empty_plan()
    x, g = np.zeros(30), np.full(10, 0.75)
    assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, 0, _p(x), _p(x), None, None, _p(g), -1, None, 0) == OK
    assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, 0, None, None, None, None, None, -1, None, 0) == OK
    assert L.sctl_amd_lists_eval_transpose_densities_device(p._h, 0, None, None, None, None, None, -1, None, 0, None) == OK
    assert L.sctl_amd_eval_lists_transpose_densities_host(0, 0, 0, 0, None, None, None, None, 10, 10, _p(x), _p(x), None, None, _p(g), -1, None, 0, 0) == OK
    assert np.all(g == 0.75)
    G = p.eval_transpose_densities_host(x, x, None, np.zeros((0, 10)))
    assert G.shape == (0, 10)
    p.close()


def test_plan_of_empty_lists_returns_zeros_and_needs_no_device():
    p = _empty_plan()
    assert p.transpose_info() == dict(pairs=0, work_items=0, target_ranges=0)
    G = p.eval_transpose_densities_host(np.zeros(30), np.ones(30), None, np.ones((3, 10)))
    assert G.shape == (3, 10) and G.dtype == np.float64 and not G.any()
    G0 = np.arange(30.0).reshape(3, 10)
    assert np.array_equal(p.eval_transpose_densities_host(np.zeros(30), np.ones(30), None, np.ones((3, 10)), G_src=G0.copy()), G0)
    L = sctl_amd.lib()                    # without work the arrays are not looked at: null arrays are fine, as in sctl_amd_lists_eval_transpose_host
    assert L.sctl_amd_lists_eval_transpose_densities_host(p._h, 3, None, None, None, None, None, -1, None, 0) == OK
    assert L.sctl_amd_lists_eval_transpose_densities_device(p._h, 3, None, None, None, None, None, -1, None, 0, None) == OK
    p.close()
    one = sctl_amd.eval_lists_transpose_densities_host("Stokes3D-FxU", i8(0, 5), i8(0, 3), i8(0, 0), i8(4, 0), np.zeros(30), np.ones(30), None, np.ones((3, 30)))
    assert one.shape == (3, 30) and not one.any()


def test_work_without_a_device_is_refused():
    x = np.random.default_rng(0).random(30)
    call = lambda: sctl_amd.eval_lists_transpose_densities_host("Laplace3D-FxU", i8(0), i8(4), i8(0), i8(4), x, x, None, np.ones((3, 10)))
    if sctl_amd.device_count() == 0:      # real work without a GPU: refused, there is no CPU path
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
            call()
    else:
        assert call().shape == (3, 10)


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "ltmulti_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return open(out).read()


def test_shipped_forms_have_no_scratch_and_two_waves_per_simd(tmp_path):
    """The ten ltmulti_*.hip units with the Makefile's flags.  Every lists_multi_transpose_kernel in them is a shipped form: ScratchSize 0, at most
    256 vector registers (512 per SIMD lane: two waves), and an LDS allocation (granules of 1280 bytes on gfx950, 160 KB per CU, one wave per
    workgroup) of which eight fit a CU: two per SIMD.  Every kernel has at least the 2-form in both precisions, and every mode of a width."""
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=ltmulti_" + u), str(tmp_path / (u + ".s"))) for u in UNITS]
    assert all("-fno-slp-vectorize" in j[1] for j in jobs)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        srcs = list(ex.map(_unit_asm, jobs))
    seen = set()
    for unit, src in zip(UNITS, srcs):
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*lists_multi_transpose_kernelINS_(\w+?)E([df])Li(\d)ELi(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, M, meta = m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5)), m.group(6)
            assert unit in ker, (unit, sym)
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta).group(1))
            tail = src[src.index("\n" + sym + ":"):]
            scratch, vgprs = int(re.search(r"; ScratchSize: (\d+)", tail).group(1)), int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
            lds = field("group_segment_fixed_size")
            print("%-17s %s mode %d M %d: %3d VGPRs, %5d B LDS, scratch %d" % (unit, real, mode, M, vgprs, lds, scratch))
            assert scratch == 0 and field("private_segment_fixed_size") == 0, sym
            assert 512 // vgprs >= 2, (sym, vgprs)
            assert 8 * ((lds + 1279) // 1280 * 1280) <= 160 * 1024, (sym, lds)
            seen.add((unit, real, mode, M))
    for unit in UNITS:
        for real, modes in (("d", (0, 1, 2)), ("f", (0, 1))):
            widths = sorted({M for (u, r, _, M) in seen if u == unit and r == real})
            assert widths and widths[0] == 2 and widths in ([2], [2, 4], [2, 4, 8]), (unit, real, widths)
            for M in widths:
                assert all((unit, real, mode, M) in seen for mode in modes), (unit, real, M)
