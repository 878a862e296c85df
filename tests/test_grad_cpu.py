"""Coordinate and normal gradients of a kernel sum (sctl_amd_eval_grad_*): what can be checked without a GPU.  The dense torch formula the GPU
tests differentiate against the reference's KernelMatrix blocks, the three symbols, the argument checks and the refusal of work without a device,
the planner's arithmetic including the 2 GB cut of the owners, and the device assembly of the ten inst_g_*.hip units: no scratch, registers and
LDS that leave two or more waves per SIMD."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, rel_l2
from grad_truth import HELMHOLTZ_KS, kernel_blocks

OK, UNKNOWN_KERNEL, BAD_ARGUMENT, NO_DEVICE, BAD_CONTEXT = 0, -1, -2, -3, -5
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
UNITS = ["Laplace3D_FxU", "Laplace3D_DxU", "Laplace3D_FxdU", "Stokes3D_FxU", "Stokes3D_DxU", "Stokes3D_FxT", "Stokes3D_FSxU", "Stokes3D_FxUP",
         "Laplace3D_FDxUdU", "Helmholtz3D_FxU"]
SYMS = ("sctl_amd_eval_grad_device", "sctl_amd_eval_grad_host", "sctl_amd_eval_grad_plan")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_torch_formula_matches_the_reference_kernel_matrix(name, O):
    """The truth of tests/test_gpu_grad.py is torch autograd of the dense formula in tests/grad_truth.py.  Its K0 x K1 blocks against the oracle's
    KernelMatrix on random points, rel-L2 <= 1e-13: derivatives of an analytic formula that matches the reference's values are the reference's
    derivatives.  Helmholtz at both wavenumbers the GPU tests use."""
    import torch
    info = sctl_amd.kernel_info(name)
    rng = np.random.default_rng(3)
    Nt, Ns = 37, 29
    xt, xs = rng.random(Nt * 3), rng.random(Ns * 3)
    xn = rng.random(Ns * 3) - 0.5 if info["nd"] else None
    for ctx in (HELMHOLTZ_KS if name.startswith("Helmholtz") else [None]):
        c = None if ctx is None else np.array(ctx)
        M = O.kernel_matrix(name, xt, xs, xn, ctx=c)                                   # (Ns*K0) x (Nt*K1)
        U = kernel_blocks(name, torch.from_numpy(xt).view(-1, 3), torch.from_numpy(xs).view(-1, 3), None if xn is None else torch.from_numpy(xn).view(-1, 3), ctx)
        mine = U.permute(1, 2, 0, 3).reshape(Ns * info["k0"], Nt * info["k1"]).numpy()   # U[t, s, k0, k1]
        err = rel_l2(mine, M)
        print("%s ctx %s: rel-L2 of the blocks %.2e" % (name, ctx, err))
        assert err <= 1e-13, (name, ctx, err)


def test_symbols_exist_in_library_header_and_binding():
    L = sctl_amd.lib()
    hdr = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    for name in SYMS:
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name) and re.search(r"\bint %s\(" % name, hdr)
    assert int(re.search(r"#define SCTL_AMD_DEVICE_ABI (\d+)", hdr).group(1)) == 4
    for f in ("eval_grad_host", "eval_grad_device", "plan_grad"):
        assert callable(getattr(sctl_amd, f))
    assert callable(sctl_amd.GenericKernel.EvalGrad)
    from sctl_amd.autograd import kernel_sum_geometry
    assert callable(kernel_sum_geometry)


def test_bad_arguments_are_refused_before_anything_else():
    L = sctl_amd.lib()
    z = np.zeros(64)
    dev = lambda *a: L.sctl_amd_eval_grad_device(*a)
    host = lambda *a: L.sctl_amd_eval_grad_host(*a)
    # (kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, [accumulate,] digits, ctx, ctx_bytes, stream | device)
    assert dev(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, -1, None, 0, None) == UNKNOWN_KERNEL
    assert host(99, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, 1, -1, None, 0, 0) == UNKNOWN_KERNEL
    assert dev(0, 7, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, -1, None, 0, None) == BAD_ARGUMENT and b"real must be" in L.sctl_amd_last_error()
    assert dev(0, 0, -1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, -1, None, 0, None) == BAD_ARGUMENT and b"negative size" in L.sctl_amd_last_error()
    assert host(0, 0, 1, 1, None, _p(z), None, _p(z), _p(z), _p(z), _p(z), None, 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null coordinate" in L.sctl_amd_last_error()
    assert host(0, 0, 1, 1, _p(z), _p(z), None, None, _p(z), _p(z), _p(z), None, 1, -1, None, 0, 0) == BAD_ARGUMENT and b"null density or weight" in L.sctl_amd_last_error()
    assert dev(0, 0, 1, 1, _p(z), _p(z), None, _p(z), None, _p(z), _p(z), None, -1, None, 0, None) == BAD_ARGUMENT and b"null density or weight" in L.sctl_amd_last_error()
    assert host(1, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, 1, -1, None, 0, 0) == BAD_ARGUMENT and b"needs source normals" in L.sctl_amd_last_error()
    assert host(9, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), None, 1, -1, None, 0, 0) == BAD_CONTEXT and b"context blob of 16 bytes" in L.sctl_amd_last_error()
    # g_nrm for a kernel without a normal, on both entries, whatever else is asked for
    for k in (0, 2, 3, 5, 6, 7):
        assert host(k, 0, 1, 1, _p(z), _p(z), None, _p(z), _p(z), None, None, _p(z), 1, -1, None, 0, 0) == BAD_ARGUMENT and b"g_nrm must be null" in L.sctl_amd_last_error()
        assert dev(k, 1, 1, 1, _p(z), _p(z), None, _p(z), _p(z), _p(z), _p(z), _p(z), -1, None, 0, None) == BAD_ARGUMENT and b"g_nrm must be null" in L.sctl_amd_last_error()
    assert L.sctl_amd_eval_grad_plan(99, 0, 10, 10, -1, None, None, None, None, None, None) == UNKNOWN_KERNEL
    assert L.sctl_amd_eval_grad_plan(0, 3, 10, 10, -1, None, None, None, None, None, None) == BAD_ARGUMENT
    assert L.sctl_amd_eval_grad_plan(0, 0, -10, 10, -1, None, None, None, None, None, None) == BAD_ARGUMENT
    with pytest.raises(sctl_amd.api.SctlAmdError, match="w_trg must be"):
        sctl_amd.eval_grad_host("Stokes3D-FxUP", np.zeros(30), np.zeros(30), None, np.zeros(30), np.zeros(30))     # TrgDim 4: 40 weights
    with pytest.raises(sctl_amd.api.SctlAmdError, match="g_nrm must be null"):
        sctl_amd.eval_grad_host("Laplace3D-FxU", np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10), want=("nrm",))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="want holds"):
        sctl_amd.eval_grad_host("Laplace3D-FxU", np.zeros(30), np.zeros(30), None, np.zeros(10), np.zeros(10), want=("density",))


def test_work_without_a_device_is_refused():
    L = sctl_amd.lib()
    x = np.random.default_rng(0).random(30)
    f, w, g = np.ones(10), np.ones(10), np.zeros(30)
    rc_h = L.sctl_amd_eval_grad_host(0, 0, 10, 10, _p(x), _p(x + 1.0), None, _p(f), _p(w), _p(g), None, None, 1, -1, None, 0, 0)
    if sctl_amd.device_count() == 0:      # there is no CPU path
        assert rc_h == NO_DEVICE and b"no HIP device" in L.sctl_amd_last_error()
        assert L.sctl_amd_eval_grad_device(0, 0, 10, 10, _p(x), _p(x), None, _p(f), _p(w), _p(g), None, None, -1, None, 0, None) == NO_DEVICE
        assert L.sctl_amd_eval_grad_host(0, 0, 0, 10, None, _p(x), None, _p(f), None, None, _p(g), None, 1, -1, None, 0, 0) == NO_DEVICE   # as the forward entry: before the no-op
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no HIP device"):
            sctl_amd.eval_grad_host("Laplace3D-FxU", x, x, None, f, w)
        assert not g.any()
    else:
        assert rc_h == OK and g.all()


def test_planner_arithmetic():
    """The transposed plan's arithmetic (256 CUs when planning without a device, the MI355X's count) with the owner's output width: 3 sums per target,
    3 or, with a normal, 6 per source; one owner per lane on both sides of every kernel; the streamed range split in whole 256-record tiles."""
    P = sctl_amd.plan_grad
    if sctl_amd.device_count() > 0:
        import torch
        if torch.cuda.get_device_properties(0).multi_processor_count != 256:
            pytest.skip("the figures below are those of a 256-CU device")
    # 1000 targets x 300 sources: the targets' pass streams 2 tiles of sources, the sources' pass 4 tiles of targets, one per split
    assert P("Laplace3D-FxU", 0, 1000, 300) == dict(trg=dict(per_lane=1, splits=2, workspace_bytes=2 * 1000 * 3 * 8), src=dict(per_lane=1, splits=4, workspace_bytes=4 * 300 * 3 * 8))
    assert P("Laplace3D-DxU", 1, 1000, 300) == dict(trg=dict(per_lane=1, splits=2, workspace_bytes=2 * 1000 * 3 * 4), src=dict(per_lane=1, splits=4, workspace_bytes=4 * 300 * 6 * 4))
    assert P("Stokes3D-DxU", 0, 100, 200) == dict(trg=dict(per_lane=1, splits=1, workspace_bytes=0), src=dict(per_lane=1, splits=1, workspace_bytes=0))   # one tile: no partial sums
    assert P("Stokes3D-FxT", 1, 40000, 64)["src"] == dict(per_lane=1, splits=157, workspace_bytes=157 * 64 * 3 * 4)
    # 20000 owners, one per lane: 79 workgroups, ceil(1024 / 79) = 13 splits wanted, 118 tiles -> 10 per split -> 12 splits
    assert P("Laplace3D-DxU", 0, 30000, 20000)["src"] == dict(per_lane=1, splits=12, workspace_bytes=12 * 20000 * 6 * 8)
    assert P("Laplace3D-DxU", 0, 20000, 30000)["trg"] == dict(per_lane=1, splits=12, workspace_bytes=12 * 20000 * 3 * 8)
    # 2^18 x 2^18 (2^36 pairs), one owner per lane: 1024 workgroups, 2048 wanted -> 2; the 2 MB rule: sources {x, f} 8 MB -> 4 -> 8, targets {x, w} likewise
    assert P("Laplace3D-FxU", 0, 1 << 18, 1 << 18) == dict(trg=dict(per_lane=1, splits=8, workspace_bytes=8 * (1 << 18) * 24), src=dict(per_lane=1, splits=8, workspace_bytes=8 * (1 << 18) * 24))
    # the 2 GB bound at its real size: 2^22 x 2^22 stresslet, fp64.  Sources {x, n, f} 72 B x 2^22 = 288 MB -> 144 -> 64 splits (the cap): 64 * 2^22 * 24 B = 6 GB of
    # partial sums for the targets in one launch, so they go in launches of 2^31 / (64 * 24) = 1398101 -> whole workgroups of 256: 1398016; the splits stay 64.
    # The sources own 6 sums: 2^31 / (64 * 48) = 699050 -> 698880.
    pl = P("Stokes3D-DxU", 0, 1 << 22, 1 << 22)
    assert pl["trg"] == dict(per_lane=1, splits=64, workspace_bytes=64 * 1398016 * 24) and pl["trg"]["workspace_bytes"] <= 1 << 31
    assert pl["src"] == dict(per_lane=1, splits=64, workspace_bytes=64 * 698880 * 48) and pl["src"]["workspace_bytes"] <= 1 << 31
    for name in sctl_amd.KERNEL_NAMES:
        for real in (0, 1):
            for Nt, Ns in ((0, 0), (0, 10), (10, 0), (1, 1), (1 << 20, 1 << 20), (1 << 23, 1 << 14), (1 << 14, 1 << 23)):
                for side in P(name, real, Nt, Ns).values():
                    assert side["per_lane"] == 1 and 1 <= side["splits"] <= 1024 and 0 <= side["workspace_bytes"] <= 1 << 31, (name, real, Nt, Ns, side)


def test_workspace_bound_can_be_lowered_but_not_raised(monkeypatch):
    """the gradient plan shares the transposed plan's owner cut and its lowering variable (tests/test_gpu_grad.py runs the cut on small shapes)"""
    P = lambda: sctl_amd.plan_grad("Stokes3D-DxU", 0, 1 << 22, 1 << 22)
    for value, owners in (("1", (256, 256)), (str(64 * 48 * 1024), (2048, 1024)), (str(1 << 40), (1398016, 698880)), ("x", (1398016, 698880))):
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", value)
        pl = P()
        assert (pl["trg"]["workspace_bytes"], pl["src"]["workspace_bytes"]) == (64 * owners[0] * 24, 64 * owners[1] * 48), (value, pl)
    monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
    assert P()["trg"]["workspace_bytes"] == 64 * 1398016 * 24


def _unit_asm(args):
    unit, flags, out = args
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--offload-device-only", "-S", os.path.join(CSRC, "inst_g_%s.hip" % unit), "-o", out],
                   capture_output=True, check=True, timeout=1500)
    return out


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """device assembly of the ten inst_g_*.hip units with the Makefile's flags"""
    td = tmp_path_factory.mktemp("inst_g_asm")
    mk = lambda *a: subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()
    flags = mk("print-flags")
    jobs = [(u, flags + mk("print-unit-flags", "UNIT=inst_g_" + u), str(td / ("inst_g_%s.s" % u))) for u in UNITS]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(UNITS, ex.map(_unit_asm, jobs)))


def test_shipped_forms_have_no_scratch_and_two_waves_per_simd(unit_asm):
    """Every eval_grad_kernel<Ker, R, MODE, SIDE, T> the library launches, from its metadata (register counts and scratch size only): ScratchSize 0,
    at most 256 vector registers (512 per SIMD lane: two waves), and an LDS allocation of which two 256-lane workgroups fit a CU (160 KB).  Per
    kernel: fp64 modes 0-2 and fp32 modes 0-1, both sides, one owner per lane."""
    for unit, path in unit_asm.items():
        src = open(path).read()
        seen = set()
        for m in re.finditer(r"\.amdhsa_kernel (_ZN\w*eval_grad_kernelINS_\d+(\w+?)E([df])Li(\d)ELi(\d)ELi(\d)E\w*)\n(.*?)\.end_amdhsa_kernel", src, re.S):
            sym, ker, real, mode, side, T, meta = m.group(1), m.group(2), m.group(3), int(m.group(4)), int(m.group(5)), int(m.group(6)), m.group(7)
            assert ker == unit, (unit, sym)
            field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, meta).group(1))
            tail = src[src.index("\n" + sym + ":"):]
            scratch, vgprs = int(re.search(r"; ScratchSize: (\d+)", tail).group(1)), int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
            lds = field("group_segment_fixed_size")
            print("%-17s %s mode %d side %d T %d: %3d VGPRs, %5d B LDS, scratch %d" % (unit, real, mode, side, T, vgprs, lds, scratch))
            assert scratch == 0 and field("private_segment_fixed_size") == 0, sym
            assert 512 // vgprs >= 2, (sym, vgprs)
            assert (160 * 1024) // ((lds + 1279) // 1280 * 1280) >= 2, (sym, lds)
            seen.add((real, mode, side, T))
        assert seen == {(r, m, s, 1) for r, modes in (("d", (0, 1, 2)), ("f", (0, 1))) for m in modes for s in (0, 1)}, (unit, sorted(seen))
