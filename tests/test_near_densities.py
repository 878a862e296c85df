"""Several densities through the near field and ComputePotential (sctl_amd_near_apply_densities_*, sctl_amd_op_eval_potential_densities,
BoundaryIntegralOp::ComputePotentialDensities).  CPU: the symbols, the argument errors that can be had without a handle (a handle needs a
device: the checks that need one are in the GPU part), the device assembly of the several-densities kernels, the C++ driver.  GPU: the
reference's operator arrays and results of tests/golden/near_field.npz, and oracle.near_apply_restatement (pinned to the reference by
tests/test_near_field.py) for rows the reference did not compute."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, rel_l2
from test_near_field import CASES, IDS, dims, gold, matrix_free_part, near_inputs

OK, BAD = 0, -2
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
ARRS = ("elem_nds_cnt", "near_elem_cnt", "K_near_cnt", "K_near", "near_scatter_index", "near_trg_cnt", "near_trg_dsp")
NDS = (1, 2, 3, 5, 8, 9, 17)     # every pass width, a remainder, more than two passes


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_errors_without_a_handle():
    L = sctl_amd.lib()
    for name in ("sctl_amd_near_apply_densities_host", "sctl_amd_near_apply_densities_device", "sctl_amd_op_eval_potential_densities"):
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name)
    z = np.zeros(8)
    for nd in (-1, 0, 1, 2):
        assert L.sctl_amd_near_apply_densities_host(None, nd, _p(z), _p(z)) == BAD
        assert b"null near-field handle" in L.sctl_amd_last_error()
        assert L.sctl_amd_near_apply_densities_device(None, nd, _p(z), _p(z), None) == BAD
        assert L.sctl_amd_op_eval_potential_densities(None, nd, _p(z), _p(z), _p(z), 0, -1, None, 0) == BAD
        assert b"null handle" in L.sctl_amd_last_error()


def _near_asm(tmp_path):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    extra = subprocess.run(["make", "-s", "-C", CSRC, "print-unit-flags", "UNIT=near"], capture_output=True, text=True, check=True).stdout.split()
    out = str(tmp_path / "near.s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra + ["--offload-device-only", "-S", os.path.join(CSRC, "near.hip"), "-o", out],
                   capture_output=True, check=True, timeout=900)
    return open(out).read()


def test_several_densities_kernels_have_no_scratch_and_no_atomics(tmp_path):
    """near.hip with the Makefile's flags: forms of 2, 4 and 8 densities in both precisions, operator and accumulation kernel; none uses
    scratch memory or an atomic instruction, and the operator kernels keep at least 4 waves per SIMD (at most 128 vector registers: with 8
    row loads per lane that is 4 x 4 waves x 4 KB = 64 KB of K_near in flight per CU in fp64)."""
    src = _near_asm(tmp_path)
    seen = set()
    for m in re.finditer(r"^(_ZN\w*(near_gemm_kernel|near_accumulate_multi_kernel)I([df])Li(\d)E\w*):", src, re.M):
        sym, kind, real, M = m.group(1), m.group(2), m.group(3), int(m.group(4))
        body = src[m.end():src.index(".Lfunc_end", m.end())]
        meta = re.search(r"\.amdhsa_kernel " + sym + r"\n(.*?)\.end_amdhsa_kernel", src, re.S).group(1)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, sym
        assert int(re.search(r"; ScratchSize: (\d+)", src[m.end():]).group(1)) == 0, sym
        ops = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.strip() and l.strip()[0] not in ".;"]
        assert ops and not [o for o in ops if "atomic" in o or o.startswith(("scratch_", "ds_add", "ds_cmpst"))], sym
        if kind == "near_gemm_kernel":
            assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128, sym
            loads = [o for o in ops if o.startswith("global_load")]
            assert len(loads) == 32, (sym, len(loads))      # 8 rows x (whole groups, last rows) x (wide, narrow): every entry loaded once for the M densities
        seen.add((kind, real, M))
    assert seen == {(k, r, M) for k in ("near_gemm_kernel", "near_accumulate_multi_kernel") for r in "df" for M in (2, 4, 8)}


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    from test_cpp_host import _build
    exe = _build(tmp_path, "bie_densities_driver")          # -std=c++11 -Wall -Werror
    if sctl_amd.device_count() > 0:
        pytest.skip("a GPU is present: the no-device abort cannot be observed")
    p = subprocess.run([exe, "Laplace3D-FxU", "1", "50", "60", "4", "1", "0", "0", str(tmp_path / "o"), "0.2"], capture_output=True, text=True)
    assert p.returncode != 0
    assert "no HIP device" in p.stderr and "no CPU fallback" in p.stderr


def test_python_wrappers_check_shapes_before_the_library():
    class Fake(sctl_amd.NearOp):
        def __init__(self):
            self.dtype, self.density_len, self.potential_len, self._h = np.dtype(np.float64), 6, 4, None
    op = Fake()
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        op.apply_densities(np.zeros(6))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        op.apply_densities(np.zeros((2, 5)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="shape"):
        op.apply_densities(np.zeros((2, 6)), U=np.zeros((3, 4)))


def _rows(f, nd, rng):
    """rows: the golden density, -2 x it, then random rows"""
    F = rng.standard_normal((nd, f.size))
    F[0] = f
    if nd > 1:
        F[1] = -2 * f
    return F


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_near_densities_match_reference(O, oracle_mod, case):
    import torch
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    op = sctl_amd.NearOp(k0, k1, **arrs)
    op32 = sctl_amd.NearOp(k0, k1, **dict(arrs, K_near=arrs["K_near"].astype(np.float32)))
    ref_f = gold(case, "u_near") - matrix_free_part(O, case, arrs, xt, xnt, xs, xn, w, f)      # the REFERENCE's result for f
    rng = np.random.default_rng(case["seed"])
    Fall = _rows(f, max(NDS), rng)
    ref = np.stack([ref_f if m == 0 else -2 * ref_f if m == 1 else oracle_mod.near_apply_restatement(k0, k1, F=Fall[m], **arrs) for m in range(max(NDS))])
    single = op.apply(f)
    for nd in NDS:
        F = np.ascontiguousarray(Fall[:nd])
        U = op.apply_densities(F)
        assert U.shape == (nd, ref_f.size)
        errs = [rel_l2(U[m], ref[m]) for m in range(nd)]
        print("%s nd=%d fp64 rel-L2 per row: %s" % (case["key"], nd, " ".join("%.1e" % e for e in errs)))
        assert max(errs) < 1e-14, (nd, errs)
        if nd == 1:
            assert np.array_equal(U[0], single)                                   # nd == 1 IS the single-density entry
        assert np.array_equal(op.apply_densities(F), U)                           # bit-identical from run to run
        U0 = rng.standard_normal(U.shape)                                         # accumulation into a pre-filled U
        U2 = op.apply_densities(F, U=U0.copy())
        assert rel_l2(U2, U0 + ref[:nd]) < 1e-14
        Fd, Ud = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()          # the device entry adds on the device, the host entry on the host
        op.apply_densities_device(Fd, Ud)
        assert rel_l2(Ud.cpu().numpy(), U2) < 1e-14
        Uz = torch.zeros_like(Ud)
        op.apply_densities_device(Fd, Uz)
        assert np.array_equal(Uz.cpu().numpy(), U)                                # from zero: the same kernels, the same sums
        U32 = op32.apply_densities(F.astype(np.float32))
        errs32 = [rel_l2(U32[m].astype(np.float64), ref[m]) for m in range(nd)]
        print("%s nd=%d fp32 rel-L2 per row: %s" % (case["key"], nd, " ".join("%.1e" % e for e in errs32)))
        assert max(errs32) < 5e-6, (nd, errs32)
    op.close()
    op32.close()


@pytest.mark.gpu
def test_near_densities_large_random_operator(oracle_mod):
    """The operator of test_near_device_large_random_operator (wide blocks, blocks with fewer rows than a workgroup has waves, empty and
    matrix-free elements, targets without entries) at nd = 8 against the restatement."""
    rng = np.random.default_rng(17)
    nelem, ntrg, k0, k1 = 3000, 20000, 3, 3
    nds = rng.integers(0, 9, nelem)
    near = rng.integers(0, 120, nelem)
    near[::97] = 700
    kcnt = nds * near
    kcnt[5::11] = 0
    K = rng.standard_normal(int(kcnt.sum()) * k0 * k1)
    n_near = int(near.sum())
    trg_of_entry = rng.integers(0, ntrg // 2, n_near)
    order = np.argsort(trg_of_entry, kind="stable")
    cnt = np.bincount(trg_of_entry, minlength=ntrg)
    dsp = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    nd = 8
    F = rng.standard_normal((nd, int(nds.sum()) * k0))
    op = sctl_amd.NearOp(k0, k1, nds, near, K, order, cnt, dsp, K_near_cnt=kcnt)
    U = op.apply_densities(F)
    for m in range(nd):
        ref = oracle_mod.near_apply_restatement(k0, k1, nds, near, kcnt, K, order, cnt, dsp, F[m])
        assert rel_l2(U[m], ref) < 1e-14, (m, rel_l2(U[m], ref))
    assert np.all(U.reshape(nd, ntrg, k1)[:, ntrg // 2:] == 0)                    # untouched targets stay exactly 0 in every row
    assert np.array_equal(op.apply_densities(F[:3])[2], op.apply_densities(F[:4])[2])   # a partly filled pass computes the same sums
    op.close()


@pytest.mark.gpu
def test_near_densities_argument_errors_on_a_handle():
    """What needs a handle (and so a device): nd < 0 and null arrays are refused, nd == 0 does nothing."""
    L = sctl_amd.lib()
    op = sctl_amd.NearOp(1, 1, [2], [1], np.ones(2), [0], [1], [0])
    z = np.zeros(8)
    assert L.sctl_amd_near_apply_densities_host(op._h, -1, _p(z), _p(z)) == BAD and b"densities" in L.sctl_amd_last_error()
    assert L.sctl_amd_near_apply_densities_host(op._h, 2, None, _p(z)) == BAD
    assert L.sctl_amd_near_apply_densities_host(op._h, 2, _p(z), None) == BAD
    assert L.sctl_amd_near_apply_densities_device(op._h, -1, _p(z), _p(z), None) == BAD
    assert L.sctl_amd_near_apply_densities_device(op._h, 2, None, _p(z), None) == BAD
    assert L.sctl_amd_near_apply_densities_host(op._h, 0, None, None) == OK and not z.any()
    assert L.sctl_amd_near_apply_densities_device(op._h, 0, None, None, None) == OK
    U = op.apply_densities(np.array([[1.0, 2.0], [3.0, -1.0], [0.5, 0.5]]))
    assert np.array_equal(U, [[3.0], [2.0], [1.0]])
    d = sctl_amd.DirectOp("Laplace3D-FxU", np.float64)
    d.set_targets(np.zeros(3))
    d.set_sources(np.ones(3))
    assert L.sctl_amd_op_eval_potential_densities(d._h, -1, _p(z), _p(z), _p(z), 0, -1, None, 0) == BAD
    assert L.sctl_amd_op_eval_potential_densities(d._h, 2, _p(z), _p(z), _p(z), 0, -1, None, 0) == BAD and b"no near-field operator" in L.sctl_amd_last_error()
    d.set_near(1, [1], [1], np.ones(1), [0], [1], [0])
    assert L.sctl_amd_op_eval_potential_densities(d._h, 2, None, _p(z), _p(z), 0, -1, None, 0) == BAD
    assert L.sctl_amd_op_eval_potential_densities(d._h, 2, _p(z), None, _p(z), 0, -1, None, 0) == BAD
    assert L.sctl_amd_op_eval_potential_densities(d._h, 2, _p(z), _p(z), None, 0, -1, None, 0) == BAD
    assert L.sctl_amd_op_eval_potential_densities(d._h, 0, None, None, None, 0, -1, None, 0) == OK
    d.close()
    op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eval_potential_densities_on_the_operator_handle(O, case):
    """sctl_amd_op_eval_potential_densities on device lists (0,), (0,0), (0,0,0) (one GPU listed several times stands in for a multi-GPU
    node), fed with the REFERENCE's near-operator arrays: row f against the reference's ComputePotential, every row against the two legs."""
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    self_trg = case["Nt"] == 0
    T, Tn = (xs, xn) if self_trg else (xt, xnt)
    ups = case["upsample"]
    info = O.info(case["kernel"])
    x_far, n_far = np.repeat(xs.reshape(-1, 3), ups, 0).ravel(), np.repeat(xn.reshape(-1, 3), ups, 0).ravel()
    w_far = np.repeat(w / ups, ups)
    nd = 5
    F = _rows(f, nd, np.random.default_rng(case["seed"] + 1))
    F_far = np.stack([np.repeat(F[m].reshape(-1, k0), ups, 0).ravel() for m in range(nd)])
    expect = gold(case, "u_total") - matrix_free_part(O, case, arrs, xt, xnt, xs, xn, w, f)
    near_op = sctl_amd.NearOp(k0, k1, **arrs)
    first = None
    for devs in ((0,), (0, 0), (0, 0, 0)):
        op = sctl_amd.DirectOp(case["kernel"], np.float64, devices=devs)
        op.set_targets(T)
        op.set_sources(x_far, n_far if info["nd"] else None)
        op.set_source_weights(w_far)
        if case["trg_normal_dot_prod"]:
            op.set_target_normals(Tn)
        op.set_near(k1, arrs["elem_nds_cnt"], arrs["near_elem_cnt"], arrs["K_near"], arrs["near_scatter_index"], arrs["near_trg_cnt"], arrs["near_trg_dsp"],
                    K_near_cnt=arrs["K_near_cnt"])
        U = op.eval_potential_densities(F_far, F, digits=11)
        assert U.shape == (nd, expect.size)
        print("%s devices %s: row f vs reference %.2e, row -2f %.2e" % (case["key"], devs, rel_l2(U[0], expect), rel_l2(U[1], -2 * expect)))
        assert rel_l2(U[0], expect) < 1e-10 and rel_l2(U[1], -2 * expect) < 1e-10            # the reference's far field ran at tol 1e-10
        legs = near_op.apply_densities(F, U=op.eval_densities(F_far, digits=11))
        for m in range(nd):
            assert rel_l2(U[m], legs[m]) < 1e-14, (devs, m, rel_l2(U[m], legs[m]))
        if first is None:
            first = U
        assert rel_l2(U, first) < 1e-14                                                      # independent of the device list
        U2 = op.eval_potential_densities(F_far, F, V_trg=U.copy(), accumulate=True, digits=11)
        assert rel_l2(U2, 2 * U) < 1e-15
        one = op.eval_potential_densities(F_far[:1], F[:1], digits=11)                        # nd == 1 IS eval_potential
        assert np.array_equal(one[0], op.eval_potential(F_far[0], F[0], digits=11))
        op.set_targets(T)                                                                    # new targets drop the attached operator
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no near-field operator"):
            op.eval_potential_densities(F_far, F)
        op.close()
    near_op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compute_potential_densities_end_to_end(tmp_path, case):
    """BoundaryIntegralOp::ComputePotentialDensities (tests/cpp/bie_densities_driver.cpp) with rows {f, -2 f} against the REAL reference's
    ComputePotential; the driver itself asserts that one density gives ComputePotential's bits."""
    from test_cpp_host import _build, _read_vector
    exe = _build(tmp_path, "bie_densities_driver")
    out = str(tmp_path / (case["key"] + ".bin"))
    args = [exe, case["kernel"], str(case["seed"]), str(case["Nt"]), str(case["Ns"]), str(case["nodes_per_elem"]), str(case["upsample"]),
            str(case["trg_normal_dot_prod"]), str(int(case["Nt"] == 0)), out, repr(case["rad"]), str(case.get("free_nodes", 0))]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    u0, u1 = _read_vector(out + ".0"), _read_vector(out + ".1")
    assert rel_l2(u0, gold(case, "u_total")) < 1e-10, rel_l2(u0, gold(case, "u_total"))      # the reference's far field ran at tol 1e-10
    assert rel_l2(u1, -2 * gold(case, "u_total")) < 1e-10
