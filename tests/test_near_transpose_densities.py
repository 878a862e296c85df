"""Several weight vectors through the adjoint of the near field and of ComputePotential (sctl_amd_near_apply_transpose_densities_*,
sctl_amd_op_eval_transpose_densities, sctl_amd_op_eval_potential_transpose_densities, sctl_amd.autograd.near_apply_densities /
potential_densities).  Every row is checked against test_near_transpose.expected_transpose in long double at that module's bounds (1e-14 in
fp64, 5e-6 in fp32 rel-L2: its docstring derives them); the several-vectors kernels add the same terms in the same order in a lane and over
the same tree across lanes as the single-vector kernel.  Shipped forms: 2 and 4 vectors per pass in fp64, 2 in fp32, so nd runs over 1, 2, 3
(a partly filled 4; 2 + a single one left over), 4, 5 (4 + a single one), 7 (4 + a partly filled 4) and 9 (4 + 4 + a single one)."""
import ctypes
import os
import re

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, rel_l2
from test_near_densities import _near_asm
from test_near_field import CASES, IDS, dims, gold, near_inputs
from test_near_transpose import ARRS, TOL32, TOL64, expected_transpose

OK, BAD = 0, -2
NEW = ("sctl_amd_near_apply_transpose_densities_host", "sctl_amd_near_apply_transpose_densities_device", "sctl_amd_op_eval_transpose_densities",
       "sctl_amd_op_eval_potential_transpose_densities")
FORMS = {"d": (2, 4), "f": (2,)}     # vectors per pass of the shipped kernels: the fp32 form of 4 lost to four single calls and is not built
NDS = (1, 2, 3, 4, 5, 7, 9)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_list_and_library():
    header = open(os.path.join(ROOT, "include", "sctl_amd.h")).read()
    L = sctl_amd.lib()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in sctl_amd.api.SYMBOLS and getattr(L, name)


def test_null_handle_is_a_bad_argument():
    L = sctl_amd.lib()
    z = np.zeros(8)
    calls = [lambda: L.sctl_amd_near_apply_transpose_densities_host(None, 2, _p(z), _p(z)),
             lambda: L.sctl_amd_near_apply_transpose_densities_device(None, 2, _p(z), _p(z), None),
             lambda: L.sctl_amd_op_eval_transpose_densities(None, 2, _p(z), _p(z), 0, -1, None, 0),
             lambda: L.sctl_amd_op_eval_potential_transpose_densities(None, 2, _p(z), _p(z), _p(z), 0, -1, None, 0)]
    for call in calls:
        assert call() == BAD
        assert b"null" in L.sctl_amd_last_error()


def test_python_wrappers_check_shapes_before_the_library():
    class FakeNear(sctl_amd.NearOp):
        def __init__(self):
            self.dtype, self.density_len, self.potential_len, self._h = np.dtype(np.float64), 6, 4, None
    op = FakeNear()
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"weights must have shape \(nd, 4\)"):
        op.apply_transpose_densities(np.zeros((2, 6)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"weights must have shape \(nd, 4\)"):
        op.apply_transpose_densities(np.zeros(4))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="density gradients"):
        op.apply_transpose_densities(np.zeros((2, 4)), G=np.zeros((3, 6)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="density gradients"):
        op.apply_transpose_densities(np.zeros((2, 4)), G=np.zeros((2, 6), dtype=np.float32))
    import torch
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"shapes \(nd, 4\) and \(nd, 6\)"):
        op.apply_transpose_densities_device(torch.zeros((2, 5), dtype=torch.float64), torch.zeros((2, 6), dtype=torch.float64))
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"shapes \(nd, 4\) and \(nd, 6\)"):
        op.apply_transpose_densities_device(torch.zeros((2, 4), dtype=torch.float64), torch.zeros((3, 6), dtype=torch.float64))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="must be torch.float64 tensors"):
        op.apply_transpose_densities_device(torch.zeros((2, 4), dtype=torch.float32), torch.zeros((2, 6), dtype=torch.float64))

    class FakeOp(sctl_amd.DirectOp):
        def __init__(self):
            self.info, self.dtype, self.ctx = sctl_amd.api.kernel_info("Stokes3D-FxU"), np.dtype(np.float64), None
            self.Nt, self.Ns, self._h, self._near_len, self._near_k1 = 4, 5, None, 9, 3
    d = FakeOp()
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"W_trg must have shape \(nd, 12\)"):
        d.eval_transpose_densities(np.zeros((2, 4)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="G_src must be"):
        d.eval_transpose_densities(np.zeros((2, 12)), G_src=np.zeros((2, 14)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match=r"W_trg must have shape \(nd, 12\)"):
        d.eval_potential_transpose_densities(np.zeros(12))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="G_near must be"):
        d.eval_potential_transpose_densities(np.zeros((2, 12)), G_near=np.zeros((2, 8)))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="G_src_far must be"):
        d.eval_potential_transpose_densities(np.zeros((2, 12)), G_src_far=np.zeros((2, 15), dtype=np.float32))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="W_trg must be a contiguous float64"):
        d.eval_transpose_densities(np.zeros((2, 12), dtype=np.float32))


def test_several_vectors_kernels_isa(tmp_path):
    """near.hip with the Makefile's flags: every shipped form of near_gemm_t_kernel and near_gather_multi_kernel exists in both precisions, uses
    no scratch memory, no atomic and no LDS add / compare-and-store, at most 256 vector registers (2 waves per SIMD), and the operator kernel
    has the same number of non-temporal loads of K_near for every M: an entry is loaded once for all M vectors."""
    src = _near_asm(tmp_path)
    seen, k_loads = set(), {}
    for m in re.finditer(r"^(_ZN\w*(near_gemm_t_kernel|near_gather_multi_kernel)I([df])Li(\d+)E\w*):", src, re.M):
        sym, kind, real, M = m.group(1), m.group(2), m.group(3), int(m.group(4))
        body = src[m.end():src.index(".Lfunc_end", m.end())]
        meta = re.search(r"\.amdhsa_kernel " + sym + r"\n(.*?)\.end_amdhsa_kernel", src, re.S).group(1)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, sym
        assert int(re.search(r"; ScratchSize: (\d+)", src[m.end():]).group(1)) == 0, sym
        ops = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.strip() and l.strip()[0] not in ".;"]
        assert ops and not [o for o in ops if "atomic" in o or o.startswith(("scratch_", "ds_add", "ds_cmpst"))], sym
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
        print("%s<%s, %d>: %d VGPRs" % (kind, real, M, vgpr))
        assert vgpr <= 256, sym
        if kind == "near_gemm_t_kernel":
            k_loads[(real, M)] = len([l for l in body.split("\n") if re.match(r"\s+global_load_dword\w*\s", l) and l.rstrip().endswith(" nt")])
        seen.add((kind, real, M))
    assert seen == {(k, r, M) for k in ("near_gemm_t_kernel", "near_gather_multi_kernel") for r in "df" for M in FORMS[r]}
    print("non-temporal K_near loads:", k_loads)
    single = {}                                                                        # ... and the number of the single-vector kernel
    for m in re.finditer(r"^(_ZN\w*near_gemv_t_kernelI([df])E\w*):", src, re.M):
        body = src[m.end():src.index(".Lfunc_end", m.end())]
        single[m.group(2)] = len([l for l in body.split("\n") if re.match(r"\s+global_load_dword\w*\s", l) and l.rstrip().endswith(" nt")])
    assert min(k_loads.values()) > 0 and all(n == single[r] for (r, M), n in k_loads.items()), (k_loads, single)


def test_isa_rules_still_hold_with_the_new_kernels(tmp_path):
    """tools/check_isa_rules.py (the rules test_boundary.py holds every shipped unit to) over near.hip with the new kernels in it; and the exact
    sets of kernels that tests/test_near_transpose.py and tests/test_near_densities.py demand by name: the new names match neither expression."""
    import subprocess
    import sys
    for name in ("near_gemm_t_kernelIdLi4E", "near_gather_multi_kernelIfLi2E"):
        assert not re.search(r"(near_gemv_t_kernel|near_gather_kernel)I([df])E", name)
        assert not re.search(r"(near_gemm_kernel|near_accumulate_multi_kernel)I", name)
    _near_asm(tmp_path)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa_rules.py"), str(tmp_path / "near.s")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    import subprocess
    from test_cpp_host import _build
    exe = _build(tmp_path, "bie_transpose_densities_driver")          # -std=c++11 -Wall -Werror
    if sctl_amd.device_count() > 0:
        return                                                         # (the abort can only be observed without a device)
    p = subprocess.run([exe, "Laplace3D-FxU", "1", "50", "60", "4", "1", "0", "0", str(tmp_path / "o"), "3", "0.2"], capture_output=True, text=True)
    assert p.returncode != 0
    assert "no HIP device" in p.stderr and "no CPU fallback" in p.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _check_operator(arrs, k0, k1, rng, what, nds=NDS):
    """apply_transpose_densities in fp64 and fp32, every row against the long-double value; run-to-run bits, device == host, accumulation,
    untouched entries, nd == 1, a zero row, the forward untouched, growth of the gathered array, and the adjoint identity per row."""
    import torch
    op = sctl_amd.NearOp(k0, k1, **arrs)
    op32 = sctl_amd.NearOp(k0, k1, **dict(arrs, K_near=np.asarray(arrs["K_near"]).astype(np.float32)))
    nmax = max(nds)
    Wall = rng.standard_normal((nmax, op.potential_len))
    refs = [expected_transpose(k0, k1, W=Wall[m], **arrs) for m in range(nmax)]
    refs32 = [expected_transpose(k0, k1, W=Wall[m].astype(np.float32), **arrs)[0] for m in range(nmax)]
    ref, owned = np.array([r[0] for r in refs]), refs[0][1]
    f = rng.standard_normal(op.density_len)
    u_before = op.apply(f)
    singles = np.array([op.apply_transpose(Wall[m]) for m in range(nmax)])
    same_bits = True
    for nd in nds:                                                                     # ascending: 2 comes before 4 and grows the gathered array
        W = np.ascontiguousarray(Wall[:nd])
        G = op.apply_transpose_densities(W)
        G32 = op32.apply_transpose_densities(W.astype(np.float32))
        e64 = max(rel_l2(G[m], ref[m]) for m in range(nd))
        e32 = max(rel_l2(G32[m].astype(np.float64), refs32[m]) for m in range(nd))
        print("%s nd=%d: fp64 rel-L2 %.2e, fp32 rel-L2 %.2e" % (what, nd, e64, e32))
        assert e64 < TOL64, (nd, e64)
        assert e32 < TOL32, (nd, e32)
        assert np.all(G[:, ~owned] == 0)
        same_bits = same_bits and np.array_equal(G, singles[:nd])
        if nd == 1:
            assert np.array_equal(G[0], singles[0])                                    # nd == 1 is the single entry, bit for bit
        assert np.array_equal(op.apply_transpose_densities(W), G)                      # bit-identical from run to run
        Wd, Gd = torch.from_numpy(W).cuda(), torch.zeros(G.shape, dtype=torch.float64, device="cuda")
        op.apply_transpose_densities_device(Wd, Gd)
        assert np.array_equal(Gd.cpu().numpy(), G)                                     # device entry == host entry from zero, bit for bit
        G0 = rng.standard_normal(G.shape)                                              # accumulation into a pre-filled G, one row of W all zero
        Wz = W.copy()
        Wz[nd // 2] = 0
        G2 = op.apply_transpose_densities(Wz, G=G0.copy())
        for m in range(nd):
            if m == nd // 2:
                assert np.array_equal(G2[m], G0[m])                                    # rows do not leak into each other
            else:
                assert rel_l2(G2[m], G0[m] + ref[m]) < TOL64
        assert np.array_equal(G2[:, ~owned], G0[:, ~owned])                            # entries no block owns keep their exact bits
        Gd0 = torch.from_numpy(G0).cuda()
        op.apply_transpose_densities_device(torch.from_numpy(Wz).cuda(), Gd0)
        assert np.array_equal(Gd0.cpu().numpy(), G2)
        if nd > 1:                                                                     # <W[m], (N F)[m]> == <G[m], F[m]>, both sides from the device
            F = rng.standard_normal((nd, op.density_len))
            U = op.apply_densities(F)
            for m in range(nd):
                a, b = W[m] * U[m], G[m] * F[m]
                assert abs(a.sum() - b.sum()) <= 1e-13 * (np.abs(a).sum() + np.abs(b).sum()), (nd, m)
    print("%s: rows of a several-vectors call equal the single calls bit for bit: %s" % (what, same_bits))
    assert np.array_equal(op.apply(f), u_before)                                       # the forward is untouched by transposed calls in between
    fresh = sctl_amd.NearOp(k0, k1, **arrs)                                            # 2 first, then the widest form, on a new handle
    W = np.ascontiguousarray(Wall[:max(FORMS["d"])])
    g2 = fresh.apply_transpose_densities(W[:2])
    g4 = fresh.apply_transpose_densities(W)
    assert np.array_equal(g2, g4[:2]) and max(rel_l2(g4[m], ref[m]) for m in range(W.shape[0])) < TOL64
    g2b = fresh.apply_transpose_densities(W[:2])                                       # ... and the narrow form on the grown array
    assert np.array_equal(g2b, g2)
    fresh.close()
    op.close()
    op32.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_near_transpose_densities_match_long_double(O, case):
    k0, k1 = dims(O, case)
    arrs = {k: gold(case, k) for k in ARRS}
    _check_operator(arrs, k0, k1, np.random.default_rng(case["seed"]), case["key"])


@pytest.mark.gpu
def test_near_transpose_densities_large_random_operator():
    """The operator of test_near_transpose_large_random_operator: blocks up to 24 x 2100, empty rows and columns, matrix-free elements,
    targets without entries."""
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
    arrs = dict(elem_nds_cnt=nds, near_elem_cnt=near, K_near_cnt=kcnt, K_near=K, near_scatter_index=order, near_trg_cnt=cnt, near_trg_dsp=dsp)
    _check_operator(arrs, k0, k1, rng, "large random")


@pytest.mark.gpu
def test_near_transpose_densities_boundary_shapes():
    """The operator of test_near_transpose_boundary_shapes: one element per pair of sd and td at the borders of the kernel's paths."""
    rng = np.random.default_rng(5)
    shapes = [(sd, td) for sd in (1, 3, 4, 5, 9, 144) for td in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025)]
    nds, near = np.array([s for s, _ in shapes]), np.array([t for _, t in shapes])
    K = rng.standard_normal(int((nds * near).sum()))
    n_near = int(near.sum())
    cnt = []
    while sum(cnt) < n_near:
        cnt.append(min(int(rng.integers(1, 4)), n_near - sum(cnt)))                   # every target has 1 to 3 entries
    cnt = np.array(cnt)
    dsp = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    arrs = dict(elem_nds_cnt=nds, near_elem_cnt=near, K_near_cnt=None, K_near=K, near_scatter_index=rng.permutation(n_near), near_trg_cnt=cnt, near_trg_dsp=dsp)
    _check_operator(arrs, 1, 1, rng, "boundary shapes")


@pytest.mark.gpu
def test_near_transpose_densities_argument_errors_on_a_handle():
    L = sctl_amd.lib()
    op = sctl_amd.NearOp(1, 1, [2], [1], np.ones(2), [0], [1], [0])
    z, g = np.ones(8), np.full(8, 7.0)
    assert L.sctl_amd_near_apply_transpose_densities_host(op._h, -1, _p(z), _p(g)) == BAD and b"negative" in L.sctl_amd_last_error()
    assert L.sctl_amd_near_apply_transpose_densities_device(op._h, -1, _p(z), _p(g), None) == BAD
    assert L.sctl_amd_near_apply_transpose_densities_host(op._h, 0, _p(z), _p(g)) == OK and np.all(g == 7.0)
    assert L.sctl_amd_near_apply_transpose_densities_host(op._h, 0, None, None) == OK
    assert L.sctl_amd_near_apply_transpose_densities_host(op._h, 2, None, _p(g)) == BAD and b"null" in L.sctl_amd_last_error()
    assert L.sctl_amd_near_apply_transpose_densities_host(op._h, 2, _p(z), None) == BAD
    assert L.sctl_amd_near_apply_transpose_densities_device(op._h, 2, None, _p(g), None) == BAD
    assert np.array_equal(op.apply_transpose_densities(np.array([[3.0], [5.0]])), [[3.0, 3.0], [5.0, 5.0]])
    op.close()
    empty = sctl_amd.NearOp(1, 1, [2], [1], np.zeros(0), [0], [1], [0], K_near_cnt=[0])       # no entries: OK, nothing touched
    g = np.array([[1.5, -2.5], [-0.0, 4.0]])
    out = empty.apply_transpose_densities(np.array([[3.0], [4.0]]), G=g.copy())
    assert np.array_equal(out, g) and np.array_equal(np.signbit(out), np.signbit(g))
    empty.close()


def _expand(w, n_trg, k1):
    """w_full[t][k*3+l] = w[t][k] n_trg[t][l]"""
    return (w.reshape(-1, k1, 1) * n_trg.reshape(-1, 1, 3)).ravel()


def _operator_case(O, case, nd):
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    T, Tn = (xs, xn) if case["Nt"] == 0 else (xt, xnt)
    ups = case["upsample"]
    info = O.info(case["kernel"])
    x_far, n_far = np.repeat(xs.reshape(-1, 3), ups, 0).ravel(), np.repeat(xn.reshape(-1, 3), ups, 0).ravel()
    w_far = np.repeat(w / ups, ups)
    rng = np.random.default_rng(case["seed"] + 5)
    Wt = rng.standard_normal((nd, T.size // 3 * k1))
    F = rng.standard_normal((nd, f.size))
    F_far = np.array([np.repeat(F[m].reshape(-1, k0), ups, 0).ravel() for m in range(nd)])
    far_ref = np.array([np.repeat(w_far, k0) * sctl_amd.api.eval_transpose_host(case["kernel"], T, x_far, n_far if info["nd"] else None,
                                                                                _expand(Wt[m], Tn, k1) if case["trg_normal_dot_prod"] else Wt[m])
                        for m in range(nd)])
    first = None
    for devs in ((0,), (0, 0), (0, 0, 0)):
        op = sctl_amd.DirectOp(case["kernel"], np.float64, devices=devs)
        op.set_targets(T)
        op.set_sources(x_far, n_far if info["nd"] else None)
        op.set_source_weights(w_far)
        if case["trg_normal_dot_prod"]:
            op.set_target_normals(Tn)
        G_only = op.eval_transpose_densities(Wt)
        for m in range(nd):
            assert rel_l2(G_only[m], far_ref[m]) < 1e-12, (devs, m, rel_l2(G_only[m], far_ref[m]))
            assert rel_l2(G_only[m], op.eval_transpose(Wt[m])) < 1e-14
        op.set_near(k1, arrs["elem_nds_cnt"], arrs["near_elem_cnt"], arrs["K_near"], arrs["near_scatter_index"], arrs["near_trg_cnt"], arrs["near_trg_dsp"],
                    K_near_cnt=arrs["K_near_cnt"])
        pairs0 = sctl_amd.api.counters()["pair_interactions"]
        G_far, G_near = op.eval_potential_transpose_densities(Wt)
        assert sctl_amd.api.counters()["pair_interactions"] - pairs0 == nd * (T.size // 3) * (x_far.size // 3)
        for m in range(nd):
            g_far, g_near = op.eval_potential_transpose(Wt[m])
            assert rel_l2(G_far[m], far_ref[m]) < 1e-12
            assert rel_l2(G_far[m], g_far) < 1e-14 and rel_l2(G_near[m], g_near) < 1e-14, (devs, m, rel_l2(G_far[m], g_far), rel_l2(G_near[m], g_near))
        if first is None:
            first = (G_far, G_near)
        for m in range(nd):                                                               # the device lists agree to rounding
            assert rel_l2(G_far[m], first[0][m]) < 1e-14 and rel_l2(G_near[m], first[1][m]) < 1e-14
        U = op.eval_potential_densities(F_far, F, digits=-1)                              # <W[m], P(F_far, F)[m]> == <G_far[m], F_far[m]> + <G_near[m], F[m]>
        for m in range(nd):
            a, b = Wt[m] * U[m], np.concatenate([G_far[m] * F_far[m], G_near[m] * F[m]])
            assert abs(a.sum() - b.sum()) <= 1e-12 * (np.abs(a).sum() + np.abs(b).sum()), (devs, m, a.sum(), b.sum())
        H_far, H_near = op.eval_potential_transpose_densities(Wt, G_src_far=G_far.copy(), G_near=G_near.copy(), accumulate=True)
        for m in range(nd):
            assert rel_l2(H_far[m], 2 * G_far[m]) < 1e-15 and rel_l2(H_near[m], 2 * G_near[m]) < 1e-15
        op.set_targets(T)                                                                 # new targets drop the attached operator
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no near-field operator"):
            op.eval_potential_transpose_densities(Wt)
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eval_potential_transpose_densities_on_the_operator_handle(O, case):
    _operator_case(O, case, 3)


@pytest.mark.gpu
def test_operator_handle_with_target_normals_and_the_traction_kernel(O):
    """One case with target normals, and Stokes3D-FxT (its widest far form is 4) at nd = 5."""
    dotted = next(c for c in CASES if c["trg_normal_dot_prod"])
    _operator_case(O, dotted, 3)
    fxt = [c for c in CASES if c["kernel"] == "Stokes3D-FxT"]
    assert fxt, "no golden case with Stokes3D-FxT"
    _operator_case(O, fxt[0], 5)


@pytest.mark.gpu
def test_op_transpose_densities_argument_errors_on_a_handle():
    L = sctl_amd.lib()
    z, g = np.ones(32), np.full(32, 7.0)
    d = sctl_amd.DirectOp("Laplace3D-FxU", np.float64)
    d.set_targets(np.arange(6.0))
    d.set_sources(np.arange(9.0) + 10)
    assert L.sctl_amd_op_eval_transpose_densities(d._h, -1, _p(z), _p(g), 0, -1, None, 0) == BAD and b"negative" in L.sctl_amd_last_error()
    assert L.sctl_amd_op_eval_transpose_densities(d._h, 0, None, None, 0, -1, None, 0) == OK
    assert L.sctl_amd_op_eval_transpose_densities(d._h, 0, _p(z), _p(g), 0, -1, None, 0) == OK and np.all(g == 7.0)
    assert L.sctl_amd_op_eval_transpose_densities(d._h, 2, None, _p(g), 0, -1, None, 0) == BAD and b"null" in L.sctl_amd_last_error()
    assert L.sctl_amd_op_eval_potential_transpose_densities(d._h, 2, _p(z), _p(g), _p(g), 0, -1, None, 0) == BAD and b"no near-field operator" in L.sctl_amd_last_error()
    w = np.arange(4.0).reshape(2, 2) + 1
    assert np.array_equal(d.eval_transpose_densities(w[:1])[0], d.eval_transpose(w[0]))      # nd == 1 is the single entry
    d.close()


@pytest.mark.gpu
def test_op_transpose_densities_refuse_a_plugin_kernel_without_pair_t(tmp_path_factory):
    from test_gpu_transpose import LAM, _ensure
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    d = sctl_amd.DirectOp(name, np.float64, ctx=np.array([LAM]))
    d.set_targets(np.arange(6.0))
    d.set_sources(np.arange(9.0) + 10)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        d.eval_transpose_densities(np.ones((2, 2)))
    d.close()


@pytest.mark.gpu
def test_autograd_through_several_densities(O):
    import torch
    from sctl_amd import autograd
    case = next(c for c in CASES if c["key"] == "c3")
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    near_op = sctl_amd.NearOp(k0, k1, **arrs)
    rng = np.random.default_rng(3)
    nd = 3
    Wt = rng.standard_normal((nd, near_op.potential_len))
    F = rng.standard_normal((nd, f.size))
    Fd = torch.from_numpy(F).cuda().requires_grad_(True)
    U = autograd.near_apply_densities(near_op, Fd)
    assert np.array_equal(U.detach().cpu().numpy(), near_op.apply_densities(F))
    (U * torch.from_numpy(Wt).cuda()).sum().backward()
    expect = near_op.apply_transpose_densities_device(torch.from_numpy(Wt).cuda(), torch.zeros(F.shape, dtype=torch.float64, device="cuda"))
    assert np.array_equal(Fd.grad.cpu().numpy(), expect.cpu().numpy())
    T, Tn = (xs, xn) if case["Nt"] == 0 else (xt, xnt)
    ups = case["upsample"]
    info = O.info(case["kernel"])
    x_far, n_far = np.repeat(xs.reshape(-1, 3), ups, 0).ravel(), np.repeat(xn.reshape(-1, 3), ups, 0).ravel()
    op = sctl_amd.DirectOp(case["kernel"], np.float64)
    op.set_targets(T)
    op.set_sources(x_far, n_far if info["nd"] else None)
    op.set_source_weights(np.repeat(w / ups, ups))
    if case["trg_normal_dot_prod"]:
        op.set_target_normals(Tn)
    op.set_near(k1, arrs["elem_nds_cnt"], arrs["near_elem_cnt"], arrs["K_near"], arrs["near_scatter_index"], arrs["near_trg_cnt"], arrs["near_trg_dsp"],
                K_near_cnt=arrs["K_near_cnt"])
    F_far = torch.from_numpy(np.array([np.repeat(F[m].reshape(-1, k0), ups, 0).ravel() for m in range(nd)])).requires_grad_(True)
    F_near = torch.from_numpy(F.copy()).requires_grad_(True)
    U = autograd.potential_densities(op, F_far, F_near)
    assert np.array_equal(U.detach().numpy(), op.eval_potential_densities(F_far.detach().numpy(), F))
    (U * torch.from_numpy(Wt)).sum().backward()
    G_far, G_near = op.eval_potential_transpose_densities(Wt)
    assert np.array_equal(F_far.grad.numpy(), G_far) and np.array_equal(F_near.grad.numpy(), G_near)
    op.close()
    near_op.close()


DRIVER_CASES = [c for c in CASES if c["key"] in ("c0", "c3", "c5", "c6")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DRIVER_CASES, ids=[c["key"] for c in DRIVER_CASES])
def test_compute_potential_transpose_densities_end_to_end(tmp_path, case):
    """BoundaryIntegralOp::ComputePotentialTransposeDensities (tests/cpp/bie_transpose_densities_driver.cpp), nd = 3: per row
    <W, ComputePotentialDensities(F)> against <ComputePotentialTransposeDensities(W), F> to 1e-13 of the sum of the terms' magnitudes, and
    the row against ComputePotentialTranspose of that row to 1e-14."""
    import subprocess
    from test_cpp_host import _build, _read_vector
    exe = _build(tmp_path, "bie_transpose_densities_driver")
    out = str(tmp_path / (case["key"] + ".bin"))
    nd = 3
    args = [exe, case["kernel"], str(case["seed"]), str(case["Nt"]), str(case["Ns"]), str(case["nodes_per_elem"]), str(case["upsample"]),
            str(case["trg_normal_dot_prod"]), str(int(case["Nt"] == 0)), out, str(nd), repr(case["rad"]), str(case.get("free_nodes", 0))]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    G, ip = _read_vector(out), _read_vector(out + ".ip").reshape(nd, 5)
    k0, _ = dims(__import__("oracle").restatement(), case)
    assert G.size == nd * case["Ns"] * k0 and np.all(np.isfinite(G))
    for m in range(nd):
        print("%s row %d: <W, P F> = %.15e, <P^T W, F> = %.15e, difference %.2e of the sum of |terms|, row vs single %.2e"
              % (case["key"], m, ip[m, 0], ip[m, 1], abs(ip[m, 0] - ip[m, 1]) / (ip[m, 2] + ip[m, 3]), ip[m, 4]))
        assert abs(ip[m, 0] - ip[m, 1]) <= 1e-13 * (ip[m, 2] + ip[m, 3])
        assert ip[m, 4] < 1e-14
