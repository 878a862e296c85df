"""The adjoint of the near field and of ComputePotential (sctl_amd_near_apply_transpose_*, sctl_amd_op_eval_transpose,
sctl_amd_op_eval_potential_transpose, sctl_amd.autograd.near_apply / potential).  The expected value of G = N^T W is built here from the
operator arrays: per element B_e @ Wn_e in numpy long double, Wn gathered through near_scatter_index, near_trg_cnt and near_trg_dsp.  A
plain fp64 numpy evaluation lies within 3.5e-16 rel-L2 of that value and an fp32 one within 1.5e-7, so the bounds of the forward near
tests carry over with more than 25x margin: 1e-14 in fp64, 5e-6 in fp32."""
import ctypes
import os
import re

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, rel_l2
from test_near_densities import _near_asm
from test_near_field import CASES, IDS, dims, gold, near_inputs

OK, BAD = 0, -2
ARRS = ("elem_nds_cnt", "near_elem_cnt", "K_near_cnt", "K_near", "near_scatter_index", "near_trg_cnt", "near_trg_dsp")
NEW = ("sctl_amd_near_apply_transpose_host", "sctl_amd_near_apply_transpose_device", "sctl_amd_op_eval_transpose", "sctl_amd_op_eval_potential_transpose")
TOL64, TOL32 = 1e-14, 5e-6


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def expected_transpose(k0, k1, elem_nds_cnt, near_elem_cnt, K_near_cnt, K_near, near_scatter_index, near_trg_cnt, near_trg_dsp, W):
    """(G, owned): G = N^T W in long double; owned[j] is False for the density entries of elements without a matrix or without near targets."""
    ld = np.longdouble
    nds, near, cnt, dsp = (np.asarray(a, dtype=np.int64) for a in (elem_nds_cnt, near_elem_cnt, near_trg_cnt, near_trg_dsp))
    kcnt = nds * near if K_near_cnt is None else np.asarray(K_near_cnt, dtype=np.int64)
    ntrg, n_near = cnt.size, int(near.sum())
    p = np.repeat(dsp, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)      # the entries of target i: dsp[i] .. dsp[i] + cnt[i]
    Wn = np.zeros((n_near, k1), dtype=ld)
    Wn[np.asarray(near_scatter_index, dtype=np.int64)[p]] = np.asarray(W, dtype=ld).reshape(ntrg, k1)[np.repeat(np.arange(ntrg), cnt)]
    Wn = Wn.ravel()
    G, owned = np.zeros(int(nds.sum()) * k0, dtype=ld), np.zeros(int(nds.sum()) * k0, dtype=bool)
    K = np.asarray(K_near)
    f_off = u_off = k_off = 0
    for e in range(nds.size):
        sd, td = int(nds[e]) * k0, int(near[e]) * k1
        if kcnt[e] and sd and td:
            G[f_off:f_off + sd] = K[k_off:k_off + sd * td].reshape(sd, td).astype(ld) @ Wn[u_off:u_off + td]
            owned[f_off:f_off + sd] = True
            k_off += sd * td
        f_off += sd
        u_off += td
    return G, owned


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
    calls = [lambda: L.sctl_amd_near_apply_transpose_host(None, _p(z), _p(z)), lambda: L.sctl_amd_near_apply_transpose_device(None, _p(z), _p(z), None),
             lambda: L.sctl_amd_op_eval_transpose(None, _p(z), _p(z), 0, -1, None, 0),
             lambda: L.sctl_amd_op_eval_potential_transpose(None, _p(z), _p(z), _p(z), 0, -1, None, 0)]
    for call in calls:
        assert call() == BAD
        assert b"null" in L.sctl_amd_last_error()


def test_transposed_kernels_have_no_scratch_and_no_atomics(tmp_path):
    """near.hip with the Makefile's flags: the transposed operator kernel and the gather exist in both precisions, use no scratch memory, no
    atomic and no LDS add / compare-and-store, and keep at least 4 waves per SIMD (at most 128 vector registers)."""
    src = _near_asm(tmp_path)
    seen = set()
    for m in re.finditer(r"^(_ZN\w*(near_gemv_t_kernel|near_gather_kernel)I([df])E\w*):", src, re.M):
        sym, kind, real = m.group(1), m.group(2), m.group(3)
        body = src[m.end():src.index(".Lfunc_end", m.end())]
        meta = re.search(r"\.amdhsa_kernel " + sym + r"\n(.*?)\.end_amdhsa_kernel", src, re.S).group(1)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, sym
        assert int(re.search(r"; ScratchSize: (\d+)", src[m.end():]).group(1)) == 0, sym
        ops = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.strip() and l.strip()[0] not in ".;"]
        assert ops and not [o for o in ops if "atomic" in o or o.startswith(("scratch_", "ds_add", "ds_cmpst"))], sym
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128, sym
        seen.add((kind, real))
    assert seen == {(k, r) for k in ("near_gemv_t_kernel", "near_gather_kernel") for r in "df"}


def test_python_wrappers_check_shapes_before_the_library():
    class FakeNear(sctl_amd.NearOp):
        def __init__(self):
            self.dtype, self.density_len, self.potential_len, self._h = np.dtype(np.float64), 6, 4, None
    op = FakeNear()
    with pytest.raises(sctl_amd.api.SctlAmdError, match="weights must hold 4"):
        op.apply_transpose(np.zeros(6))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="density gradient"):
        op.apply_transpose(np.zeros(4), G=np.zeros(5))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="density gradient"):
        op.apply_transpose(np.zeros(4), G=np.zeros(6, dtype=np.float32))
    import torch
    with pytest.raises(sctl_amd.api.SctlAmdError, match="must hold 4 and 6"):
        op.apply_transpose_device(torch.zeros(5, dtype=torch.float64), torch.zeros(6, dtype=torch.float64))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="must hold 4 and 6"):
        op.apply_transpose_device(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))

    class FakeOp(sctl_amd.DirectOp):
        def __init__(self):
            self.info, self.dtype, self.ctx = sctl_amd.api.kernel_info("Stokes3D-FxU"), np.dtype(np.float64), None
            self.Nt, self.Ns, self._h, self._near_len, self._near_k1 = 4, 5, None, 9, 3
    d = FakeOp()
    with pytest.raises(sctl_amd.api.SctlAmdError, match="w_trg must hold 12"):
        d.eval_transpose(np.zeros(4))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="g_src must be"):
        d.eval_transpose(np.zeros(12), g_src=np.zeros(14))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="w_trg must hold 12"):
        d.eval_potential_transpose(np.zeros(5))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="g_near must be"):
        d.eval_potential_transpose(np.zeros(12), g_near=np.zeros(8))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="g_src_far must be"):
        d.eval_potential_transpose(np.zeros(12), g_src_far=np.zeros(15, dtype=np.float32))


def test_cpp_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    import subprocess
    from test_cpp_host import _build
    exe = _build(tmp_path, "bie_transpose_driver")          # -std=c++11 -Wall -Werror
    if sctl_amd.device_count() > 0:
        pytest.skip("a GPU is present: the no-device abort cannot be observed")
    p = subprocess.run([exe, "Laplace3D-FxU", "1", "50", "60", "4", "1", "0", "0", str(tmp_path / "o"), "0.2"], capture_output=True, text=True)
    assert p.returncode != 0
    assert "no HIP device" in p.stderr and "no CPU fallback" in p.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _check_operator(arrs, k0, k1, rng, what, free_entries=None):
    """apply_transpose in fp64 and fp32 against the long-double value, accumulation, device == host from zero, run-to-run bits, untouched
    entries, and the adjoint identity against the forward application."""
    import torch
    op = sctl_amd.NearOp(k0, k1, **arrs)
    op32 = sctl_amd.NearOp(k0, k1, **dict(arrs, K_near=np.asarray(arrs["K_near"]).astype(np.float32)))
    W = rng.standard_normal(op.potential_len)
    ref, owned = expected_transpose(k0, k1, W=W, **arrs)
    if free_entries is not None:
        assert int((~owned).sum()) == free_entries
    G = op.apply_transpose(W)
    e64 = rel_l2(G, ref)
    G32 = op32.apply_transpose(W.astype(np.float32))
    e32 = rel_l2(G32.astype(np.float64), expected_transpose(k0, k1, W=W.astype(np.float32), **arrs)[0])
    print("%s: fp64 rel-L2 %.2e, fp32 rel-L2 %.2e" % (what, e64, e32))
    assert e64 < TOL64, e64
    assert e32 < TOL32, e32
    assert np.all(G[~owned] == 0)
    assert np.array_equal(op.apply_transpose(W), G)                                   # bit-identical from run to run
    G0 = rng.standard_normal(G.size)                                                  # accumulation into a pre-filled G
    G2 = op.apply_transpose(W, G=G0.copy())
    assert rel_l2(G2, G0 + ref) < TOL64
    assert np.array_equal(G2[~owned], G0[~owned])                                     # entries no block owns keep their exact bits
    Wd, Gd = torch.from_numpy(W).cuda(), torch.zeros(G.size, dtype=torch.float64, device="cuda")
    op.apply_transpose_device(Wd, Gd)
    assert np.array_equal(Gd.cpu().numpy(), G)                                        # device entry == host entry from zero, bit for bit
    Gd0 = torch.from_numpy(G0).cuda()
    op.apply_transpose_device(Wd, Gd0)
    assert rel_l2(Gd0.cpu().numpy(), G0 + ref) < TOL64
    assert np.array_equal(Gd0.cpu().numpy()[~owned], G0[~owned])
    f = rng.standard_normal(op.density_len)                                           # <w, N f> == <N^T w, f>, both sides from the device
    a, b = W * op.apply(f), G * f
    print("%s: adjoint identity %.2e of the sum of |terms|" % (what, abs(a.sum() - b.sum()) / (np.abs(a).sum() + np.abs(b).sum())))
    assert abs(a.sum() - b.sum()) <= 1e-13 * (np.abs(a).sum() + np.abs(b).sum())
    assert np.array_equal(op.apply(f), op.apply(f))                                   # the forward is untouched by transposed calls in between
    op.close()
    op32.close()


FREE = {"t0": 90, "t1": 183, "t2": 50}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_near_transpose_matches_long_double(O, case):
    k0, k1 = dims(O, case)
    arrs = {k: gold(case, k) for k in ARRS}
    _check_operator(arrs, k0, k1, np.random.default_rng(case["seed"]), case["key"], free_entries=FREE.get(case["key"], 0))


@pytest.mark.gpu
def test_near_transpose_large_random_operator():
    """The operator of test_near_densities_large_random_operator: blocks up to 24 x 2100, empty rows and columns, matrix-free elements,
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
def test_near_transpose_boundary_shapes():
    """One element per pair of sd and td at the borders of the kernel's paths: rows packed into a wave (td < 64), the lane tail, rows cut over
    the waves of a workgroup (td >= 1024), blocks with fewer rows than loads in flight."""
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
def test_near_transpose_argument_errors_on_a_handle():
    L = sctl_amd.lib()
    op = sctl_amd.NearOp(1, 1, [2], [1], np.ones(2), [0], [1], [0])
    z = np.zeros(8)
    assert L.sctl_amd_near_apply_transpose_host(op._h, None, _p(z)) == BAD and b"null" in L.sctl_amd_last_error()
    assert L.sctl_amd_near_apply_transpose_host(op._h, _p(z), None) == BAD
    assert L.sctl_amd_near_apply_transpose_device(op._h, None, _p(z), None) == BAD
    assert np.array_equal(op.apply_transpose(np.array([3.0])), [3.0, 3.0])
    op.close()
    empty = sctl_amd.NearOp(1, 1, [2], [1], np.zeros(0), [0], [1], [0], K_near_cnt=[0])       # no entries: OK, nothing touched
    g = np.array([1.5, -2.5])
    assert np.array_equal(empty.apply_transpose(np.array([3.0]), G=g), [1.5, -2.5])
    empty.close()


def _expand(w, n_trg, k1):
    """w_full[t][k*3+l] = w[t][k] n_trg[t][l]"""
    return (w.reshape(-1, k1, 1) * n_trg.reshape(-1, 1, 3)).ravel()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eval_potential_transpose_on_the_operator_handle(O, case):
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    self_trg = case["Nt"] == 0
    T, Tn = (xs, xn) if self_trg else (xt, xnt)
    ups = case["upsample"]
    info = O.info(case["kernel"])
    x_far, n_far = np.repeat(xs.reshape(-1, 3), ups, 0).ravel(), np.repeat(xn.reshape(-1, 3), ups, 0).ravel()
    w_far, f_far = np.repeat(w / ups, ups), np.repeat(f.reshape(-1, k0), ups, 0).ravel()
    rng = np.random.default_rng(case["seed"] + 2)
    wt = rng.standard_normal(T.size // 3 * k1)
    w_full = _expand(wt, Tn, k1) if case["trg_normal_dot_prod"] else wt
    far_ref = np.repeat(w_far, k0) * sctl_amd.api.eval_transpose_host(case["kernel"], T, x_far, n_far if info["nd"] else None, w_full)
    near_op = sctl_amd.NearOp(k0, k1, **arrs)
    near_ref = near_op.apply_transpose(wt)
    near_op.close()
    first = None
    for devs in ((0,), (0, 0), (0, 0, 0)):
        op = sctl_amd.DirectOp(case["kernel"], np.float64, devices=devs)
        op.set_targets(T)
        op.set_sources(x_far, n_far if info["nd"] else None)
        op.set_source_weights(w_far)
        if case["trg_normal_dot_prod"]:
            op.set_target_normals(Tn)
        g_only = op.eval_transpose(wt)
        assert rel_l2(g_only, far_ref) < 1e-12, (devs, rel_l2(g_only, far_ref))
        op.set_near(k1, arrs["elem_nds_cnt"], arrs["near_elem_cnt"], arrs["K_near"], arrs["near_scatter_index"], arrs["near_trg_cnt"], arrs["near_trg_dsp"],
                    K_near_cnt=arrs["K_near_cnt"])
        pairs0 = sctl_amd.api.counters()["pair_interactions"]
        g_far, g_near = op.eval_potential_transpose(wt)
        assert sctl_amd.api.counters()["pair_interactions"] - pairs0 == (T.size // 3) * (x_far.size // 3)
        print("%s devices %s: far leg %.2e, far vs eval_transpose %.2e, near leg %.2e" % (case["key"], devs, rel_l2(g_far, far_ref), rel_l2(g_far, g_only),
                                                                                          rel_l2(g_near, near_ref)))
        assert rel_l2(g_far, far_ref) < 1e-12
        assert rel_l2(g_far, g_only) < 1e-14 and rel_l2(g_near, near_ref) < 1e-14
        if first is None:
            first = (g_far, g_near)
        assert rel_l2(g_far, first[0]) < 1e-14 and rel_l2(g_near, first[1]) < 1e-14      # the device lists agree to rounding
        a = wt * op.eval_potential(f_far, f, digits=-1)                                   # <w, P(f_far, f)> == <g_far, f_far> + <g_near, f>
        b = np.concatenate([g_far * f_far, g_near * f])
        assert abs(a.sum() - b.sum()) <= 1e-12 * (np.abs(a).sum() + np.abs(b).sum()), (devs, a.sum(), b.sum())
        h_far, h_near = op.eval_potential_transpose(wt, g_src_far=g_far.copy(), g_near=g_near.copy(), accumulate=True)
        assert rel_l2(h_far, 2 * g_far) < 1e-15 and rel_l2(h_near, 2 * g_near) < 1e-15
        op.set_targets(T)                                                                 # new targets drop the attached operator
        with pytest.raises(sctl_amd.api.SctlAmdError, match="no near-field operator"):
            op.eval_potential_transpose(wt)
        op.close()


@pytest.mark.gpu
def test_autograd_through_the_near_field_and_the_potential(O):
    import torch
    from sctl_amd import autograd
    case = next(c for c in CASES if c["key"] == "c3")
    k0, k1 = dims(O, case)
    xt, xnt, xs, xn, w, f = near_inputs(case, k0)
    arrs = {k: gold(case, k) for k in ARRS}
    near_op = sctl_amd.NearOp(k0, k1, **arrs)
    rng = np.random.default_rng(3)
    wt = rng.standard_normal(near_op.potential_len)
    fd = torch.from_numpy(f).cuda().requires_grad_(True)
    u = autograd.near_apply(near_op, fd)
    assert np.array_equal(u.detach().cpu().numpy(), near_op.apply(f))
    (u * torch.from_numpy(wt).cuda()).sum().backward()
    expect = near_op.apply_transpose_device(torch.from_numpy(wt).cuda(), torch.zeros(f.size, dtype=torch.float64, device="cuda"))
    assert np.array_equal(fd.grad.cpu().numpy(), expect.cpu().numpy())
    self_trg = case["Nt"] == 0
    T, Tn = (xs, xn) if self_trg else (xt, xnt)
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
    f_far = torch.from_numpy(np.repeat(f.reshape(-1, k0), ups, 0).ravel()).requires_grad_(True)
    f_near = torch.from_numpy(f.copy()).requires_grad_(True)
    u = autograd.potential(op, f_far, f_near)
    assert np.array_equal(u.detach().numpy(), op.eval_potential(f_far.detach().numpy(), f))
    (u * torch.from_numpy(wt)).sum().backward()
    g_far, g_near = op.eval_potential_transpose(wt)
    assert np.array_equal(f_far.grad.numpy(), g_far) and np.array_equal(f_near.grad.numpy(), g_near)
    op.close()
    near_op.close()
    # gradcheck on a 2-element, 5-target operator
    small = sctl_amd.NearOp(1, 1, [2, 3], [3, 4], rng.standard_normal(2 * 3 + 3 * 4), rng.permutation(7), [2, 1, 1, 2, 1], [0, 2, 3, 4, 6])
    x = torch.from_numpy(rng.standard_normal(5)).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: autograd.near_apply(small, t), (x,), eps=1e-6, atol=1e-7, nondet_tol=0.0)
    d = sctl_amd.DirectOp("Laplace3D-FxU", np.float64)
    d.set_targets(rng.standard_normal(15))
    d.set_sources(rng.standard_normal(15))
    d.set_source_weights(rng.random(5))
    d.set_near(1, [2, 3], [3, 4], rng.standard_normal(2 * 3 + 3 * 4), rng.permutation(7), [2, 1, 1, 2, 1], [0, 2, 3, 4, 6])
    a, b = (torch.from_numpy(rng.standard_normal(5)).requires_grad_(True) for _ in range(2))
    assert torch.autograd.gradcheck(lambda p, q: autograd.potential(d, p, q), (a, b), eps=1e-6, atol=1e-7)
    d.close()
    small.close()


@pytest.mark.gpu
def test_op_transpose_argument_errors_on_a_handle():
    """The error paths of sctl_amd_op_eval_transpose / _potential_transpose that need a live handle, and the empty sides."""
    L = sctl_amd.lib()
    z, g = np.ones(16), np.full(16, 7.0)
    d = sctl_amd.DirectOp("Stokes3D-FxT", np.float64)                                # TrgDim 9: contracts to 3 with target normals
    d.set_targets(np.arange(6.0))
    d.set_sources(np.arange(9.0) + 10)
    assert L.sctl_amd_op_eval_transpose(d._h, None, _p(g), 0, -1, None, 0) == BAD and b"null" in L.sctl_amd_last_error()
    assert L.sctl_amd_op_eval_transpose(d._h, _p(z), None, 0, -1, None, 0) == BAD
    assert L.sctl_amd_op_eval_potential_transpose(d._h, _p(z), _p(g), _p(g), 0, -1, None, 0) == BAD and b"no near-field operator" in L.sctl_amd_last_error()
    d.set_near(9, [1], [2], np.ones(3 * 18), [0, 1], [1, 1], [0, 1])
    assert L.sctl_amd_op_eval_potential_transpose(d._h, _p(np.ones(18)), _p(g), None, 0, -1, None, 0) == BAD and b"null" in L.sctl_amd_last_error()
    d.set_target_normals(np.ones(6))                                                 # the far field now delivers 3 per target, the near operator 9
    assert L.sctl_amd_op_eval_potential_transpose(d._h, _p(z), _p(g), _p(g), 0, -1, None, 0) == BAD and b"another potential dimension" in L.sctl_amd_last_error()
    d.close()
    h = sctl_amd.DirectOp("Helmholtz3D-FxU", np.float64, ctx=np.array([7.5, 0.3]))   # needs its context blob
    h.set_targets(np.arange(6.0))
    h.set_sources(np.arange(9.0) + 10)
    assert L.sctl_amd_op_eval_transpose(h._h, _p(z), _p(g), 0, -1, None, 0) == -5 and b"context blob" in L.sctl_amd_last_error()
    h.close()
    e = sctl_amd.DirectOp("Laplace3D-FxU", np.float64)                               # no sources: nothing to write; no targets: zeros, or G kept
    e.set_targets(np.arange(6.0))
    e.set_sources(np.zeros(0))
    c0 = sctl_amd.api.counters()["pair_interactions"]
    assert e.eval_transpose(np.ones(2)).size == 0
    e.set_near(1, [2], [2], np.array([1.0, 2.0, 3.0, 4.0]), [0, 1], [1, 1], [0, 1])
    g_far, g_near = e.eval_potential_transpose(np.array([1.0, 10.0]))               # Ns == 0: the near field alone, as in the forward
    assert g_far.size == 0 and np.array_equal(g_near, [21.0, 43.0])
    e.set_targets(np.zeros(0))
    e.set_sources(np.arange(6.0))
    assert np.array_equal(e.eval_transpose(np.zeros(0), g_src=np.full(2, 5.0)), [0.0, 0.0])
    assert np.array_equal(e.eval_transpose(np.zeros(0), g_src=np.full(2, 5.0), accumulate=True), [5.0, 5.0])
    assert sctl_amd.api.counters()["pair_interactions"] == c0
    e.close()


@pytest.mark.gpu
def test_op_transpose_refuses_a_plugin_kernel_without_pair_t(tmp_path_factory):
    """A registered kernel whose functor supplies no pair_t (tests/plugin/yukawa_kernel.hip): SCTL_AMD_ERR_UNKNOWN_KERNEL from the operator
    handle's transposed entries, while its forward evaluation works."""
    from test_gpu_transpose import LAM, _ensure
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    d = sctl_amd.DirectOp(name, np.float64, ctx=np.array([LAM]))
    d.set_targets(np.arange(6.0))
    d.set_sources(np.arange(9.0) + 10)
    assert np.all(np.isfinite(d.eval(np.ones(3))))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        d.eval_transpose(np.ones(2))
    d.set_near(1, [3], [2], np.ones(6), [0, 1], [1, 1], [0, 1])
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        d.eval_potential_transpose(np.ones(2))
    d.close()


DRIVER_CASES = [c for c in CASES if c["key"] in ("c0", "c3", "c5", "c6")]


def _driver_args(exe, case, out):
    return [exe, case["kernel"], str(case["seed"]), str(case["Nt"]), str(case["Ns"]), str(case["nodes_per_elem"]), str(case["upsample"]),
            str(case["trg_normal_dot_prod"]), str(int(case["Nt"] == 0)), out, repr(case["rad"]), str(case.get("free_nodes", 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DRIVER_CASES, ids=[c["key"] for c in DRIVER_CASES])
def test_compute_potential_transpose_end_to_end(tmp_path, case):
    """BoundaryIntegralOp::ComputePotentialTranspose (tests/cpp/bie_transpose_driver.cpp): <W, ComputePotential(F)> against
    <ComputePotentialTranspose(W), F>, the far field of both at the header's fmm_digits() for tolerance 1e-10."""
    import subprocess
    from test_cpp_host import _build, _read_vector
    exe = _build(tmp_path, "bie_transpose_driver")
    out = str(tmp_path / (case["key"] + ".bin"))
    p = subprocess.run(_driver_args(exe, case, out), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    G, ip = _read_vector(out), _read_vector(out + ".ip")
    k0, _ = dims(__import__("oracle").restatement(), case)
    assert G.size == case["Ns"] * k0 and np.all(np.isfinite(G))
    print("%s: <W, P F> = %.15e, <P^T W, F> = %.15e, difference %.2e of the sum of |terms|" % (case["key"], ip[0], ip[1], abs(ip[0] - ip[1]) / (ip[2] + ip[3])))
    assert abs(ip[0] - ip[1]) <= 1e-10 * (ip[2] + ip[3])


@pytest.mark.gpu
def test_compute_potential_transpose_refuses_matrix_free_lists(tmp_path):
    """A two-list operator whose second list is matrix-free (t0): the check comes before any setup, the driver aborts with the message."""
    import subprocess
    from test_cpp_host import _build
    case = next(c for c in CASES if c["key"] == "t0")
    exe = _build(tmp_path, "bie_transpose_driver")
    p = subprocess.run(_driver_args(exe, case, str(tmp_path / "t0.bin")), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "matrix-free element list" in p.stderr and "ComputePotentialTranspose" in p.stderr
