"""The tangent of a kernel sum along a perturbation of the geometry (sctl_amd_eval_jvp_*, sctl_amd/csrc/jvp_kernel.hpp) on the GPU.

Expected value throughout: torch.func.jvp on the CPU, in fp64, of u = einsum("tsjk,sj->tk", kernel_blocks(...), f) with the dense formula of
tests/grad_truth.py (which tests/test_grad_cpu.py ties to the reference's KernelMatrix).  The inputs and the tangents are fp32-representable doubles,
so one truth serves the fp64 and the fp32 run of a shape.  Bounds: fp64 rel-L2 <= 1e-12 at full precision and 10 * 10^-d at digits = d (DESIGN.md
§2).  fp32 has no fitted number: the same formula and its tangent in torch float32 on the same inputs has some rel-L2 against the fp64 truth, computed
here per case, and the kernel is allowed 4 times that (the rule of tests/test_gpu_grad.py).  Every figure is printed before it is asserted."""
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ctx_for, rel_l2
from grad_truth import HELMHOLTZ_KS, kernel_blocks
from test_gpu_grad import as_dt, cloud, share_points

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES


def tangents(seed, Nt, Ns, info):
    """fp32-representable doubles drawn as cloud() draws densities: tangents of the targets, the sources and the normals"""
    rng = np.random.default_rng(seed)
    r32 = lambda n: (rng.random(n) - 0.5).astype(np.float32).astype(np.float64)
    return r32(Nt * 3), r32(Ns * 3), (r32(Ns * 3) if info["nd"] else None)


def truth(name, xt, xs, xn, f, dxt, dxs, dxn, ctx, dtype=None, df=None):
    """the tangent of u along (dxt, dxs, dxn) and, with df, along the densities too; None is a zero tangent.  Flat numpy, in `dtype` (default fp64)."""
    import torch
    dtype = dtype or torch.float64
    k0 = f.size // (xs.size // 3)
    T = lambda a, k: None if a is None else torch.from_numpy(a).to(dtype).view(-1, k)
    Z = lambda a, like: torch.zeros_like(like) if a is None else T(a, like.shape[1])
    t_xt, t_xs, t_xn, t_f = T(xt, 3), T(xs, 3), T(xn, 3), T(f, k0)
    c = None if ctx is None else tuple(ctx)
    if t_xn is None:
        fn = lambda a, b, g: torch.einsum("tsjk,sj->tk", kernel_blocks(name, a, b, None, c), g)
        _, du = torch.func.jvp(fn, (t_xt, t_xs, t_f), (Z(dxt, t_xt), Z(dxs, t_xs), Z(df, t_f)))
    else:
        fn = lambda a, b, n, g: torch.einsum("tsjk,sj->tk", kernel_blocks(name, a, b, n, c), g)
        _, du = torch.func.jvp(fn, (t_xt, t_xs, t_xn, t_f), (Z(dxt, t_xt), Z(dxs, t_xs), Z(dxn, t_xn), Z(df, t_f)))
    return du.numpy().ravel()


_CASES = {}


def case(name, Nt, Ns, ctx_key="default", shared=0):
    """inputs, tangents, the fp64 truth and torch-fp32's error against it, computed once per (kernel, shape) and shared by the tests"""
    key = (name, Nt, Ns, ctx_key, shared)
    if key not in _CASES:
        import torch
        info = sctl_amd.kernel_info(name)
        xt, xs, xn, f, _ = cloud(4000 + 17 * KERNELS.index(name) + Nt + Ns, Nt, Ns, info)
        if shared:
            share_points(xt, xs, shared, 5)
        dxt, dxs, dxn = tangents(6000 + 13 * KERNELS.index(name) + Nt + Ns, Nt, Ns, info)
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        ref = truth(name, xt, xs, xn, f, dxt, dxs, dxn, ctx)
        err32 = rel_l2(truth(name, xt, xs, xn, f, dxt, dxs, dxn, ctx, dtype=torch.float32), ref)
        _CASES[key] = (xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, err32)
    return _CASES[key]


def bound_for(dt, digits, err32):
    if dt == np.float64:
        return 1e-12 if digits < 0 else 10.0 * 10.0 ** -digits
    return 4.0 * err32


def check(tag, got, ref, bound):
    """prints the figure before it asserts"""
    err, finite = rel_l2(got, ref), bool(np.all(np.isfinite(got)))
    print("%s: rel-L2 %.2e (bound %.2e)" % (tag, err, bound))
    assert finite and err <= bound, (tag, err, bound)


def jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, **kw):
    a = as_dt(dt, xt, xs, xn, f, dxt, dxs, dxn)
    return sctl_amd.eval_jvp_host(name, a[0], a[1], a[2], a[3], d_trg=a[4], d_src=a[5], d_nrm=a[6], **kw)


@pytest.mark.parametrize("dt,digits", [(np.float64, -1), (np.float64, 10), (np.float32, -1), (np.float32, 9)], ids=["f64", "f64-d10", "f32", "f32-d9"])
@pytest.mark.parametrize("name", KERNELS)
def test_small_shape(name, dt, digits):
    """300 targets x 50 sources: one tile, the always-masked path"""
    xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, err32 = case(name, 300, 50)
    got = jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, digits=digits, ctx=ctx)
    assert got.dtype == dt
    check("%s %s digits %d 300 x 50" % (name, dt.__name__, digits), got, ref, bound_for(dt, digits, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_ragged_shapes_with_shared_points(name, dt):
    """513 x 1100 and 1100 x 513, 40 points shared between the sets: a ragged last tile, a ragged last workgroup, several splits through the reduce
    (asserted from the plan); the shared pairs contribute exactly 0, as in the truth"""
    for Nt, Ns in ((513, 1100), (1100, 513)):
        assert sctl_amd.plan_jvp(name, 0 if dt == np.float64 else 1, Nt, Ns)["splits"] > 1
        xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, err32 = case(name, Nt, Ns, shared=40)
        got = jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, ctx=ctx)
        check("%s %s %d x %d, 40 shared" % (name, dt.__name__, Nt, Ns), got, ref, bound_for(dt, -1, err32))


# ---- the unmasked pass and its repair -----------------------------------------------------------------------------------------------------
SPEC_NT, SPEC_NS = 20000 + 77, 13 * 4 * 256 + 300     # 79 workgroups -> 13 splits wanted -> at least 4 tiles per split (asserted from the plan)
_SPEC = {}


def _spec_case(name):
    """inputs, and the truth for some 70 targets against all sources (the dense truth of the whole shape is out of reach)"""
    if name not in _SPEC:
        import torch
        info = sctl_amd.kernel_info(name)
        xt, xs, xn, f, _ = cloud(700 + KERNELS.index(name), SPEC_NT, SPEC_NS, info)
        t, _s = share_points(xt, xs, 40, 7)
        dxt, dxs, dxn = tangents(800 + KERNELS.index(name), SPEC_NT, SPEC_NS, info)
        sub = np.unique(np.r_[t, 0:8, 254:258, SPEC_NT - 20:SPEC_NT])       # the shared targets, a workgroup boundary, the ragged last workgroup
        ctx = ctx_for(name)
        pick = lambda a: a.reshape(-1, 3)[sub].ravel().copy()
        ref = truth(name, pick(xt), xs, xn, f, pick(dxt), dxs, dxn, ctx)
        err32 = rel_l2(truth(name, pick(xt), xs, xn, f, pick(dxt), dxs, dxn, ctx, dtype=torch.float32), ref)
        _SPEC[name] = (xt, xs, xn, f, dxt, dxs, dxn, ctx, sub, ref, err32)
    return _SPEC[name]


@pytest.mark.parametrize("name", KERNELS)
def test_unmasked_pass_and_repair(name):
    """Each split holds at least four tiles, so tiles run unmasked, and 40 shared points send some of them through the compare and the masked re-run.
    Both precisions against the truth of some 70 targets (all shared ones among them) over all sources; the rest of the fp64 result must be finite."""
    import torch
    k1 = sctl_amd.kernel_info(name)["k1"]
    xt, xs, xn, f, dxt, dxs, dxn, ctx, sub, ref, err32 = _spec_case(name)
    rows = (sub[:, None] * k1 + np.arange(k1)).ravel()
    for dt in (np.float64, np.float32):
        pl = sctl_amd.plan_jvp(name, 0 if dt == np.float64 else 1, SPEC_NT, SPEC_NS)
        tiles = -(-SPEC_NS // 256)
        per = -(-tiles // pl["splits"])                       # tiles per split; the last split holds what is left
        assert per >= 4 and tiles - (pl["splits"] - 1) * per >= 4, pl
        d = [None if a is None else torch.from_numpy(a.astype(dt)).cuda() for a in (xt, xs, xn, f, dxt, dxs, dxn)]
        got = sctl_amd.eval_jvp_device(name, d[0], d[1], d[2], d[3], d_trg=d[4], d_src=d[5], d_nrm=d[6], ctx=ctx).cpu().numpy()
        assert np.all(np.isfinite(got))
        check("%s %s %s" % (name, dt.__name__, pl), got[rows], ref, bound_for(dt, -1, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_targets_cut_into_several_launches(name, dt, monkeypatch):
    """The cut of the targets that keeps the partial sums under 2 GB, with the bound lowered to one workgroup's 256 owners: bit for bit the single launch"""
    real, k1 = (0 if dt == np.float64 else 1), sctl_amd.kernel_info(name)["k1"]
    for Nt, Ns in ((513, 1100), (1100, 513)):
        xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, err32 = case(name, Nt, Ns, shared=40)
        whole = jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, ctx=ctx)
        one = sctl_amd.plan_jvp(name, real, Nt, Ns)
        assert one["splits"] > 1 and one["workspace_bytes"] == one["splits"] * Nt * k1 * dt().itemsize, one
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", "1")
        try:
            pl = sctl_amd.plan_jvp(name, real, Nt, Ns)
            assert pl["workspace_bytes"] == pl["splits"] * 256 * k1 * dt().itemsize, pl
            cut = jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, ctx=ctx)
        finally:
            monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
        assert np.array_equal(cut, whole), (name, Nt, Ns)


@pytest.mark.parametrize("k", HELMHOLTZ_KS, ids=["complex-one-reduction", "real-one-reduction", "complex-two-reductions", "re0-two-reductions"])
def test_helmholtz_wavenumbers(k):
    """the wavenumbers of the transposed and gradient tests: every table form and variant the forward kernel has"""
    name = "Helmholtz3D-FxU"
    for Nt, Ns in ((300, 50), (513, 1100)):
        xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, err32 = case(name, Nt, Ns, k, shared=0 if Nt == 300 else 40)
        for dt, digits in ((np.float64, -1), (np.float64, 10), (np.float32, -1)):
            got = jvp_host(name, dt, xt, xs, xn, f, dxt, dxs, dxn, digits=digits, ctx=ctx)
            check("Helmholtz k %s %s digits %d %d x %d" % (k, dt.__name__, digits, Nt, Ns), got, ref, bound_for(dt, digits, err32))


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-DxU", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"])
def test_null_tangents_and_linearity(name):
    """each tangent alone with the others null is bit for bit the call with zero arrays in their place; the single-tangent results sum to the full call;
    an output passed in is accumulated into; with all three null the output is untouched; d_nrm for a kernel without a normal raises"""
    import torch
    xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, _ = case(name, 513, 1100, shared=40)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, f)]
    tan = [None if a is None else torch.from_numpy(a).cuda() for a in (dxt, dxs, dxn)]
    J = lambda t, **kw: sctl_amd.eval_jvp_device(name, *d, d_trg=t[0], d_src=t[1], d_nrm=t[2], ctx=ctx, **kw)
    full = J(tan)
    check("%s full" % name, full.cpu().numpy(), ref, 1e-12)
    parts = torch.zeros_like(full)
    for i in range(3):
        if tan[i] is None:
            continue
        alone = J([tan[j] if j == i else None for j in range(3)])
        zeros = J([tan[j] if j == i else (None if tan[j] is None else torch.zeros_like(tan[j])) for j in range(3)])
        assert torch.equal(alone, zeros), (name, i)
        parts += alone
    gap = float((parts - full).norm() / full.norm())
    print("%s: sum of the single tangents against the full call %.2e" % (name, gap))
    assert gap <= 1e-12
    # accumulation into an output passed in, and the null call
    rng = np.random.default_rng(3)
    u0 = torch.from_numpy(rng.random(full.numel()) - 0.5).cuda()
    buf = u0.clone()
    assert J(tan, dv_trg=buf) is buf
    check("%s accumulated" % name, buf.cpu().numpy(), u0.cpu().numpy() + ref, 1e-12)
    buf = u0.clone()
    assert J([None, None, None], dv_trg=buf) is buf and torch.equal(buf, u0)
    h0 = u0.cpu().numpy().copy()
    h = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, dv_trg=h0.copy(), ctx=ctx)
    assert np.array_equal(h, h0)
    if xn is None:
        with pytest.raises(sctl_amd.api.SctlAmdError, match="d_nrm must be null"):
            sctl_amd.eval_jvp_device(name, *d, d_nrm=torch.zeros(1100 * 3, dtype=torch.float64, device="cuda"), ctx=ctx)


@pytest.mark.parametrize("name", KERNELS)
def test_translation(name):
    """u depends on differences of coordinates only: moving both sets by one constant vector, with the normals fixed, changes nothing"""
    xt, xs, xn, f, _, _, _, ctx, _, _ = case(name, 1100, 513, shared=40)
    c = np.array([0.375, -0.625, 0.25])
    ct, cs = np.tile(c, 1100), np.tile(c, 513)
    both = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, d_trg=ct, d_src=cs, ctx=ctx)
    alone = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, d_trg=ct, ctx=ctx)
    print("%s: |du| %.3e for both sets moved, %.3e for the targets alone" % (name, np.linalg.norm(both), np.linalg.norm(alone)))
    assert np.linalg.norm(alone) > 0 and np.linalg.norm(both) <= 1e-12 * np.linalg.norm(alone)


@pytest.mark.parametrize("name", KERNELS)
def test_duality_with_the_gradient_entry(name):
    """<w, J delta> = <J^T w, delta> with the merged reverse-mode entry: <w, eval_jvp(delta)> against <eval_grad(w), delta>"""
    Nt, Ns = 1100, 513
    xt, xs, xn, f, dxt, dxs, dxn, ctx, _, _ = case(name, Nt, Ns, shared=40)
    w = (np.random.default_rng(9).random(Nt * sctl_amd.kernel_info(name)["k1"]) - 0.5).astype(np.float32).astype(np.float64)
    du = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, d_trg=dxt, d_src=dxs, d_nrm=dxn, ctx=ctx)
    g = sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, ctx=ctx)
    lhs = np.longdouble(0) + (w.astype(np.longdouble) * du).sum()
    pairs = [(a, b) for a, b in zip(g, (dxt, dxs, dxn)) if a is not None]
    rhs = sum((a.astype(np.longdouble) * b).sum() for a, b in pairs)
    mag = np.abs(w * du).sum() + sum(np.abs(a * b).sum() for a, b in pairs)
    print("%s: <w, J d> %.15e, <J^T w, d> %.15e, difference %.2e of %.3e" % (name, float(lhs), float(rhs), float(abs(lhs - rhs)), mag))
    assert abs(lhs - rhs) <= 1e-12 * mag


@pytest.mark.parametrize("name", ["Stokes3D-FxT", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"])
def test_bit_reproducible(name):
    """six calls, several splits through the reduce, with another kernel between them: identical bits"""
    import torch
    xt, xs, xn, f, dxt, dxs, dxn, ctx, _, _ = case(name, 513, 1100, shared=40)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, dxt, dxs, dxn)]
    runs = []
    for i in range(6):
        runs.append(sctl_amd.eval_jvp_device(name, d[0], d[1], d[2], d[3], d_trg=d[4], d_src=d[5], d_nrm=d[6], ctx=ctx))
        sctl_amd.eval_jvp_device("Stokes3D-FxU", d[0], d[1], None, torch.ones(1100 * 3, dtype=torch.float64, device="cuda"), d_trg=d[4])
    assert all(torch.equal(runs[0], r) for r in runs[1:])


def test_side_stream_empty_sets_and_counters():
    """the device entry on a side stream equals the host entry; an empty set touches nothing; the counters grow by Nt * Ns pairs"""
    import torch
    name = "Laplace3D-FDxUdU"
    xt, xs, xn, f, dxt, dxs, dxn, ctx, ref, _ = case(name, 513, 1100, shared=40)
    host = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, d_trg=dxt, d_src=dxs, d_nrm=dxn)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, dxt, dxs, dxn)]
        dev = sctl_amd.eval_jvp_device(name, d[0], d[1], d[2], d[3], d_trg=d[4], d_src=d[5], d_nrm=d[6], stream=st)
    st.synchronize()
    check("side stream", dev.cpu().numpy(), ref, 1e-12)
    assert np.array_equal(dev.cpu().numpy(), host)
    check("GenericKernel.EvalJvp", sctl_amd.GenericKernel(name).EvalJvp(xt, xs, xn, f, dxt, dxs, dxn), ref, 1e-12)
    over = sctl_amd.eval_jvp_host(name, xt, xs, xn, f, d_trg=dxt, d_src=dxs, d_nrm=dxn, dv_trg=np.full(ref.size, 7.0), accumulate=False)
    assert np.array_equal(over, host)
    # empty sets: nothing is touched
    e, keep = np.zeros(0), np.full(ref.size, 7.0)
    assert sctl_amd.eval_jvp_host(name, e, xs, xn, f, d_src=dxs).size == 0                                  # Nt = 0
    got = sctl_amd.eval_jvp_host(name, xt, e, e, e, d_trg=dxt, dv_trg=keep.copy())                          # Ns = 0
    assert np.array_equal(got, keep)
    flops = sctl_amd.kernel_info(name)["flops"]
    for kw, pairs in ((dict(d_trg=dxt), 513 * 1100), (dict(d_trg=dxt, d_src=dxs, d_nrm=dxn), 513 * 1100), (dict(), 0)):
        sctl_amd.reset_counters()
        sctl_amd.eval_jvp_host(name, xt, xs, xn, f, **kw)
        c = sctl_amd.counters()
        assert c["pair_interactions"] == pairs and c["sctl_flops"] == pairs * flops, (kw.keys(), c)


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxU"])
def test_forward_mode_through_kernel_sum_geometry(name):
    """torch.func.jvp through sctl_amd.autograd.kernel_sum_geometry with tangents on coordinates, normals and densities against the truth, which
    includes the A dv term; torch.autograd.forward_ad gives the same; backward through the same function still matches eval_grad"""
    import torch
    import torch.autograd.forward_ad as fwAD
    from sctl_amd.autograd import kernel_sum_geometry
    Nt, Ns = 300, 50
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, f, dxt, dxs, dxn, ctx, _, _ = case(name, Nt, Ns)
    df = (np.random.default_rng(21).random(f.size) - 0.5).astype(np.float32).astype(np.float64)
    ref = truth(name, xt, xs, xn, f, dxt, dxs, dxn, ctx, df=df)
    C = lambda a: None if a is None else torch.from_numpy(a).cuda()
    prim = [C(a) for a in (xt, xs, xn, f)]
    tang = [C(a) for a in (dxt, dxs, dxn, df)]
    if xn is None:
        fn = lambda a, b, g: kernel_sum_geometry(name, a, b, None, g, ctx=ctx)
        u, du = torch.func.jvp(fn, (prim[0], prim[1], prim[3]), (tang[0], tang[1], tang[3]))
    else:
        fn = lambda a, b, n, g: kernel_sum_geometry(name, a, b, n, g, ctx=ctx)
        u, du = torch.func.jvp(fn, tuple(prim), tuple(tang))
    assert torch.equal(u, sctl_amd.eval_device(name, *prim, ctx=ctx))
    check("%s torch.func.jvp, all tangents" % name, du.cpu().numpy(), ref, 1e-12)
    # the densities held fixed: the geometry tangent alone is eval_jvp_device's bits
    _, dg = torch.func.jvp(lambda a: kernel_sum_geometry(name, a, prim[1], prim[2], prim[3], ctx=ctx), (prim[0],), (tang[0],))
    assert torch.equal(dg, sctl_amd.eval_jvp_device(name, *prim, d_trg=tang[0], ctx=ctx))
    with fwAD.dual_level():
        o = kernel_sum_geometry(name, fwAD.make_dual(prim[0], tang[0]), fwAD.make_dual(prim[1], tang[1]), prim[2], fwAD.make_dual(prim[3], tang[3]), ctx=ctx)
        dfw = fwAD.unpack_dual(o).tangent
    check("%s forward_ad, no normal tangent" % name, dfw.cpu().numpy(), truth(name, xt, xs, xn, f, dxt, dxs, None, ctx, df=df), 1e-12)
    # backward is what it was
    w = (np.random.default_rng(22).random(Nt * info["k1"]) - 0.5).astype(np.float32).astype(np.float64)
    req = [None if a is None else a.clone().requires_grad_(True) for a in prim]
    (kernel_sum_geometry(name, *req, ctx=ctx) * C(w)).sum().backward()
    g = sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, ctx=ctx)
    for what, a, b in zip(("r_trg", "r_src", "n_src"), req, g):
        if a is not None:
            assert np.array_equal(a.grad.cpu().numpy().ravel(), b), (name, what)
    assert np.array_equal(req[3].grad.cpu().numpy(), sctl_amd.eval_transpose_host(name, xt, xs, xn, w, ctx=ctx))


# ---- C++ --------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_jvp_against_the_python_entry(tmp_path):
    """tests/cpp/jvp_driver.cpp: GenericKernel<Stokes3D_DxU>::EvalJvp (g++ -Wall -Werror) writes its inputs, its tangents and its result; the Python
    entry on the same inputs gives the same bits"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "jvp_driver")
    out = str(tmp_path / "jvp.bin")
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    Nt, Ns = 700, 450
    a = np.fromfile(out, dtype=np.float64)
    sizes = [Nt * 3, Ns * 3, Ns * 3, Ns * 3, Nt * 3, Ns * 3, Ns * 3, Nt * 3]
    assert a.size == sum(sizes)
    xt, xs, xn, f, dxt, dxs, dxn, du = [x.copy() for x in np.split(a, np.cumsum(sizes)[:-1])]
    assert np.array_equal(sctl_amd.eval_jvp_host("Stokes3D-DxU", xt, xs, xn, f, d_trg=dxt, d_src=dxs, d_nrm=dxn), du)
