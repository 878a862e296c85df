"""Several weight vectors through the transposed list sum, G[m] += sum over the lists of A_l^T W[m] (sctl_amd_lists_eval_transpose_densities_*,
sctl_amd/csrc/lists_rows_kernel.hpp) on the GPU.

Expected value throughout: per list the KernelMatrix block of (target range, source range) from sctl_amd_kernel_matrix_batch_host at full precision —
the matrix the existing suite pins against the reference, which zeroes coincident pairs —, applied once to all nd rows of W in numpy long double and
added into the source range, as expected() of tests/test_gpu_lists_transpose.py does for one row.  It is never the several-vectors path itself nor nd
single transposed calls.  Inputs are fp32-representable doubles, so one expected value serves the fp64 and the fp32 run of a shape.  Tolerances are
the project's own: fp64 rel-L2 <= 1e-12 per row, fp32 <= 2e-5 against the fp64 expected value, digits = d <= 10 * 10^-d."""
import os
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ctx_for, rel_l2
from test_gpu_lists_transpose import DTS, KERNELS, TOL, as_dt, edge_shape, grid_shape, i8, r32, small_ranges  # noqa: F401  (small_ranges: a fixture)

pytestmark = pytest.mark.gpu

ND_MAX = 9
SHAPES = ["grid-8", "grid-32", "grid-70", "edges"]
_CASES = {}


def expected_rows(name, lists, xt, xs, xn, W, ctx=None, budget=1 << 22):
    """rows m of sum over the lists of M_l . W[m]_l in long double, M_l = KernelMatrix of (target range l, source range l)"""
    info = sctl_amd.kernel_info(name)
    k0, k1, nd = info["k0"], info["k1"], info["nd"]
    G = np.zeros((W.shape[0], xs.size // 3 * k0), dtype=np.longdouble)
    Wl = W.astype(np.longdouble)
    live = [l for l in range(lists[0].size) if lists[1][l] > 0 and lists[3][l] > 0]
    while live:
        n, size = 0, 0
        while n < len(live) and (n == 0 or size + lists[1][live[n]] * lists[3][live[n]] * k0 * k1 <= budget):
            size += lists[1][live[n]] * lists[3][live[n]] * k0 * k1
            n += 1
        batch, live = live[:n], live[n:]
        cut = lambda a, off, cnt, dim: np.concatenate([a[off[l] * dim:(off[l] + cnt[l]) * dim] for l in batch])
        Ms = sctl_amd.kernel_matrix_batch_host(name, lists[1][batch], lists[3][batch], cut(xt, lists[0], lists[1], 3), cut(xs, lists[2], lists[3], 3),
                                               cut(xn, lists[2], lists[3], nd) if nd else None, ctx=ctx)
        for l, M in zip(batch, Ms):
            t0, t1, s0, s1 = lists[0][l], lists[0][l] + lists[1][l], lists[2][l], lists[2][l] + lists[3][l]
            G[:, s0 * k0:s1 * k0] += Wl[:, t0 * k1:t1 * k1] @ M.astype(np.longdouble).T
    return G.astype(np.float64)


def weights(seed, nd, n):
    return r32(np.random.default_rng(seed), nd * n).reshape(nd, n)


def case(name, shape):
    """inputs, ND_MAX weight rows and their expected rows of (kernel, shape), computed once and shared by the fp64, fp32, digits and packing runs;
    a run of nd rows uses the first nd"""
    key = (name, shape)
    if key not in _CASES:
        info = sctl_amd.kernel_info(name)
        seed = 7000 + 31 * KERNELS.index(name) + SHAPES.index(shape)
        lists, xt, xs, xn, _ = edge_shape(seed, info) if shape == "edges" else grid_shape(seed, int(shape.split("-")[1]), info)
        nrows = ND_MAX if shape == "edges" else 5
        W = weights(seed + 1, nrows, xt.size // 3 * info["k1"])
        ctx = ctx_for(name)
        _CASES[key] = (lists, xt, xs, xn, W, ctx, expected_rows(name, lists, xt, xs, xn, W, ctx))
    return _CASES[key]


def make_plan(name, dt, lists, xt, xs, ctx, directions):
    return sctl_amd.ListsPlan(name, dt, *lists, xt.size // 3, xs.size // 3, ctx=ctx, directions=directions)


def several(name, dt, lists, xt, xs, xn, W, ctx, directions="transpose", digits=-1, G_src=None):
    plan = make_plan(name, dt, lists, xt, xs, ctx, directions)
    try:
        same = xt is xs
        xt_, xs_, xn_, W_ = as_dt(dt, xt, xs, xn, W)
        return plan.eval_transpose_densities_host(xt_, xt_ if same else xs_, xn_, W_, G_src=G_src, digits=digits)
    finally:
        plan.close()


def check_rows(G, ref, tol, what):
    assert G.shape == ref.shape and np.all(np.isfinite(G)), what
    errs = [rel_l2(G[m], ref[m]) for m in range(ref.shape[0])]
    print("%s: worst row rel-L2 %.3e" % (what, max(errs)))
    assert max(errs) <= tol, (what, errs)


@pytest.mark.parametrize("dt", DTS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_parity_with_kernel_matrix(name, dt, small_ranges):
    """edges: all seven item shapes, the halves, both SPL settings; nd = 2, 3, 5, 8, 9: every width, a partly filled form, one row left over, two passes"""
    lists, xt, xs, xn, W, ctx, ref = case(name, "edges")
    for nd in (2, 3, 5, 8, 9):
        G = several(name, dt, lists, xt, xs, xn, W[:nd], ctx, "transpose")
        check_rows(G, ref[:nd], TOL[dt], "%s %s edges %s nd %d" % (name, dt.__name__, small_ranges, nd))
    for shape in ("grid-8", "grid-70"):
        lists, xt, xs, xn, W, ctx, ref = case(name, shape)
        G = several(name, dt, lists, xt, xs, xn, W, ctx, "both")
        check_rows(G, ref, TOL[dt], "%s %s %s %s nd 5" % (name, dt.__name__, shape, small_ranges))


@pytest.mark.parametrize("name", KERNELS)
def test_sources_are_the_targets(name, small_ranges):
    """one array, every box against itself and its neighbours: a coincident pair in every self list (the packed known_coincident step and the tile
    repair), boxes of up to 8 and up to 70 points, nd = 3"""
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    for max_pts in (8, 70):
        lists, xt, xs, xn, _ = grid_shape(177 + max_pts, max_pts, info, self_targets=True)
        assert xt is xs
        W = weights(max_pts, 3, xt.size // 3 * info["k1"])
        ref = expected_rows(name, lists, xt, xs, xn, W, ctx)
        for dt in DTS:
            check_rows(several(name, dt, lists, xt, xs, xn, W, ctx, "both"), ref, TOL[dt], "%s self %d %s" % (name, max_pts, dt.__name__))


@pytest.mark.parametrize("name", KERNELS)
def test_coincident_points_in_separate_arrays(name, small_ranges):
    """one whole 64-record tile of streamed targets that coincide with owners (100 and 40 owners: two per lane, and packed or replicas): always_masked; nd = 4"""
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    rng = np.random.default_rng(5)
    xs2, xt2 = r32(rng, 140 * 3, 0.0), r32(rng, 200 * 3, 0.0)
    xt2[:64 * 3] = xs2[:64 * 3]                           # targets 0 .. 63 are sources 0 .. 63 (of the first owner range), and
    xt2[64 * 3:104 * 3] = xs2[100 * 3:]                   # targets 64 .. 103 the 40 sources of the second
    lists2 = [i8(0, 64, 0, 64), i8(64, 136, 64, 136), i8(0, 0, 100, 100), i8(100, 100, 40, 40)]
    xn2 = r32(rng, 140 * info["nd"]) if info["nd"] else None
    W = weights(6, 4, 200 * info["k1"])
    ref = expected_rows(name, lists2, xt2, xs2, xn2, W, ctx)
    for dt in DTS:
        check_rows(several(name, dt, lists2, xt2, xs2, xn2, W, ctx), ref, TOL[dt], "%s coincident %s" % (name, dt.__name__))


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-FxT", "Stokes3D-FxUP"])
def test_row_independence_padding_and_accumulation(name):
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, xn, W, ctx, ref = case(name, "edges")
    k0 = info["k0"]
    for dt in DTS:
        # a zero row stays exactly zero, and does not touch its neighbours
        W3 = W[:3].copy()
        W3[1] = 0
        G = several(name, dt, lists, xt, xs, xn, W3, ctx)
        assert not G[1].any()
        check_rows(G[[0, 2]], ref[[0, 2]], TOL[dt], "%s zero row %s" % (name, dt.__name__))
        # rows that are a slice of a larger array: rows 2 .. 4 of the nine, contiguous and row-major, without a copy
        big = W.astype(dt)
        part = big[2:5]
        assert part.base is not None and part.flags["C_CONTIGUOUS"]
        plan = make_plan(name, dt, lists, xt, xs, ctx, "transpose")
        xt_, xs_, xn_ = as_dt(dt, xt, xs, xn)
        Gp = plan.eval_transpose_densities_host(xt_, xs_, xn_, part)
        check_rows(Gp, ref[2:5], TOL[dt], "%s slice %s" % (name, dt.__name__))
        # a G given is accumulated into, in every row, and returned
        G0 = np.random.default_rng(2).random((3, xs.size // 3 * k0)).astype(dt)
        Ga = plan.eval_transpose_densities_host(xt_, xs_, xn_, part, G_src=G0.copy())
        assert np.array_equal(Ga, G0 + Gp)
        plan.close()
    # sources that no list names keep their bits: the edges lists with the owner range of 300 sources left out
    keep = lists[2] != lists[2].max()
    cut = [a[keep] for a in lists]
    s_lo = int(lists[2].max()) * k0
    G0 = np.random.default_rng(3).random((3, xs.size // 3 * k0))
    Gc = several(name, np.float64, cut, xt, xs, xn, W[:3], ctx, G_src=G0.copy())
    assert np.array_equal(Gc[:, s_lo:], G0[:, s_lo:]) and not np.array_equal(Gc[:, :s_lo], G0[:, :s_lo])


@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxUP"])
def test_bits_entries_and_counters(name):
    import torch
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, xn, W, ctx, ref = case(name, "grid-32")
    Nt, Ns = xt.size // 3, xs.size // 3
    nd = W.shape[0]
    plan = make_plan(name, np.float64, lists, xt, xs, ctx, "both")
    pairs = plan.transpose_info()["pairs"]
    assert pairs == int((lists[1] * lists[3]).sum())
    # nd == 1 IS the single-vector entry: the same bits
    assert np.array_equal(plan.eval_transpose_densities_host(xt, xs, xn, W[:1])[0], plan.eval_transpose_host(xt, xs, xn, W[0].copy()))
    pc0 = sctl_amd.counters()["pair_interactions"]
    G = plan.eval_transpose_densities_host(xt, xs, xn, W)
    assert sctl_amd.counters()["pair_interactions"] - pc0 == nd * pairs                              # the counters grow by nd x the plan's pairs
    check_rows(G, ref, 1e-12, name + " grid-32")
    assert np.array_equal(plan.eval_transpose_densities_host(xt, xs, xn, W), G)                       # run to run: the same bits
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, W)]
    Gd = plan.eval_transpose_densities_device(*d)
    torch.cuda.synchronize()
    assert np.array_equal(Gd.cpu().numpy(), G)                                                        # device entry against host entry: the same bits
    acc = torch.full((nd, Ns * info["k0"]), 0.5, dtype=torch.float64, device="cuda")
    assert plan.eval_transpose_densities_device(*d, G_src=acc) is acc                                 # ... and it accumulates: the kernel adds into G_src
    torch.cuda.synchronize()
    check_rows(acc.cpu().numpy(), ref + 0.5, 1e-12, name + " accumulated on the device")              # (the kernel's own add: one rounding, not the host entry's two)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Gs = plan.eval_transpose_densities_device(*d, stream=side)
    side.synchronize()
    assert np.array_equal(Gs.cpu().numpy(), G)
    assert np.array_equal(sctl_amd.eval_lists_transpose_densities_host(name, *lists, xt, xs, xn, W, ctx=ctx), G)      # the one-shot form
    Z = plan.eval_transpose_densities_device(d[0], d[1], d[2], torch.zeros((0, Nt * info["k1"]), dtype=torch.float64, device="cuda"))
    assert tuple(Z.shape) == (0, Ns * info["k0"])
    plan.close()


@pytest.mark.parametrize("dt", DTS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxT", "Helmholtz3D-FxU"])
def test_adjoint_identity_against_the_forward_densities_entry(name, dt):
    """|<W, L V> - <L^T W, V>| <= tol (|W| |L V| + |L^T W| |V|), summed over the rows; tol is the rel-L2 bound of the precision"""
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, xn, W, ctx, _ = case(name, "grid-32")
    nd = W.shape[0]
    V = weights(99, nd, xs.size // 3 * info["k0"])
    plan = make_plan(name, dt, lists, xt, xs, ctx, "both")
    xt_, xs_, xn_, W_, V_ = as_dt(dt, xt, xs, xn, W, V)
    U = plan.eval_densities_host(xt_, xs_, xn_, V_).astype(np.longdouble)
    G = plan.eval_transpose_densities_host(xt_, xs_, xn_, W_).astype(np.longdouble)
    plan.close()
    Wl, Vl = W.astype(np.longdouble), V.astype(np.longdouble)
    nrm = lambda a: float(np.sqrt((a * a).sum()))
    lhs, rhs = float((Wl * U).sum()), float((G * Vl).sum())
    bound = TOL[dt] * sum(nrm(Wl[m]) * nrm(U[m]) + nrm(G[m]) * nrm(Vl[m]) for m in range(nd))
    print("%s %s: <W, L V> = %.17g, <L^T W, V> = %.17g, |difference| %.3e, bound %.3e" % (name, dt.__name__, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("digits", [3, 10])
@pytest.mark.parametrize("name", KERNELS)
def test_digits(name, digits):
    lists, xt, xs, xn, W, ctx, ref = case(name, "grid-32")
    G = several(name, np.float64, lists, xt, xs, xn, W[:4], ctx, digits=digits)
    check_rows(G, ref[:4], 10.0 * 10.0 ** -digits, "%s digits %d" % (name, digits))


# ---- plugins ------------------------------------------------------------------------------------------------------------------------
LAM = 2.5


def test_plugin_with_pair_t_runs_row_by_row(tmp_path_factory):
    from test_gpu_transpose import _ensure, numpy_yukawa_matrix
    name = "Yukawa3D-FxU-T"
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    lists, xt, xs, _, _ = grid_shape(901, 32, info)
    xt[lists[0][0] * 3:lists[0][0] * 3 + 3] = xs[lists[2][0] * 3:lists[2][0] * 3 + 3]      # one coincident pair
    W = weights(902, 3, xt.size // 3)
    ref = np.zeros((3, xs.size // 3), dtype=np.longdouble)
    for t0, tc, s0, sc in zip(*lists):
        ref[:, s0:s0 + sc] += W[:, t0:t0 + tc].astype(np.longdouble) @ numpy_yukawa_matrix(xt[t0 * 3:(t0 + tc) * 3], xs[s0 * 3:(s0 + sc) * 3], LAM).T
    ref = ref.astype(np.float64)
    for dt in DTS:
        plan = make_plan(name, dt, lists, xt, xs, ctx, "transpose")
        xt_, xs_, W_ = as_dt(dt, xt, xs, W)
        pc0 = sctl_amd.counters()["pair_interactions"]
        G = plan.eval_transpose_densities_host(xt_, xs_, None, W_)
        assert sctl_amd.counters()["pair_interactions"] - pc0 == 3 * plan.transpose_info()["pairs"]
        check_rows(G, ref, TOL[dt], "%s %s" % (name, dt.__name__))
        for m in range(3):                                                                 # row by row through lists_transpose_kernel: its bits
            assert np.array_equal(G[m], plan.eval_transpose_host(xt_, xs_, None, W_[m].copy()))
        plan.close()


def test_plugin_without_pair_t_is_refused_at_plan_creation(tmp_path_factory):
    from test_gpu_transpose import _ensure
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, _, _ = grid_shape(41, 20, info)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        sctl_amd.eval_lists_transpose_densities_host(name, *lists, xt, xs, None, np.ones((2, xt.size // 3)), ctx=np.array([LAM]))


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
def _small(name, nd=3):
    import torch
    from test_gpu_lists_transpose import _small_plan
    info = sctl_amd.kernel_info(name)
    plan, xt, xs, xn, _ = _small_plan(name)
    V = torch.from_numpy(np.random.default_rng(12).random((nd, xs.numel() // 3 * info["k0"])) - 0.5).cuda().requires_grad_(True)
    return plan, xt, xs, xn, V


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-FxU"])
def test_autograd_gradcheck(name):
    """finite differences of lists_sum_densities' output against its backward: a 2^3 grid with at most 6 points per box, nd = 3, fp64"""
    import torch
    from sctl_amd.autograd import lists_sum_densities
    plan, xt, xs, xn, V = _small(name)
    fn = lambda V_: lists_sum_densities(plan, xt, xs, xn, V_)
    assert torch.autograd.gradcheck(fn, (V,), eps=1e-3, atol=1e-7, rtol=1e-7, nondet_tol=0.0)     # (linear in V: a large step has no truncation error)
    U = fn(V)
    U.square().sum().backward()
    assert torch.equal(V.grad, plan.eval_transpose_densities_device(xt, xs, xn, (2 * U).detach()))   # bit-equal to the transposed entry on 2 U
    plan.close()


def test_autograd_refusals():
    import torch
    from sctl_amd.autograd import lists_sum_densities
    plan, xt, xs, xn, V = _small("Laplace3D-FxU")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_src requires grad"):
        lists_sum_densities(plan, xt, xs.clone().requires_grad_(True), None, V)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_trg requires grad"):
        lists_sum_densities(plan, xt.clone().requires_grad_(True), xs, None, V)
    fwd = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, i8(0), i8(xt.numel() // 3), i8(0), i8(xs.numel() // 3), xt.numel() // 3, xs.numel() // 3)
    with pytest.raises(sctl_amd.api.SctlAmdError, match='directions="both"'):
        lists_sum_densities(fwd, xt, xs, None, V)
    (gV,) = torch.autograd.grad(lists_sum_densities(plan, xt, xs, None, V).square().sum(), V, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gV.sum().backward()
    fwd.close()
    plan.close()


# ---- C++ ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_lists_transpose_densities(tmp_path):
    """tests/cpp/lists_transpose_densities_driver.cpp: GenericKernel<...>::EvalListsTransposeDensities against a loop of EvalListsTranspose over the
    rows (g++ -Wall -Werror)"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "lists_transpose_densities_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
