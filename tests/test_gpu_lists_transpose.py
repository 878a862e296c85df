"""The transposed list sum g_src += sum over the lists of A_l^T w_trg (sctl_amd_lists_eval_transpose_*, include/sctl_amd/device/lists_transpose_kernel.hpp)
on the GPU.

Expected value throughout: per list the KernelMatrix block of (target range, source range) from sctl_amd_kernel_matrix_batch_host at full precision —
the (ns*K0) x (nt*K1) matrix the existing suite pins against the reference, which zeroes coincident pairs —, multiplied by w in numpy long double and
added into the source range.  Inputs are fp32-representable doubles, so one expected value serves the fp64 and the fp32 run of a shape.  Tolerances
are the project's own: fp64 rel-L2 <= 1e-12, fp32 <= 2e-5 against the fp64 expected value, digits = d <= 10 * 10^-d."""
import os
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ctx_for, rel_l2
from sctl_amd.lists import grid_neighbour_lists, points_in_boxes

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
TOL = {np.float64: 1e-12, np.float32: 2e-5}
DTS = [np.float64, np.float32]
i8 = lambda *v: np.array(v, dtype=np.int64)


@pytest.fixture(params=["packed", "packed up to 64", "one range per wave"])
def small_ranges(request):
    """the three packing settings of tests/test_lists.py: owner ranges of up to 32 points packed (the default), up to 64 (SCTL_AMD_LISTS_PACK=64), none (=0)"""
    if request.param == "packed":
        os.environ.pop("SCTL_AMD_LISTS_PACK", None)
        yield request.param
    else:
        os.environ["SCTL_AMD_LISTS_PACK"] = "64" if request.param.endswith("64") else "0"
        try:
            yield request.param
        finally:
            del os.environ["SCTL_AMD_LISTS_PACK"]


def r32(rng, n, shift=0.5):
    return (rng.random(n) - shift).astype(np.float32).astype(np.float64)     # rounded to fp32 LAST: exactly representable


def expected(name, lists, xt, xs, xn, w, ctx=None, g0=None, budget=1 << 22):
    """sum over the lists of M_l . w_l in long double, M_l = KernelMatrix of (target range l, source range l), `budget` matrix entries per launch"""
    info = sctl_amd.kernel_info(name)
    k0, k1, nd = info["k0"], info["k1"], info["nd"]
    g = np.zeros(xs.size // 3 * k0, dtype=np.longdouble) if g0 is None else g0.astype(np.longdouble)
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
            g[s0 * k0:s1 * k0] += M.astype(np.longdouble) @ w[t0 * k1:t1 * k1].astype(np.longdouble)
    return g.astype(np.float64)


def grid_shape(seed, max_pts, info, self_targets=False):
    """a 3^3 grid, every box against itself and its neighbours (343 lists), 1 .. max_pts points per box"""
    rng = np.random.default_rng(seed)
    cs = rng.integers(1, max_pts + 1, 27)
    ct = cs if self_targets else rng.integers(1, max_pts + 1, 27)
    xs = points_in_boxes(3, cs, rng, np.float32).astype(np.float64)
    xt = xs if self_targets else points_in_boxes(3, ct, rng, np.float32).astype(np.float64)
    Ns, Nt = int(cs.sum()), int(ct.sum())
    xn = r32(rng, Ns * info["nd"]) if info["nd"] else None
    return [a.copy() for a in grid_neighbour_lists(3, ct, cs)], xt, xs, xn, r32(rng, Nt * info["k1"])


OWNERS = [1, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 300]


def edge_shape(seed, info):
    """Hand-made lists.  Owner (source) ranges of the sizes at which the item shape changes; streamed sequences of 63, 64, 65 and 1000 records (ranges A, B,
    C, D) and one built from thirty ranges of 5 points (E); every source range is listed by several target ranges, not in sorted order, and the lists come
    owner by owner in descending order (the plan sorts them back, keeping the order inside a group); two target ranges overlap the others, which only a transposed-only plan accepts."""
    rng = np.random.default_rng(seed)
    A, B, Cc, D = (0, 63), (63, 64), (127, 65), (192, 1000)
    E = [(1192 + 5 * j, 5) for j in range(30)]
    Nt, Ns = 1342, sum(OWNERS)
    s_off = np.concatenate([[0], np.cumsum(OWNERS)[:-1]])
    rows = []
    for i, n in enumerate(OWNERS):
        mine = []
        if i % 2 == 0:
            mine += E[::-1]                              # descending target offsets: the group's order is the caller's, not a sorted one
        if i in (2, 8, 12):
            mine.append(D)
        mine.append((A, B, Cc)[i % 3])
        if i == 3:
            mine.append((30, 70))                        # overlaps A and B
        if i == 13:
            mine.append((100, 200))                      # overlaps B, C and D
        rows += [(t0, tc, int(s_off[i]), n) for t0, tc in mine]
    # Lists arrive owner by owner in DESCENDING owner order; inside an owner's group the order above is kept (it is the summation order)
    rows = [r for i in reversed(range(len(OWNERS))) for r in rows if r[2] == int(s_off[i])]
    lists = [np.array([r[c] for r in rows], dtype=np.int64) for c in range(4)]
    xt, xs = r32(rng, Nt * 3, 0.0), r32(rng, Ns * 3, 0.0)
    xn = r32(rng, Ns * info["nd"]) if info["nd"] else None
    return lists, xt, xs, xn, r32(rng, Nt * info["k1"])


SHAPES = ["grid-8", "grid-32", "grid-64", "grid-200", "edges"]
_CASES = {}


def case(name, shape):
    """inputs and expected value of (kernel, shape), computed once and shared by the fp64, fp32, digits and packing runs"""
    key = (name, shape)
    if key not in _CASES:
        info = sctl_amd.kernel_info(name)
        seed = 5000 + 31 * KERNELS.index(name) + SHAPES.index(shape)
        lists, xt, xs, xn, w = edge_shape(seed, info) if shape == "edges" else grid_shape(seed, int(shape.split("-")[1]), info)
        ctx = ctx_for(name)
        _CASES[key] = (lists, xt, xs, xn, w, ctx, expected(name, lists, xt, xs, xn, w, ctx))
    return _CASES[key]


def as_dt(dt, *arrays):
    return [None if a is None else a.astype(dt) for a in arrays]


def transposed(name, dt, lists, xt, xs, xn, w, ctx, directions="transpose", digits=-1, g_src=None):
    plan = sctl_amd.ListsPlan(name, dt, *lists, xt.size // 3, xs.size // 3, ctx=ctx, directions=directions)
    try:
        same = xt is xs
        xt_, xs_, xn_, w_ = as_dt(dt, xt, xs, xn, w)
        return plan.eval_transpose_host(xt_, xt_ if same else xs_, xn_, w_, g_src=g_src, digits=digits), plan.transpose_info()
    finally:
        plan.close()


@pytest.mark.parametrize("dt", DTS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_parity_with_kernel_matrix(name, dt, small_ranges):
    for shape in SHAPES:
        lists, xt, xs, xn, w, ctx, ref = case(name, shape)
        g, info = transposed(name, dt, lists, xt, xs, xn, w, ctx, "transpose" if shape == "edges" else "both")
        err = rel_l2(g, ref)
        print("%s %s %s %s: %d work items, rel-L2 %.3e" % (name, dt.__name__, shape, small_ranges, info["work_items"], err))
        assert info["pairs"] == int((lists[1] * lists[3]).sum())
        assert np.all(np.isfinite(g)) and err <= TOL[dt], (shape, err)


@pytest.mark.parametrize("digits", [3, 10])
@pytest.mark.parametrize("name", KERNELS)
def test_digits(name, digits):
    for shape in ("grid-32", "edges"):
        lists, xt, xs, xn, w, ctx, ref = case(name, shape)
        g, _ = transposed(name, np.float64, lists, xt, xs, xn, w, ctx, digits=digits)
        err = rel_l2(g, ref)
        print("%s digits %d %s: rel-L2 %.3e" % (name, digits, shape, err))
        assert err <= 10.0 * 10.0 ** -digits, (shape, err)


@pytest.mark.parametrize("name", KERNELS)
def test_sources_are_the_targets(name, small_ranges):
    """one array, every box against itself and its neighbours: a coincident pair in every self list (in the packed form the step that fetches a group's own
    points runs masked at once), boxes of up to 8 and up to 70 points"""
    info = sctl_amd.kernel_info(name)
    for max_pts in (8, 70):
        lists, xt, xs, xn, w = grid_shape(77 + max_pts, max_pts, info, self_targets=True)
        assert xt is xs
        ctx = ctx_for(name)
        ref = expected(name, lists, xt, xs, xn, w, ctx)
        for dt in DTS:
            g, _ = transposed(name, dt, lists, xt, xs, xn, w, ctx, "both")
            assert np.all(np.isfinite(g)) and rel_l2(g, ref) <= TOL[dt], (max_pts, dt, rel_l2(g, ref))


@pytest.mark.parametrize("name", KERNELS)
def test_coincident_points_in_separate_arrays(name, small_ranges):
    """a handful of shared points in a grid, and one whole 64-record tile of streamed targets that coincide with owners (100 and 40 owners: two per lane,
    and packed or replicas)"""
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    lists, xt, xs, xn, w = grid_shape(99, 40, info)
    for l in (0, 5, 170, 171, 342):                       # the first point of a list's target range IS the first of its source range
        xt[lists[0][l] * 3:lists[0][l] * 3 + 3] = xs[lists[2][l] * 3:lists[2][l] * 3 + 3]
    rng = np.random.default_rng(5)
    xs2, xt2 = r32(rng, 140 * 3, 0.0), r32(rng, 200 * 3, 0.0)
    xt2[:64 * 3] = xs2[:64 * 3]                           # targets 0 .. 63 are sources 0 .. 63 (of the first owner range), and
    xt2[64 * 3:104 * 3] = xs2[100 * 3:]                   # targets 64 .. 103 the 40 sources of the second
    lists2 = [i8(0, 64, 0, 64), i8(64, 136, 64, 136), i8(0, 0, 100, 100), i8(100, 100, 40, 40)]
    xn2 = r32(rng, 140 * info["nd"]) if info["nd"] else None
    w2 = r32(rng, 200 * info["k1"])
    for ls, a, b, n, ww in ((lists, xt, xs, xn, w), (lists2, xt2, xs2, xn2, w2)):
        ref = expected(name, ls, a, b, n, ww, ctx)
        for dt in DTS:
            g, _ = transposed(name, dt, ls, a, b, n, ww, ctx)
            assert np.all(np.isfinite(g)) and rel_l2(g, ref) <= TOL[dt], (dt, rel_l2(g, ref))


def test_adjoint_identity_against_the_forward_list_entry():
    """|<w, L f> - <L^T w, f>| <= tol (|w| |L f| + |L^T w| |f|) on the lists and clouds of tests/golden/lists_manifest.json, whose forward results
    tests/test_lists.py pins to the reference's golden outputs; tol is the rel-L2 bound of the case (Cauchy-Schwarz on the two rel-L2 bounds)"""
    from test_lists import CASES, case_data, tol
    for c in CASES:
        info = sctl_amd.kernel_info(c["kernel"])
        lists, xt, xs, xn, f, ctx = case_data(c, info)
        w = (np.random.default_rng(c["seed"] + 50).random(c["Nt"] * info["k1"]) - 0.5).astype(xt.dtype)
        plan = sctl_amd.ListsPlan(c["kernel"], xt.dtype, *lists, c["Nt"], c["Ns"], ctx=ctx, directions="both")
        u = plan.eval_host(xt, xs, xn, f, digits=c["digits"]).astype(np.longdouble)
        g = plan.eval_transpose_host(xt, xs, xn, w, digits=c["digits"]).astype(np.longdouble)
        assert plan.transpose_info()["pairs"] == plan.pairs == c["pairs"]
        plan.close()
        wl, fl = w.astype(np.longdouble), f.astype(np.longdouble)
        nrm = lambda a: float(np.sqrt((a * a).sum()))
        lhs, rhs, bound = float(wl @ u), float(g @ fl), tol(c) * (nrm(wl) * nrm(u) + nrm(g) * nrm(fl))
        print("%s %s: <w, L f> = %.17g, <L^T w, f> = %.17g, |difference| %.3e, bound %.3e" % (c["key"], c["kernel"], lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound, c["key"]


@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxT", "Helmholtz3D-FxU"])
def test_one_list_is_the_dense_transposed_sum(name):
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    for Ns, Nt in ((300, 1000), (129, 65)):
        rng = np.random.default_rng(Ns)
        xt, xs, w = r32(rng, Nt * 3, 0.0), r32(rng, Ns * 3, 0.0), r32(rng, Nt * info["k1"])
        xn = r32(rng, Ns * info["nd"]) if info["nd"] else None
        one = [i8(0), i8(Nt), i8(0), i8(Ns)]
        for dt in DTS:
            a = sctl_amd.eval_lists_transpose_host(name, *one, *as_dt(dt, xt, xs, xn, w), ctx=ctx)
            b = sctl_amd.eval_transpose_host(name, *as_dt(dt, xt, xs, xn, w), ctx=ctx)
            assert rel_l2(a, b) <= 2 * TOL[dt], (Ns, Nt, dt, rel_l2(a, b))


def test_accumulation_bit_identity_info_and_counters():
    import torch
    name = "Stokes3D-FxUP"
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, xn, w, ctx, ref = case(name, "grid-32")
    Nt, Ns = xt.size // 3, xs.size // 3
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, Nt, Ns, directions="both")
    ti = plan.transpose_info()
    assert ti["pairs"] == plan.pairs == int((lists[1] * lists[3]).sum()) and ti["target_ranges"] == 343 and ti["work_items"] > 0
    pc0 = sctl_amd.counters()["pair_interactions"]
    g = plan.eval_transpose_host(xt, xs, xn, w)
    assert sctl_amd.counters()["pair_interactions"] - pc0 == plan.pairs                               # the counters grow by the plan's pairs
    assert np.array_equal(plan.eval_transpose_host(xt, xs, xn, w), g)                                  # run to run: the same bits
    g0 = np.random.default_rng(1).random(Ns * info["k0"])
    assert rel_l2(plan.eval_transpose_host(xt, xs, xn, w, g_src=g0.copy()), ref + g0) <= 1e-12          # the host entry accumulates
    assert np.array_equal(plan.eval_transpose_host(xt, xs, xn, w, g_src=g0.copy()), g0 + g)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, w)]
    gd = plan.eval_transpose_device(*d)
    torch.cuda.synchronize()
    assert np.array_equal(gd.cpu().numpy(), g)                                                         # device entry against host entry: the same bits
    acc = torch.full((Ns * info["k0"],), 0.5, dtype=torch.float64, device="cuda")
    plan.eval_transpose_device(*d, g_src=acc)                                                          # ... and it accumulates: the kernel adds into g_src
    assert rel_l2(acc.cpu().numpy(), ref + 0.5) <= 1e-12
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gs = plan.eval_transpose_device(*d, stream=side)
    side.synchronize()
    assert np.array_equal(gs.cpu().numpy(), g)
    assert np.array_equal(sctl_amd.eval_lists_transpose_host(name, *lists, xt, xs, xn, w), g)          # the one-shot form
    plan.close()
    # self lists with equal counts: the two sides are the same plan with the names exchanged
    rng = np.random.default_rng(3)
    for max_pts in (6, 50, 150):
        cnt = rng.integers(1, max_pts + 1, 27)
        ls = grid_neighbour_lists(3, cnt, cnt)
        n = int(cnt.sum())
        p = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *ls, n, n, directions="both")
        assert p.transpose_info() == dict(pairs=p.pairs, work_items=p.work_items, target_ranges=p.source_ranges)
        p.close()


# ---- plugins ------------------------------------------------------------------------------------------------------------------------
LAM = 2.5


def test_plugin_with_pair_t_runs_the_transposed_lists(tmp_path_factory):
    from test_gpu_transpose import _ensure, numpy_yukawa_matrix
    name = "Yukawa3D-FxU-T"
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    for shape in ("grid-32", "edges"):
        seed = 900 + SHAPES.index(shape)
        lists, xt, xs, _, w = edge_shape(seed, info) if shape == "edges" else grid_shape(seed, 32, info)
        xt[lists[0][0] * 3:lists[0][0] * 3 + 3] = xs[lists[2][0] * 3:lists[2][0] * 3 + 3]      # one coincident pair
        ref = np.zeros(xs.size // 3, dtype=np.longdouble)
        for t0, tc, s0, sc in zip(*lists):
            ref[s0:s0 + sc] += numpy_yukawa_matrix(xt[t0 * 3:(t0 + tc) * 3], xs[s0 * 3:(s0 + sc) * 3], LAM) @ w[t0:t0 + tc].astype(np.longdouble)
        ref = ref.astype(np.float64)
        for dt in DTS:
            g, _ = transposed(name, dt, lists, xt, xs, None, w, ctx)
            assert rel_l2(g, ref) <= TOL[dt], (shape, dt, rel_l2(g, ref))


def test_plugin_without_pair_t_is_refused_and_still_runs_forward(tmp_path_factory):
    from test_gpu_transpose import _ensure, numpy_yukawa_matrix
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    lists, xt, xs, _, _ = grid_shape(41, 20, info)
    Nt, Ns = xt.size // 3, xs.size // 3
    for d in ("transpose", "both"):
        with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
            sctl_amd.ListsPlan(name, np.float64, *lists, Nt, Ns, ctx=ctx, directions=d)
    f = np.random.default_rng(3).random(Ns) - 0.5
    ref = np.zeros(Nt, dtype=np.longdouble)
    for t0, tc, s0, sc in zip(*lists):
        ref[t0:t0 + tc] += numpy_yukawa_matrix(xt[t0 * 3:(t0 + tc) * 3], xs[s0 * 3:(s0 + sc) * 3], LAM).T @ f[s0:s0 + sc].astype(np.longdouble)
    assert rel_l2(sctl_amd.eval_lists_host(name, *lists, xt, xs, None, f, ctx=ctx), ref.astype(np.float64)) <= 1e-12


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
def _small_plan(name, seed=8):
    import torch
    info = sctl_amd.kernel_info(name)
    rng = np.random.default_rng(seed)
    cs, ct = rng.integers(1, 7, 8), rng.integers(1, 7, 8)
    xs, xt = points_in_boxes(2, cs, rng), points_in_boxes(2, ct, rng)
    Ns, Nt = int(cs.sum()), int(ct.sum())
    plan = sctl_amd.ListsPlan(name, np.float64, *grid_neighbour_lists(2, ct, cs), Nt, Ns, directions="both")
    xn = torch.from_numpy(rng.random(Ns * info["nd"]) - 0.5).cuda() if info["nd"] else None
    v = torch.from_numpy(rng.random(Ns * info["k0"]) - 0.5).cuda().requires_grad_(True)
    return plan, torch.from_numpy(xt).cuda(), torch.from_numpy(xs).cuda(), xn, v


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-FxU"])
def test_autograd_gradcheck(name):
    """finite differences of lists_sum's output against its backward (the transposed list sum): a 2^3 grid with at most 6 points per box, fp64"""
    import torch
    from sctl_amd.autograd import lists_sum
    plan, xt, xs, xn, v = _small_plan(name)
    fn = lambda v_: lists_sum(plan, xt, xs, xn, v_)
    assert torch.autograd.gradcheck(fn, (v,), eps=1e-3, atol=1e-7, rtol=1e-7, nondet_tol=0.0)     # (linear in v: a large step has no truncation error)
    u = fn(v)
    u.square().sum().backward()
    assert torch.equal(v.grad, plan.eval_transpose_device(xt, xs, xn, (2 * u).detach()))          # bit-equal to the transposed entry on 2 u


def test_autograd_refusals():
    import torch
    from sctl_amd.autograd import lists_sum
    plan, xt, xs, xn, v = _small_plan("Laplace3D-FxU")
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_src requires grad"):
        lists_sum(plan, xt, xs.clone().requires_grad_(True), None, v)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_trg requires grad"):
        lists_sum(plan, xt.clone().requires_grad_(True), xs, None, v)
    fwd = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, i8(0), i8(xt.numel() // 3), i8(0), i8(xs.numel() // 3), xt.numel() // 3, xs.numel() // 3)
    with pytest.raises(sctl_amd.api.SctlAmdError, match='directions="both"'):
        lists_sum(fwd, xt, xs, None, v)
    (gv,) = torch.autograd.grad(lists_sum(plan, xt, xs, None, v).square().sum(), v, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gv.sum().backward()


# ---- C++ ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_lists_transpose(tmp_path):
    """tests/cpp/lists_transpose_driver.cpp: GenericKernel<...>::EvalListsTranspose against a loop of EvalTranspose over the lists (g++ -Wall -Werror)"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "lists_transpose_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
