"""Several weight vectors through the transposed kernel sum, G[m] += A^T W[m] (sctl_amd_eval_transpose_densities_*, sctl_amd/csrc/rows_kernel.hpp),
on the GPU.

Expected value of row m: M . w_m in numpy long double, M from sctl_amd_kernel_matrix_host at full precision, the inputs fp32-representable doubles as in
test_gpu_transpose.py, so one expected value serves the fp64 and the fp32 run of a shape.  Tolerances are the project's own: fp64 rel-L2
<= 1e-12, fp32 <= 2e-5, digits = d <= 10 * 10^-d, per row.  Shapes are (owners Ns, streamed Nt) with the owners placed around the workgroup's 256 * T, T read
from the plan of the form under test; row counts 2, 3, 5, 8, 11 run every form (2, 4, 8), a form with fewer rows than it holds, and a second pass."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2
from test_gpu_transpose import LAM, TOL, _ensure, as_dt, cloud

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
NDS = (2, 3, 5, 8, 11)
NDMAX = max(NDS)
STREAMED = (255, 256, 257, 1000)


def shapes_for(name, real, nd):
    """one owner; 256 T - 1, 256 T + 1 and 2 * 256 T + 1 owners against 255 / 256 / 257 streamed; 300 against 1000; 64 against 4096 (splits and the reduce)"""
    T = sctl_amd.plan_transpose_densities(name, real, nd, 1000, 1000)["src_per_lane"]
    assert T in (1, 2)
    g = 256 * T
    return [(1, 300), (g - 1, STREAMED[0]), (g + 1, STREAMED[1]), (2 * g + 1, STREAMED[2]), (300, STREAMED[3]), (64, 4096)]


_CASES = {}


def case(name, shape, ctx_key="default"):
    """inputs (NDMAX weight rows) and the expected NDMAX result rows of (kernel, shape), computed once and shared: a test takes the first nd rows"""
    key = (name, shape, ctx_key)
    if key not in _CASES:
        info = sctl_amd.kernel_info(name)
        Ns, Nt = shape
        xt, xs, xn, _ = cloud(2000 + 17 * KERNELS.index(name) + Ns + Nt, Nt, Ns, info)
        rng = np.random.default_rng(Ns * 7 + Nt)
        W = (rng.random((NDMAX, Nt * info["k1"])) - 0.5).astype(np.float32).astype(np.float64)
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        _CASES[key] = (xt, xs, xn, W, ctx, expected(name, xt, xs, xn, W, ctx))
    return _CASES[key]


def expected(name, xt, xs, xn, W, ctx=None):
    M = sctl_amd.kernel_matrix_host(name, xt, xs, xn, ctx=ctx)
    return (M.astype(np.longdouble) @ W.T.astype(np.longdouble)).T.astype(np.float64).copy()


def rows_err(G, ref):
    return max(rel_l2(G[m], ref[m]) for m in range(G.shape[0]))


def run(name, dt, xt, xs, xn, W, ctx, **kw):
    a = as_dt(dt, xt, xs, xn)
    return sctl_amd.eval_transpose_densities_host(name, a[0], a[1], a[2], np.ascontiguousarray(W.astype(dt)), ctx=ctx, **kw)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_parity_with_kernel_matrix(name, dt):
    real = 0 if dt == np.float64 else 1
    info = sctl_amd.kernel_info(name)
    for nd in NDS:
        for shape in shapes_for(name, real, nd):
            Ns, Nt = shape
            xt, xs, xn, W, ctx, ref = case(name, shape)
            pl = sctl_amd.plan_transpose_densities(name, real, nd, Nt, Ns)
            if shape == (64, 4096):       # the XCD-owned mapping and the reduce
                assert pl["splits"] >= 8 and pl["splits"] % 8 == 0, pl
                assert pl["workspace_bytes"] == pl["vectors_per_pass"] * pl["splits"] * Ns * info["k0"] * dt().itemsize, pl
            G = run(name, dt, xt, xs, xn, W[:nd], ctx)
            err = rows_err(G, ref[:nd])
            print("%s %s nd %d (%d per pass, %d passes) owners %d streamed %d: rel-L2 %.2e" % (name, dt.__name__, nd, pl["vectors_per_pass"], pl["passes"], Ns, Nt, err))
            assert G.dtype == dt and G.shape == (nd, Ns * info["k0"]) and np.all(np.isfinite(G)) and err <= TOL[dt], (name, nd, shape, err)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_rows_agree_with_single_calls(name, dt):
    real = 0 if dt == np.float64 else 1
    for nd in (5, 11):
        for shape in shapes_for(name, real, nd)[3:]:
            xt, xs, xn, W, ctx, _ = case(name, shape)
            G = run(name, dt, xt, xs, xn, W[:nd], ctx)
            a = as_dt(dt, xt, xs, xn)
            for m in range(nd):
                single = sctl_amd.eval_transpose_host(name, a[0], a[1], a[2], W[m].astype(dt), ctx=ctx)
                assert rel_l2(G[m], single) <= TOL[dt], (name, nd, shape, m, rel_l2(G[m], single))


@pytest.mark.parametrize("name", KERNELS)
def test_one_row_is_the_single_entry_and_no_row_is_nothing(name):
    L = sctl_amd.lib()
    info = sctl_amd.kernel_info(name)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    for shape in ((300, 1000), (64, 4096)):
        Ns, Nt = shape
        xt, xs, xn, W, ctx, _ = case(name, shape)
        for dt in (np.float64, np.float32):
            real = 0 if dt == np.float64 else 1
            a = as_dt(dt, xt, xs, xn)
            w = np.ascontiguousarray(W[:1].astype(dt))
            G = sctl_amd.eval_transpose_densities_host(name, a[0], a[1], a[2], w, ctx=ctx)
            assert np.array_equal(G[0], sctl_amd.eval_transpose_host(name, a[0], a[1], a[2], w[0], ctx=ctx))
            one, single = sctl_amd.plan_transpose_densities(name, real, 1, Nt, Ns), sctl_amd.plan_transpose(name, real, Nt, Ns)
            assert one["vectors_per_pass"] == 1 and one["passes"] == 1 and all(one[k] == single[k] for k in single), (one, single)
            g0 = (np.random.default_rng(3).random(Ns * info["k0"]) - 0.5).astype(dt)
            g = g0.copy()
            cb = 0 if ctx is None else ctx.nbytes
            for acc in (1, 0):
                assert L.sctl_amd_eval_transpose_densities_host(info["id"], real, 0, Nt, Ns, p(a[0]), p(a[1]), p(a[2]), p(w), p(g), acc, -1, p(ctx), cb, 0) == 0
            assert np.array_equal(g, g0)


@pytest.mark.parametrize("digits", [3, 10])
@pytest.mark.parametrize("name", KERNELS)
def test_digits(name, digits):
    for nd in (3, 8):
        for shape in ((300, 1000), (64, 4096)):
            xt, xs, xn, W, ctx, ref = case(name, shape)
            for dt in (np.float64,) + ((np.float32,) if digits == 3 else ()):     # fp32 cannot reach 10 * 10^-10
                G = run(name, dt, xt, xs, xn, W[:nd], ctx, digits=digits)
                err = rows_err(G, ref[:nd])
                print("%s %s digits %d nd %d %s: rel-L2 %.2e" % (name, dt.__name__, digits, nd, shape, err))
                assert err <= 10.0 * 10.0 ** -digits, (name, shape, dt, nd, err)
    xt, xs, xn, W, ctx, ref = case(name, (300, 1000))                             # fp32 with digits 10: the refined rsqrt, fp32's best
    assert rows_err(run(name, np.float32, xt, xs, xn, W[:5], ctx, digits=10), ref[:5]) <= TOL[np.float32]


@pytest.mark.parametrize("k", [(7.5, 0.3), (7.5, 0.0), (-3.0, 2.5), (0.0, 0.7)], ids=["complex-one-reduction", "real-one-reduction", "complex-two-reductions", "re0-two-reductions"])
def test_helmholtz_wavenumbers(k):
    """the wavenumbers test_gpu_transpose.py runs: every launch-uniform variant of pair_tm, in every form"""
    name = "Helmholtz3D-FxU"
    for shape in ((300, 1000), (64, 4096)):
        xt, xs, xn, W, ctx, ref = case(name, shape, k)
        for nd in (2, 3, 8):
            for dt in (np.float64, np.float32):
                err = rows_err(run(name, dt, xt, xs, xn, W[:nd], ctx), ref[:nd])
                assert err <= TOL[dt], (k, shape, nd, dt, err)


@pytest.mark.parametrize("name", KERNELS)
def test_coincident_points(name):
    """targets == sources at N = 600; a handful of shared points among 1000; one whole 256-record tile of shared points: KernelMatrix zeroes a
    coincident pair, so M . w is the expected value, and everything is finite"""
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    rng = np.random.default_rng(8)
    weights = lambda Nt: (rng.random((5, Nt * info["k1"])) - 0.5).astype(np.float32).astype(np.float64)
    xt, xs, xn, _ = cloud(77, 600, 600, info)
    sets = [(xs.copy(), xs, xn, weights(600))]
    xt, xs, xn, _ = cloud(78, 1000, 1000, info)
    for t, s in ((3, 900), (255, 0), (256, 1), (700, 700), (999, 513)):
        xt[t * 3:t * 3 + 3] = xs[s * 3:s * 3 + 3]
    sets.append((xt, xs, xn, weights(1000)))
    xt, xs, xn, _ = cloud(79, 1500, 700, info)
    xt[256 * 3:512 * 3] = xs[300 * 3:556 * 3]           # the second tile: every record coincides with an owner
    sets.append((xt, xs, xn, weights(1500)))
    for xt, xs, xn, W in sets:
        ref = expected(name, xt, xs, xn, W, ctx)
        for dt in (np.float64, np.float32):
            for nd in (2, 5):
                G = run(name, dt, xt, xs, xn, W[:nd], ctx)
                assert np.all(np.isfinite(G)) and rows_err(G, ref[:nd]) <= TOL[dt], (name, dt, nd, rows_err(G, ref[:nd]))


@pytest.mark.parametrize("name", KERNELS)
def test_adjoint_identity_with_the_forward_densities(name):
    """<W_m, (A V)_m> == <(A^T W)_m, V_m> per row, A V from sctl_amd_eval_densities_host: fp64, relative 1e-12 of sum |w_i (A v)_i|"""
    info = sctl_amd.kernel_info(name)
    for shape in ((300, 1000), (64, 4096)):
        Ns, Nt = shape
        xt, xs, xn, W, ctx, _ = case(name, shape)
        nd = 5
        V = np.random.default_rng(10).random((nd, Ns * info["k0"])) - 0.5
        AV = sctl_amd.eval_densities_host(name, xt, xs, xn, V, ctx=ctx).astype(np.longdouble)
        AtW = run(name, np.float64, xt, xs, xn, W[:nd], ctx).astype(np.longdouble)
        for m in range(nd):
            wl, vl = W[m].astype(np.longdouble), V[m].astype(np.longdouble)
            lhs, rhs, bound = np.sum(wl * AV[m]), np.sum(AtW[m] * vl), 1e-12 * np.sum(np.abs(wl * AV[m]))
            assert abs(lhs - rhs) <= bound, (name, shape, m, lhs, rhs, bound)


def test_accumulate_overwrite_side_stream_empty_and_counters():
    import torch
    name = "Stokes3D-FSxU"
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, W, ctx, ref = case(name, (300, 1000))
    nd = 5
    W, ref = np.ascontiguousarray(W[:nd]), ref[:nd]
    G0 = np.random.default_rng(5).random(ref.shape) - 0.5
    assert rows_err(sctl_amd.eval_transpose_densities_host(name, xt, xs, xn, W, G_src=G0.copy()), G0 + ref) <= 1e-12               # host, accumulate
    assert rows_err(sctl_amd.eval_transpose_densities_host(name, xt, xs, xn, W, G_src=G0.copy(), accumulate=False), ref) <= 1e-12   # host, overwrite
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, W)]
        G = torch.from_numpy(G0).cuda()
        out = sctl_amd.eval_transpose_densities_device(name, d[0], d[1], None, d[2], G_src=G, stream=st)                           # device, pre-filled, side stream
    st.synchronize()
    assert out is G and rows_err(G.cpu().numpy(), G0 + ref) <= 1e-12
    assert sctl_amd.GenericKernel(name).EvalTransposeDensities(None, xt, xs, xn, W).shape == ref.shape
    # empty sets: nothing is touched
    e = np.zeros(0)
    keep = G0.copy()
    assert np.array_equal(sctl_amd.eval_transpose_densities_host(name, e, xs, None, np.zeros((nd, 0)), G_src=keep), G0)             # Nt = 0
    assert np.array_equal(sctl_amd.eval_transpose_densities_host(name, e, xs, None, np.zeros((nd, 0)), G_src=keep, accumulate=False), G0)
    assert sctl_amd.eval_transpose_densities_host(name, xt, e, None, W).shape == (nd, 0)                                           # Ns = 0
    # counters: nd * Nt * Ns pairs
    sctl_amd.reset_counters()
    sctl_amd.eval_transpose_densities_host(name, xt, xs, xn, W)
    c = sctl_amd.counters()
    assert c["pair_interactions"] == nd * 300 * 1000 and c["sctl_flops"] == nd * 300 * 1000 * info["flops"]
    sctl_amd.reset_counters()
    xt2, xs2, xn2, W2, _, _ = case(name, (64, 4096))
    sctl_amd.eval_transpose_densities_host(name, xt2, xs2, xn2, W2)             # 11 rows: two passes
    assert sctl_amd.counters()["pair_interactions"] == NDMAX * 64 * 4096


def test_bit_identical_repeat():
    for name, dt in (("Stokes3D-FxU", np.float32), ("Helmholtz3D-FxU", np.float64)):
        xt, xs, xn, W, ctx, _ = case(name, (64, 4096))
        assert sctl_amd.plan_transpose_densities(name, 0 if dt == np.float64 else 1, NDMAX, 4096, 64)["splits"] > 1
        runs = [run(name, dt, xt, xs, xn, W, ctx) for _ in range(6)]
        assert all(np.array_equal(runs[0], r) for r in runs[1:])


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import sctl_amd
z = np.load(sys.argv[2])
out = {}
for name in ("Laplace3D-DxU", "Stokes3D-FxUP"):
    info = sctl_amd.kernel_info(name)
    for tag, dt in (("f64", np.float64), ("f32", np.float32)):
        for nd in (2, 5):
            xt, xs, W = (z[name + k].astype(dt) for k in ("xt", "xs", "W"))
            xn = z[name + "xn"].astype(dt) if info["nd"] else None
            pl = sctl_amd.plan_transpose_densities(name, 0 if dt == np.float64 else 1, nd, xt.size // 3, xs.size // 3)
            assert pl["splits"] == 4 and pl["workspace_bytes"] == pl["vectors_per_pass"] * 4 * 256 * pl["src_per_lane"] * info["k0"] * dt().itemsize, pl
            out["%s_%s_%d" % (name, tag, nd)] = sctl_amd.eval_transpose_densities_host(name, xt, xs, xn, np.ascontiguousarray(W[:nd]))
np.savez(sys.argv[3], **out)
"""


def test_owners_cut_into_several_launches_in_a_fresh_process(tmp_path):
    """SCTL_AMD_TRANSPOSE_WORKSPACE lowered so far that a launch holds one workgroup's owners: 513 owners against 1000 streamed (4 splits) run as
    256 + 256 + 1 or 512 + 1, the later launches offsetting x_s, n_s and every row of G.  Bit for bit the single launch's result."""
    data, whole = {}, {}
    for name in ("Laplace3D-DxU", "Stokes3D-FxUP"):
        info = sctl_amd.kernel_info(name)
        xt, xs, xn, W, ctx, ref = case(name, (513, 1000))
        data.update({name + "xt": xt, name + "xs": xs, name + "W": W[:5]})
        if xn is not None:
            data[name + "xn"] = xn
        for tag, dt in (("f64", np.float64), ("f32", np.float32)):
            for nd in (2, 5):
                pl = sctl_amd.plan_transpose_densities(name, 0 if dt == np.float64 else 1, nd, 1000, 513)
                assert pl["splits"] == 4 and pl["workspace_bytes"] == pl["vectors_per_pass"] * 4 * 513 * info["k0"] * dt().itemsize, pl
                G = run(name, dt, xt, xs, xn, W[:nd], ctx)
                assert rows_err(G, ref[:nd]) <= TOL[dt]
                whole["%s_%s_%d" % (name, tag, nd)] = G
    np.savez(str(tmp_path / "in.npz"), **data)
    env = dict(os.environ, SCTL_AMD_TRANSPOSE_WORKSPACE="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    cut = np.load(str(tmp_path / "out.npz"))
    assert sorted(cut.files) == sorted(whole)
    for key, G in whole.items():
        assert np.array_equal(cut[key], G), key


def test_plugin_rows_are_single_calls(tmp_path_factory):
    """a registered kernel with pair_t has no form of several weight vectors: its rows go one at a time through the single path, bit for bit"""
    name = "Yukawa3D-FxU-T"
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    for Ns, Nt in ((257, 1000), (64, 4096)):
        xt, xs, _, _ = cloud(31, Nt, Ns, info)
        W = np.random.default_rng(1).random((3, Nt)) - 0.5
        pl = sctl_amd.plan_transpose_densities(name, 0, 3, Nt, Ns)
        assert pl["vectors_per_pass"] == 1 and pl["passes"] == 3, pl
        G = sctl_amd.eval_transpose_densities_host(name, xt, xs, None, W, ctx=ctx)
        for m in range(3):
            assert np.array_equal(G[m], sctl_amd.eval_transpose_host(name, xt, xs, None, W[m].copy(), ctx=ctx))


def test_plugin_without_pair_t_is_refused(tmp_path_factory):
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    x = np.random.default_rng(0).random(300)
    for nd in (1, 3):
        with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
            sctl_amd.eval_transpose_densities_host(name, x, x, None, np.ones((nd, 100)), ctx=np.array([LAM]))
        with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
            sctl_amd.plan_transpose_densities(name, 0, nd, 100, 100)


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Stokes3D-FxUP", "Laplace3D-DxU"])
def test_autograd_kernel_sum_densities(name):
    """Row m of V.grad after U.square().sum().backward() is M . (2 u_m), with M the dense (Ns*K0) x (Nt*K1) matrix and u_m = M^T v_m, both formed in
    long double from the matrix: within 1e-12"""
    import torch
    from sctl_amd.autograd import kernel_sum_densities
    info = sctl_amd.kernel_info(name)
    Nt, Ns, nd = 70, 50, 3
    xt, xs, xn, _ = cloud(11, Nt, Ns, info)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn)]
    Vn = np.random.default_rng(4).random((nd, Ns * info["k0"])) - 0.5
    V = torch.from_numpy(Vn).cuda().requires_grad_(True)
    U = kernel_sum_densities(name, d[0], d[1], d[2], V)
    assert U.shape == (nd, Nt * info["k1"])
    U.square().sum().backward()
    M = sctl_amd.kernel_matrix_host(name, xt, xs, xn).astype(np.longdouble)
    u = Vn.astype(np.longdouble) @ M                       # (nd, Nt*K1)
    ref = (2 * u @ M.T).astype(np.float64)                 # (nd, Ns*K0)
    assert rows_err(U.detach().cpu().numpy(), u.astype(np.float64)) <= 1e-12
    assert rows_err(V.grad.cpu().numpy(), ref) <= 1e-12


def test_autograd_refuses_coordinate_gradients_and_a_double_backward():
    import torch
    from sctl_amd.autograd import kernel_sum_densities
    x = torch.rand(30, dtype=torch.float64, device="cuda")
    V = torch.rand((3, 10), dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_src requires grad"):
        kernel_sum_densities("Laplace3D-FxU", x, x.clone().requires_grad_(True), None, V)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_trg requires grad"):
        kernel_sum_densities("Laplace3D-FxU", x.clone().requires_grad_(True), x, None, V)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="n_src requires grad"):
        kernel_sum_densities("Laplace3D-DxU", x, x, x.clone().requires_grad_(True), V)
    (gV,) = torch.autograd.grad(kernel_sum_densities("Laplace3D-FxU", x, x + 2.0, None, V).square().sum(), V, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gV.sum().backward()


# ---- C++ ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_transpose_densities_matches_the_python_entry(tmp_path):
    """tests/cpp/transpose_densities_driver.cpp (g++ -Wall -Werror): GenericKernel<...>::EvalTransposeDensities on drand48 inputs, bit for bit what
    sctl_amd.eval_transpose_densities_host gives for the same inputs"""
    from sctl_amd.rand48 import Rand48
    from test_cpp_host import _build
    exe = _build(tmp_path, "transpose_densities_driver")
    Nt, Ns, nd = 1000, 600, 5
    out = str(tmp_path / "g.bin")
    p = subprocess.run([exe, str(Nt), str(Ns), str(nd), out], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    g = Rand48(0)
    xt, xs = g.drand48(Nt * 3) - 0.5, g.drand48(Ns * 3) - 0.5
    W = (g.drand48(nd * Nt * 4) - 0.5).reshape(nd, Nt * 4)
    G = sctl_amd.eval_transpose_densities_host("Stokes3D-FxUP", xt, xs, None, W)
    assert np.array_equal(np.fromfile(out, dtype=np.float64).reshape(nd, Ns * 3), G)
