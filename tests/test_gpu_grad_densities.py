"""Geometry gradients for several density / weight rows in one pass (sctl_amd_eval_grad_densities_*, sctl_amd/csrc/multi_grad_kernel.hpp) on the GPU.

Expected value throughout: the sum over the rows of tests/grad_truth.py's gradients(), torch's CPU autograd of the dense fp64 formula, on
fp32-representable inputs, so one truth serves both precisions.  g_trg, g_src and g_nrm are compared separately, each as rel-L2 against its own norm.
Bounds (tests/test_gpu_grad.py): fp64 <= 1e-12 at full precision and 10 * 10^-d at digits = d; fp32 <= 4 times the rel-L2 that the same
summed formula has in torch float32 on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2
from grad_truth import HELMHOLTZ_KS, gradients
from test_gpu_grad import SPEC_OWNERS, SPEC_STREAMED, as_dt, bounds_for, check, cloud, share_points

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
OUT = ("g_trg", "g_src", "g_nrm")


def m_max(name):
    return sctl_amd.plan_grad_densities(name, 0, 64, 300, 50)["rows_per_pass"]


def rows(seed, nd, n):
    """nd rows of n fp32-representable doubles"""
    rng = np.random.default_rng(seed)
    return (rng.random((nd, n)) - 0.5).astype(np.float32).astype(np.float64)


def summed(name, xt, xs, xn, F, W, c, dtype=None, lam=None):
    """the sum over the rows of the single truth, accumulated in the dtype it is evaluated in"""
    import torch
    dtype = dtype or torch.float64
    tot = None
    for f, w in zip(F, W):
        g = gradients(name, xt, xs, xn, f, w, c, lam=lam, dtype=dtype)[:3]
        tot = g if tot is None else tuple(None if a is None else a + b for a, b in zip(tot, g))
    return tot


_CASES = {}


def case(name, Nt, Ns, nd, ctx_key="default", shared=0):
    """inputs, the fp64 truth and torch-fp32's error against it, computed once per (kernel, shape, rows) and shared by the tests"""
    key = (name, Nt, Ns, nd, ctx_key, shared)
    if key not in _CASES:
        import torch
        info = sctl_amd.kernel_info(name)
        seed = 4000 + 17 * KERNELS.index(name) + Nt + Ns
        xt, xs, xn, _, _ = cloud(seed, Nt, Ns, info)
        if shared:
            share_points(xt, xs, shared, 5)
        F, W = rows(seed + 1, nd, Ns * info["k0"]), rows(seed + 2, nd, Nt * info["k1"])
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        c = None if ctx is None else tuple(ctx)
        ref = summed(name, xt, xs, xn, F, W, c)
        ref32 = summed(name, xt, xs, xn, F, W, c, dtype=torch.float32)
        err32 = [None if r is None else rel_l2(r32, r) for r, r32 in zip(ref, ref32)]
        _CASES[key] = (xt, xs, xn, F, W, ctx, ref, err32)
    return _CASES[key]


@pytest.mark.parametrize("dt,digits", [(np.float64, -1), (np.float64, 10), (np.float32, -1)], ids=["f64", "f64-d10", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_small_shape(name, dt, digits):
    """300 targets x 50 sources, the always-masked path: a full form, a partly filled form (3 rows on the form of 4) and a second pass (M_max + 1)"""
    mm = m_max(name)
    assert mm == (4 if name == "Stokes3D-FxT" else 8)
    for nd in sorted({2, 3, mm, mm + 1}):
        pl = sctl_amd.plan_grad_densities(name, 0, nd, 300, 50)
        assert pl["passes"] == (2 if nd > mm else 1)
        xt, xs, xn, F, W, ctx, ref, err32 = case(name, 300, 50, nd)
        got = sctl_amd.eval_grad_densities_host(name, *as_dt(dt, xt, xs, xn, F, W), digits=digits, ctx=ctx)
        assert all(g is None or g.dtype == dt for g in got)
        check("%s %s digits %d 300 x 50, %d rows" % (name, dt.__name__, digits, nd), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_ragged_shapes_with_shared_points(name, dt):
    """513 owners against 1100 streamed points on each side, 40 points shared between the sets, 3 rows: a ragged last tile, a ragged last workgroup,
    several splits through the reduce; the shared pairs contribute exactly 0, as in the truth"""
    for Nt, Ns in ((513, 1100), (1100, 513)):
        pl = sctl_amd.plan_grad_densities(name, 0 if dt == np.float64 else 1, 3, Nt, Ns)
        assert pl["trg"]["splits"] > 1 and pl["src"]["splits"] > 1, pl
        xt, xs, xn, F, W, ctx, ref, err32 = case(name, Nt, Ns, 3, shared=40)
        got = sctl_amd.eval_grad_densities_host(name, *as_dt(dt, xt, xs, xn, F, W), ctx=ctx)
        check("%s %s %d x %d, 40 shared, 3 rows" % (name, dt.__name__, Nt, Ns), got, ref, bounds_for(dt, -1, err32))


@pytest.mark.parametrize("name", KERNELS)
def test_several_splits(name):
    """300 owners against enough streamed points for more than one split, by the new plan, on each side; 4 rows"""
    for Nt, Ns in ((300, 2000), (2000, 300)):
        pl = sctl_amd.plan_grad_densities(name, 0, 4, Nt, Ns)
        assert pl["trg" if Nt == 300 else "src"]["splits"] > 1, pl
        xt, xs, xn, F, W, ctx, ref, err32 = case(name, Nt, Ns, 4)
        for dt in (np.float64, np.float32):
            got = sctl_amd.eval_grad_densities_host(name, *as_dt(dt, xt, xs, xn, F, W), ctx=ctx)
            check("%s %s %d x %d, 4 rows %s" % (name, dt.__name__, Nt, Ns, pl), got, ref, bounds_for(dt, -1, err32))


# ---- the unmasked pass and its repair -----------------------------------------------------------------------------------------------------
_SPEC = {}


def _spec_case(name, side, nd=3):
    """inputs, and the truth for the subset of the owners that tests/test_gpu_grad.py uses, against all streamed points"""
    if (name, side) not in _SPEC:
        import torch
        info = sctl_amd.kernel_info(name)
        Nt, Ns = (SPEC_OWNERS, SPEC_STREAMED) if side == 0 else (SPEC_STREAMED, SPEC_OWNERS)
        xt, xs, xn, _, _ = cloud(600 + KERNELS.index(name) + side, Nt, Ns, info)
        F, W = rows(700 + side, nd, Ns * info["k0"]), rows(800 + side, nd, Nt * info["k1"])
        t, s = share_points(xt, xs, 40, 7)
        own = t if side == 0 else s
        sub = np.unique(np.r_[own, 0:8, 254:258, SPEC_OWNERS - 20:SPEC_OWNERS])       # the shared owners, a workgroup boundary, the ragged last workgroup
        ctx = ctx_for(name)
        c = None if ctx is None else tuple(ctx)
        pick = lambda a, k: None if a is None else a.reshape(-1, k)[sub].ravel().copy()
        pick_rows = lambda A, k: np.stack([pick(a, k) for a in A])
        sub_args = (pick(xt, 3), xs, xn, F, pick_rows(W, info["k1"])) if side == 0 else (xt, pick(xs, 3), pick(xn, 3), pick_rows(F, info["k0"]), W)
        keep = (lambda g: (g[0], None, None)) if side == 0 else (lambda g: (None, g[1], g[2]))
        ref = keep(summed(name, *sub_args, c))
        ref32 = keep(summed(name, *sub_args, c, dtype=torch.float32))
        err32 = [None if r is None else rel_l2(r32, r) for r, r32 in zip(ref, ref32)]
        _SPEC[(name, side)] = (xt, xs, xn, F, W, ctx, sub, ref, err32)
    return _SPEC[(name, side)]


@pytest.mark.parametrize("side", [0, 1], ids=["target-owned", "source-owned"])
@pytest.mark.parametrize("name", KERNELS)
def test_unmasked_pass_and_repair(name, side):
    """Each split holds at least four tiles, so tiles run unmasked, and 40 shared points send some of them through the compare and the masked
    re-run; 3 rows on the form of 4, so the empty row meets the poisoned tiles too.  Both precisions against the truth of some 70 owners (all shared
    ones among them) over all streamed points; the rest of the result must be finite."""
    import torch
    Nt, Ns = (SPEC_OWNERS, SPEC_STREAMED) if side == 0 else (SPEC_STREAMED, SPEC_OWNERS)
    pl = sctl_amd.plan_grad_densities(name, 0, 3, Nt, Ns)["trg" if side == 0 else "src"]
    assert -(-(-(-SPEC_STREAMED // 256)) // pl["splits"]) >= 4, pl
    xt, xs, xn, F, W, ctx, sub, ref, err32 = _spec_case(name, side)
    want = ("trg",) if side == 0 else (("src", "nrm") if xn is not None else ("src",))
    idx = (sub[:, None] * 3 + np.arange(3)).ravel()
    for dt in (np.float64, np.float32):
        d = [None if a is None else torch.from_numpy(a.astype(dt)).cuda() for a in (xt, xs, xn, F, W)]
        res = [None if g is None else g.cpu().numpy() for g in sctl_amd.eval_grad_densities_device(name, *d, want=want, ctx=ctx)]
        assert all(g is None or np.all(np.isfinite(g)) for g in res)
        check("%s side %d %s %s" % (name, side, dt.__name__, pl), [None if g is None else g[idx] for g in res], ref, bounds_for(dt, -1, err32))


@pytest.mark.parametrize("k", HELMHOLTZ_KS, ids=["complex-one-reduction", "real-one-reduction", "complex-two-reductions", "re0-two-reductions"])
def test_helmholtz_wavenumbers(k):
    """every table form and variant the forward kernel has, 3 rows, 300 x 50"""
    name = "Helmholtz3D-FxU"
    xt, xs, xn, F, W, ctx, ref, err32 = case(name, 300, 50, 3, k)
    for dt, digits in ((np.float64, -1), (np.float64, 10), (np.float32, -1)):
        got = sctl_amd.eval_grad_densities_host(name, *as_dt(dt, xt, xs, xn, F, W), digits=digits, ctx=ctx)
        check("Helmholtz k %s %s digits %d, 3 rows" % (k, dt.__name__, digits), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("name", KERNELS)
def test_one_row_is_the_single_entry_and_no_row_does_nothing(name):
    xt, xs, xn, F, W, ctx, ref, _ = case(name, 513, 1100, 3, shared=40)
    for dt in (np.float64, np.float32):
        a = as_dt(dt, xt, xs, xn, F, W)
        one = sctl_amd.eval_grad_densities_host(name, a[0], a[1], a[2], a[3][:1], a[4][:1], ctx=ctx)
        single = sctl_amd.eval_grad_host(name, a[0], a[1], a[2], a[3][0], a[4][0], ctx=ctx)
        assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(one, single)), name
        g0 = [None if r is None else np.full(r.size, 7.0, dtype=dt) for r in ref]
        for acc in (True, False):
            got = sctl_amd.eval_grad_densities_host(name, a[0], a[1], a[2], a[3][:0], a[4][:0], *g0, ctx=ctx, accumulate=acc)
            assert all(g is None or (g is b and bool((g == 7.0).all())) for g, b in zip(got, g0)), (name, acc)


@pytest.mark.parametrize("name", KERNELS)
def test_bit_identical_repeats(name):
    """three runs of one ragged shape with another kernel launched in between: the same bits"""
    import torch
    xt, xs, xn, F, W, ctx, ref, _ = case(name, 513, 1100, 3, shared=40)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, F, W)]
    runs = []
    for _ in range(3):
        runs.append(sctl_amd.eval_grad_densities_device(name, *d, ctx=ctx))
        other = sctl_amd.eval_grad_densities_device("Stokes3D-FxU", d[0], d[1], None, torch.ones((2, 1100 * 3), dtype=torch.float64, device="cuda"),
                                                    torch.ones((2, 513 * 3), dtype=torch.float64, device="cuda"))
        assert all(bool(torch.isfinite(g).all()) for g in other if g is not None)
    for r in runs[1:]:
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(r, runs[0])), name


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-DxU", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"])
def test_outputs_asked_for_alone(name):
    """each output alone is bit for bit the same output of the full call, and a buffer not asked for stays untouched"""
    import torch
    xt, xs, xn, F, W, ctx, ref, _ = case(name, 513, 1100, 3, shared=40)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, F, W)]
    full = sctl_amd.eval_grad_densities_device(name, *d, ctx=ctx)
    for i, what in enumerate(("trg", "src", "nrm")):
        if full[i] is None:
            continue
        bufs = [torch.full_like(g, 7.0) if g is not None else None for g in full]
        bufs[i] = torch.zeros_like(full[i])
        one = sctl_amd.eval_grad_densities_device(name, *d, g_trg=bufs[0], g_src=bufs[1], g_nrm=bufs[2], want=(what,), ctx=ctx)
        assert [j for j, g in enumerate(one) if g is not None] == [i]
        assert one[i] is bufs[i] and torch.equal(one[i], full[i]), (name, what)
        assert all(b is None or j == i or bool((b == 7.0).all()) for j, b in enumerate(bufs)), (name, what)


def test_accumulate_overwrite_generic_kernel_and_counters():
    name = "Stokes3D-DxU"
    nd = 3
    xt, xs, xn, F, W, ctx, ref, _ = case(name, 300, 50, nd)
    rng = np.random.default_rng(5)
    g0 = [rng.random(r.size) - 0.5 for r in ref]
    acc = sctl_amd.eval_grad_densities_host(name, xt, xs, xn, F, W, *[g.copy() for g in g0])
    check("host, accumulate", acc, [a + b for a, b in zip(g0, ref)], [1e-12] * 3)
    check("host, overwrite", sctl_amd.eval_grad_densities_host(name, xt, xs, xn, F, W, *[g.copy() for g in g0], accumulate=False), ref, [1e-12] * 3)
    K = sctl_amd.GenericKernel(name)
    fresh = K.EvalGradDensities(xt, xs, xn, F, W, np.zeros(5), None, np.zeros(7))           # wrong sizes (or None): fresh zeroed results
    check("GenericKernel.EvalGradDensities, resized", fresh, ref, [1e-12] * 3)
    again = K.EvalGradDensities(xt, xs, xn, F, W, *fresh)                                     # right sizes: accumulated into
    assert all(a is b for a, b in zip(again, fresh))
    check("GenericKernel.EvalGradDensities, accumulated", again, [2 * r for r in ref], [1e-12] * 3)
    # counters: nd * Nt * Ns pairs per side launched
    flops = sctl_amd.kernel_info(name)["flops"]
    for want, sides in ((("trg",), 1), (("src",), 1), (("nrm",), 1), (("src", "nrm"), 1), (("trg", "src", "nrm"), 2)):
        sctl_amd.reset_counters()
        sctl_amd.eval_grad_densities_host(name, xt, xs, xn, F, W, want=want)
        c = sctl_amd.counters()
        assert c["pair_interactions"] == sides * nd * 300 * 50 and c["sctl_flops"] == sides * nd * 300 * 50 * flops, (want, c)


_CUT_CHILD = r"""
import sys
import numpy as np
import sctl_amd
z = np.load(sys.argv[1], allow_pickle=True)
out = {}
for key in z["keys"]:
    name, shape, dt = key.split("|")
    a = [z["%s|%s|%d" % (name, shape, i)] for i in range(5)]
    a = [None if x.ndim == 0 else x.astype(dt) for x in a]
    ctx = z[name + "|ctx"]
    real = 0 if dt == "float64" else 1
    Nt, Ns = a[0].size // 3, a[1].size // 3
    pl = sctl_amd.plan_grad_densities(name, real, 3, Nt, Ns)
    width = 6 if a[2] is not None else 3
    assert pl["trg"]["splits"] > 1 and pl["trg"]["workspace_bytes"] == pl["trg"]["splits"] * 256 * 3 * np.dtype(dt).itemsize, pl
    assert pl["src"]["splits"] > 1 and pl["src"]["workspace_bytes"] == pl["src"]["splits"] * 256 * width * np.dtype(dt).itemsize, pl
    g = sctl_amd.eval_grad_densities_host(name, *a, ctx=None if ctx.ndim == 0 else ctx)
    for what, x in zip(("trg", "src", "nrm"), g):
        if x is not None:
            out[key + "|" + what] = x
np.savez(sys.argv[2], **out)
"""


def test_owners_cut_into_several_launches(tmp_path):
    """The cut of the owners that keeps the partial sums under 2 GB, with the bound lowered to one workgroup's 256 owners in a fresh process (one child
    for all kernels): 513 and 1100 owners, bit for bit the single launch of this process"""
    data, keys, whole = {}, [], {}
    none = np.array(0.0)
    for name in KERNELS:
        for Nt, Ns in ((513, 1100), (1100, 513)):
            xt, xs, xn, F, W, ctx, ref, _ = case(name, Nt, Ns, 3, shared=40)
            shape = "%dx%d" % (Nt, Ns)
            for i, a in enumerate((xt, xs, xn, F, W)):
                data["%s|%s|%d" % (name, shape, i)] = none if a is None else a
            data[name + "|ctx"] = none if ctx is None else ctx
            for dt in (np.float64, np.float32):
                key = "%s|%s|%s" % (name, shape, np.dtype(dt).name)
                keys.append(key)
                whole[key] = sctl_amd.eval_grad_densities_host(name, *as_dt(dt, xt, xs, xn, F, W), ctx=ctx)
    data["keys"] = np.array(keys)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, **data)
    env = dict(os.environ, SCTL_AMD_TRANSPOSE_WORKSPACE="1")
    p = subprocess.run([sys.executable, "-c", _CUT_CHILD, inp, outp], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    cut = np.load(outp)
    for key in keys:
        for what, g in zip(("trg", "src", "nrm"), whole[key]):
            assert (g is None and key + "|" + what not in cut) or np.array_equal(cut[key + "|" + what], g), (key, what)


def test_plugin_with_pair_g_and_no_pair_gm_goes_row_by_row(tmp_path):
    from test_gpu_grad import LAM, YUKAWA_G
    name = "Yukawa3D-FxU-G"
    try:
        sctl_amd.kernel_id(name)
    except KeyError:
        src, so, libdir = str(tmp_path / "yukawa_g_kernel.hip"), str(tmp_path / "libyukawa_g_kernel.so"), os.path.join(ROOT, "sctl_amd")
        open(src, "w").write(YUKAWA_G)
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), src, "-o", so,
                        "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir], check=True)
        assert sctl_amd.load_plugin(so) == [name]
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    nd = 3
    pl = sctl_amd.plan_grad_densities(name, 0, nd, 1100, 513)
    assert pl["rows_per_pass"] == 1 and pl["passes"] == nd, pl
    for Nt, Ns in ((300, 50), (1100, 513)):
        xt, xs, _, _, _ = cloud(31, Nt, Ns, info)
        xt[:3] = xs[3:6]
        F, W = rows(41, nd, Ns), rows(42, nd, Nt)
        ref = summed(name, xt, xs, None, F, W, None, lam=LAM)
        sctl_amd.reset_counters()
        got = sctl_amd.eval_grad_densities_host(name, xt, xs, None, F, W, ctx=ctx)
        assert sctl_amd.counters()["pair_interactions"] == 2 * nd * Nt * Ns
        check("plugin %d x %d, %d rows" % (Nt, Ns, nd), got, ref, [1e-12] * 3)


def test_plugin_without_pair_g_is_refused(tmp_path_factory):
    from test_gpu_transpose import _ensure
    name = "Yukawa3D-FxU-T"                       # pair and pair_t, no pair_g
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    x = np.random.default_rng(3).random(300)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_g"):
        sctl_amd.eval_grad_densities_host(name, x, x + 2.0, None, np.ones((2, 100)), np.ones((2, 100)), ctx=np.array([2.5]))
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_g"):
        sctl_amd.plan_grad_densities(name, 0, 2, 100, 100)


def test_device_entry_on_a_side_stream():
    import torch
    name = "Laplace3D-FDxUdU"
    xt, xs, xn, F, W, ctx, ref, _ = case(name, 513, 1100, 3, shared=40)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, F, W)]
        g = [torch.zeros(n, dtype=torch.float64, device="cuda") for n in (513 * 3, 1100 * 3, 1100 * 3)]
        out = sctl_amd.eval_grad_densities_device(name, *d, *g, stream=st)
    st.synchronize()
    assert all(a is b for a, b in zip(out, g))
    check("side stream", [x.cpu().numpy() for x in out], ref, [1e-12] * 3)


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------
def test_kernel_sum_densities_geometry():
    """the gradients of U.square().sum() with respect to r_trg, r_src, n_src and V_src on 60 x 50 points, 3 rows, against torch's autograd of the
    dense formula, for the stresslet; only r_src requiring grad launches the source pass alone; a double backward raises"""
    import torch
    from grad_truth import kernel_blocks
    from sctl_amd.autograd import kernel_sum_densities, kernel_sum_densities_geometry
    name, nd, Nt, Ns = "Stokes3D-DxU", 3, 60, 50
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, _, _ = cloud(11, Nt, Ns, info)
    V = rows(12, nd, Ns * info["k0"])
    cpu = [torch.from_numpy(a).view(-1, 3).clone().requires_grad_(True) for a in (xt, xs, xn)]
    Vc = torch.from_numpy(V).view(nd, Ns, info["k0"]).clone().requires_grad_(True)
    U = torch.einsum("tsjk,msj->mtk", kernel_blocks(name, cpu[0], cpu[1], cpu[2]), Vc)
    U.square().sum().backward()
    dev = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (xt, xs, xn, V)]
    Ug = kernel_sum_densities_geometry(name, *dev)
    assert Ug.shape == (nd, Nt * info["k1"]) and rel_l2(Ug.detach().cpu().numpy().ravel(), U.detach().numpy().ravel()) <= 1e-12
    Ug.square().sum().backward()
    for what, a, b in zip(("r_trg", "r_src", "n_src", "V_src"), dev, cpu + [Vc]):
        err = rel_l2(a.grad.cpu().numpy().ravel(), b.grad.numpy().ravel())
        print("%s d/d%s: rel-L2 %.2e" % (name, what, err))
        assert a.grad.shape == a.shape and err <= 1e-12, (name, what, err)
    v = dev[3].detach().clone().requires_grad_(True)
    kernel_sum_densities(name, dev[0].detach(), dev[1].detach(), dev[2].detach(), v).square().sum().backward()
    assert torch.equal(v.grad, dev[3].grad)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="densities only.*kernel_sum_densities_geometry"):
        kernel_sum_densities(name, dev[0], dev[1].detach(), dev[2].detach(), v)
    # only r_src requires grad: the backward is one source-owned pass, nd * Nt * Ns pairs
    x = dev[1].detach().clone().requires_grad_(True)
    L = kernel_sum_densities_geometry(name, dev[0].detach(), x, dev[2].detach(), dev[3].detach()).square().sum()
    sctl_amd.reset_counters()
    L.backward()
    assert sctl_amd.counters()["pair_interactions"] == nd * Nt * Ns
    assert rel_l2(x.grad.cpu().numpy().ravel(), cpu[1].grad.numpy().ravel()) <= 1e-12
    x = dev[0].detach().clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(kernel_sum_densities_geometry(name, x, dev[1].detach(), dev[2].detach(), v).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- C++ --------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_grad_densities_against_the_rows_one_at_a_time(tmp_path):
    """tests/cpp/grad_densities_driver.cpp: GenericKernel<Stokes3D_DxU>::EvalGradDensities (g++ -Wall -Werror) against the sum of EvalGrad calls per
    row, to 1e-12 of the largest entry, and a second call accumulated"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "grad_densities_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
