"""The transposed kernel sum g_src += A^T w_trg (sctl_amd_eval_transpose_*, include/sctl_amd/device/eval_transpose_kernel.hpp) on the GPU.

Expected value throughout: M . w in numpy long double, M from sctl_amd_kernel_matrix_host at full precision — the (Ns*K0) x (Nt*K1) matrix the
existing suite pins against the reference (generic-kernel.txx:191-307), which zeroes coincident pairs.  The inputs are fp32-representable doubles,
so one expected value serves the fp64 and the fp32 run of a shape.  Tolerances are the project's own: fp64 rel-L2 <= 1e-12, fp32
<= 2e-5 against the fp64 expected value, digits = d <= 10 * 10^-d.  For a plugin kernel the expected value is the functor written in numpy."""
import os
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
# (owners Ns, streamed Nt): one lane; the workgroup boundary 255 / 257 / 513 owners; the 256-record tile 255 / 256 / 257 / 1000 streamed;
# few owners against many streamed: 16 splits (the XCD-owned mapping: a multiple of 8) and 157 splits (the plain one), both through the reduce
SHAPES = [(1, 300), (255, 255), (257, 256), (513, 257), (300, 1000), (64, 4096), (64, 40000)]
SPLIT_SHAPES = {(64, 4096): 16, (64, 40000): 157}
TOL = {np.float64: 1e-12, np.float32: 2e-5}


def cloud(seed, Nt, Ns, info):
    """fp32-representable doubles: targets, sources, normals, target weights"""
    rng = np.random.default_rng(seed)
    r32 = lambda n, shift=0.5: (rng.random(n) - shift).astype(np.float32).astype(np.float64)     # rounded to fp32 LAST: exactly representable
    xt, xs = r32(Nt * 3, 0.0), r32(Ns * 3, 0.0)
    xn = r32(Ns * info["nd"]) if info["nd"] else None
    return xt, xs, xn, r32(Nt * info["k1"])


def expected(name, xt, xs, xn, w, ctx=None, block=4000):
    """M . w in long double, M = KernelMatrix at full precision, formed a block of targets at a time"""
    info = sctl_amd.kernel_info(name)
    Nt, k1 = xt.size // 3, info["k1"]
    g = np.zeros(xs.size // 3 * info["k0"], dtype=np.longdouble)
    for t0 in range(0, Nt, block):
        t1 = min(Nt, t0 + block)
        M = sctl_amd.kernel_matrix_host(name, xt[t0 * 3:t1 * 3].copy(), xs, xn, ctx=ctx)
        g += M.astype(np.longdouble) @ w[t0 * k1:t1 * k1].astype(np.longdouble)
    return g.astype(np.float64)


_CASES = {}


def case(name, shape, ctx_key="default"):
    """inputs and expected value of (kernel, shape), computed once and shared by the fp64, fp32 and digits tests"""
    key = (name, shape, ctx_key)
    if key not in _CASES:
        info = sctl_amd.kernel_info(name)
        Ns, Nt = shape
        xt, xs, xn, w = cloud(1000 + 17 * KERNELS.index(name) + Ns + Nt, Nt, Ns, info)
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        _CASES[key] = (xt, xs, xn, w, ctx, expected(name, xt, xs, xn, w, ctx))
    return _CASES[key]


def as_dt(dt, *arrays):
    return [None if a is None else a.astype(dt) for a in arrays]


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_parity_with_kernel_matrix(name, dt):
    real = 0 if dt == np.float64 else 1
    for shape in SHAPES:
        Ns, Nt = shape
        xt, xs, xn, w, ctx, ref = case(name, shape)
        if shape in SPLIT_SHAPES:
            pl = sctl_amd.plan_transpose(name, real, Nt, Ns)
            assert pl["splits"] == SPLIT_SHAPES[shape] and pl["splits"] >= 8 and pl["workspace_bytes"] == pl["splits"] * ref.size * dt().itemsize, pl
        g = sctl_amd.eval_transpose_host(name, *as_dt(dt, xt, xs, xn, w), ctx=ctx)
        err = rel_l2(g, ref)
        print("%s %s owners %d streamed %d: rel-L2 %.2e" % (name, dt.__name__, Ns, Nt, err))
        assert g.dtype == dt and np.all(np.isfinite(g)) and err <= TOL[dt], (name, shape, err)


@pytest.mark.parametrize("digits", [3, 10])
@pytest.mark.parametrize("name", KERNELS)
def test_digits(name, digits):
    for shape in ((300, 1000), (64, 4096)):
        xt, xs, xn, w, ctx, ref = case(name, shape)
        for dt in (np.float64,) + ((np.float32,) if digits == 3 else ()):     # fp32 cannot reach 10 * 10^-10: test_f32_high_digits runs its mode 1
            g = sctl_amd.eval_transpose_host(name, *as_dt(dt, xt, xs, xn, w), digits=digits, ctx=ctx)
            err = rel_l2(g, ref)
            print("%s %s digits %d %s: rel-L2 %.2e" % (name, dt.__name__, digits, shape, err))
            assert err <= 10.0 * 10.0 ** -digits, (name, shape, dt, err)


@pytest.mark.parametrize("name", KERNELS)
def test_coincident_points(name):
    """targets == sources at N = 600; a handful of shared points among 1000; one whole 256-record tile of shared points: KernelMatrix zeroes a
    coincident pair, so M . w is the expected value, and everything is finite"""
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    xt, xs, xn, w = cloud(77, 600, 600, info)
    sets = [(xs.copy(), xs, xn, w)]
    xt, xs, xn, w = cloud(78, 1000, 1000, info)
    for t, s in ((3, 900), (255, 0), (256, 1), (700, 700), (999, 513)):
        xt[t * 3:t * 3 + 3] = xs[s * 3:s * 3 + 3]
    sets.append((xt, xs, xn, w))
    xt, xs, xn, w = cloud(79, 1500, 700, info)
    xt[256 * 3:512 * 3] = xs[300 * 3:556 * 3]           # the second tile: every record coincides with an owner
    sets.append((xt, xs, xn, w))
    for xt, xs, xn, w in sets:
        ref = expected(name, xt, xs, xn, w, ctx)
        for dt in (np.float64, np.float32):
            g = sctl_amd.eval_transpose_host(name, *as_dt(dt, xt, xs, xn, w), ctx=ctx)
            assert np.all(np.isfinite(g)) and rel_l2(g, ref) <= TOL[dt], (name, dt, rel_l2(g, ref))


def test_accumulate_overwrite_and_empty():
    import torch
    name = "Stokes3D-FSxU"
    xt, xs, xn, w, ctx, ref = case(name, (300, 1000))
    g0 = np.random.default_rng(5).random(ref.size) - 0.5
    assert rel_l2(sctl_amd.eval_transpose_host(name, xt, xs, xn, w, g_src=g0.copy()), g0 + ref) <= 1e-12            # host, accumulate
    assert rel_l2(sctl_amd.eval_transpose_host(name, xt, xs, xn, w, g_src=g0.copy(), accumulate=False), ref) <= 1e-12   # host, overwrite
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, w)]
    g = torch.from_numpy(g0).cuda()
    out = sctl_amd.eval_transpose_device(name, d[0], d[1], None, d[2], g_src=g)                                       # device, into a pre-filled g_src
    assert out is g and rel_l2(g.cpu().numpy(), g0 + ref) <= 1e-12
    assert sctl_amd.GenericKernel(name).EvalTranspose(None, xt, xs, xn, w).shape == ref.shape
    # empty sets: nothing is touched
    e = np.zeros(0)
    keep = g0.copy()
    assert np.array_equal(sctl_amd.eval_transpose_host(name, e, xs, None, e, g_src=keep), g0)                        # Nt = 0
    assert np.array_equal(sctl_amd.eval_transpose_host(name, e, xs, None, e, g_src=keep, accumulate=False), g0)
    assert sctl_amd.eval_transpose_host(name, xt, e, None, w).size == 0                                               # Ns = 0
    ge = sctl_amd.eval_transpose_device(name, torch.zeros(0, dtype=torch.float64, device="cuda"), d[1], None, torch.zeros(0, dtype=torch.float64, device="cuda"), g_src=g)
    assert rel_l2(ge.cpu().numpy(), g0 + ref) <= 1e-12
    # counters: Nt * Ns pairs and Nt * Ns * FLOPS
    sctl_amd.reset_counters()
    sctl_amd.eval_transpose_host(name, xt, xs, xn, w)
    c = sctl_amd.counters()
    assert c["pair_interactions"] == 300 * 1000 and c["sctl_flops"] == 300 * 1000 * sctl_amd.kernel_info(name)["flops"]


@pytest.mark.parametrize("shared", [False, True], ids=["disjoint", "shared-points"])
@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxUP"])
def test_adjoint_identity_beyond_the_dense_matrix(name, shared):
    """<w, Eval(f)> == <EvalTranspose(w), f> at 20000 sources x 30000 targets, where each target split holds ten tiles: the unmasked pass runs.
    With shared points (scattered ones, and a whole tile of targets that are copies of one workgroup's sources) the same identity holds through
    the tile repair and the give-up-speculating path, because the forward evaluation zeroes those pairs too."""
    import torch
    info = sctl_amd.kernel_info(name)
    Ns, Nt = 20000, 30000
    pl = sctl_amd.plan_transpose(name, 0, Nt, Ns)
    ntile = -(-Nt // 256)
    assert -(-ntile // pl["splits"]) >= 4, pl                    # tiles per split: speculation is on
    xt, xs, xn, w = cloud(4242, Nt, Ns, info)
    f = np.random.default_rng(9).random(Ns * info["k0"]) - 0.5
    if shared:
        for t, s in ((5, 19000), (3000, 10), (29999, 257)):
            xt[t * 3:t * 3 + 3] = xs[s * 3:s * 3 + 3]
        xt[512 * 3:768 * 3] = xs[1024 * 3:1280 * 3]
    d = {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in dict(xt=xt, xs=xs, xn=xn, w=w, f=f).items()}
    Af = sctl_amd.eval_device(name, d["xt"], d["xs"], d["xn"], d["f"]).cpu().numpy().astype(np.longdouble)
    Atw = sctl_amd.eval_transpose_device(name, d["xt"], d["xs"], d["xn"], d["w"]).cpu().numpy().astype(np.longdouble)
    wl, fl = w.astype(np.longdouble), f.astype(np.longdouble)
    lhs, rhs, bound = np.sum(wl * Af), np.sum(Atw * fl), 1e-12 * np.sum(np.abs(wl * Af))
    print("%s shared=%s: <w, A f> = %.17g, <A^T w, f> = %.17g, |difference| %.3e, bound %.3e" % (name, shared, lhs, rhs, abs(lhs - rhs), bound))
    assert np.all(np.isfinite(Atw.astype(np.float64))) and abs(lhs - rhs) <= bound


# ---- two owners per lane, speculation on ------------------------------------------------------------------------------------------------------
T2_NS, T2_NT = 33068, 36000      # 64 full workgroups of 512 owners and one of 300 (its second owner row: 44 stored, 212 clamped); 140.6 tiles
_T2 = {}


def _t2_case(name, shared):
    """inputs, the fp64 forward sum A f, and M . w for a subset of the owners (both shared by the fp64 and the fp32 run)"""
    import torch
    if (name, shared) not in _T2:
        info = sctl_amd.kernel_info(name)
        Ns, Nt, k0 = T2_NS, T2_NT, info["k0"]
        xt, xs, xn, w = cloud(900 + KERNELS.index(name), Nt, Ns, info)
        f = np.random.default_rng(12).random(Ns * k0) - 0.5
        if shared:
            # a whole tile of targets on owners of workgroup 2 (both owner rows) and one more pair six tiles on: a repair, then the give-up;
            # single pairs on the clamped last workgroup's second row, on its first row, and in the last, partial tile
            xt[512 * 3:768 * 3] = xs[1100 * 3:1356 * 3]
            for t, s in ((2000, 1030), (5, Ns - 1), (9000, 33000), (Nt - 1, 300)):
                xt[t * 3:t * 3 + 3] = xs[s * 3:s * 3 + 3]
        # owners checked against the dense matrix: both rows of the first workgroup and their edges, the shared ones, the whole tail of the last
        sub = np.r_[0:4, 254:258, 510:514, 1028:1032, 1098:1102, 1354:1358, 32766:32770, 33000:33004, Ns - 46:Ns]
        ctx = ctx_for(name)
        gsub = expected(name, xt, xs.reshape(-1, 3)[sub].ravel(), None if xn is None else xn.reshape(-1, 3)[sub].ravel(), w, ctx)
        d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, f)]
        Af = sctl_amd.eval_device(name, *d, ctx=ctx).cpu().numpy().astype(np.longdouble)
        rows = (sub[:, None] * k0 + np.arange(k0)).ravel()
        _T2[(name, shared)] = (xt, xs, xn, w, f, ctx, Af, rows, gsub)
    return _T2[(name, shared)]


@pytest.mark.parametrize("shared", [False, True], ids=["disjoint", "shared-points"])
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_two_owners_per_lane_speculative(name, dt, shared):
    """The configuration the kernel is built for: two owners per lane (from 2^15 owners on) and enough tiles per split for the unmasked pass, the
    per-tile compare and the repair, for every kernel in both precisions, with and without shared points.  Two checks, since the dense matrix
    of the whole shape is out of reach: M . w for 78 owners (rel-L2 within the project's tolerance), and the adjoint identity against the
    fp64 forward sum over all of them.  Bound of the identity in fp64: 1e-12 sum |w_i (A f)_i|, as at 20000 x 30000.  In fp32 the transposed
    result may be off by 2e-5 in rel-L2, so by Cauchy-Schwarz <A^T w, f> by 2e-5 |A^T w| |f|; the fp64 side's bound is added."""
    import torch
    real = 0 if dt == np.float64 else 1
    pl = sctl_amd.plan_transpose(name, real, T2_NT, T2_NS)
    assert pl["src_per_lane"] == 2 and -(-(-(-T2_NT // 256)) // pl["splits"]) >= 4, pl
    xt, xs, xn, w, f, ctx, Af, rows, gsub = _t2_case(name, shared)
    d = [None if a is None else torch.from_numpy(a.astype(dt)).cuda() for a in (xt, xs, xn, w)]
    g = sctl_amd.eval_transpose_device(name, *d, ctx=ctx).cpu().numpy()
    assert g.dtype == dt and np.all(np.isfinite(g))
    err = rel_l2(g[rows].astype(np.float64), gsub)
    wl, fl, gl = w.astype(np.longdouble), f.astype(np.longdouble), g.astype(np.longdouble)
    lhs, rhs = np.sum(wl * Af), np.sum(gl * fl)
    bound = 1e-12 * np.sum(np.abs(wl * Af))
    if dt == np.float32:
        bound += 2e-5 * np.sqrt(np.sum(gl * gl) * np.sum(fl * fl))
    print("%s %s shared=%s %s: rel-L2 of %d owners %.2e; <w, A f> = %.17g, <A^T w, f> = %.17g, |difference| %.3e, bound %.3e"
          % (name, dt.__name__, shared, pl, rows.size, err, lhs, rhs, abs(lhs - rhs), bound))
    assert err <= TOL[dt], (name, dt, shared, err)
    assert abs(lhs - rhs) <= bound, (name, dt, shared, abs(lhs - rhs), bound)


@pytest.mark.parametrize("name", KERNELS)
def test_f32_high_digits(name):
    """fp32 with digits >= 8 takes the refined rsqrt (mode 1), fp32's best: no fp32 result can reach 10 * 10^-10, which is why test_digits asks
    it of fp64 only; the bound here is the fp32 tolerance of the full-precision run"""
    for shape in ((300, 1000), (64, 4096)):
        xt, xs, xn, w, ctx, ref = case(name, shape)
        g = sctl_amd.eval_transpose_host(name, *as_dt(np.float32, xt, xs, xn, w), digits=10, ctx=ctx)
        assert rel_l2(g, ref) <= TOL[np.float32], (name, shape, rel_l2(g, ref))


def test_bit_identical_repeat():
    name = "Stokes3D-FxU"
    xt, xs, xn, w, ctx, _ = case(name, (64, 40000))
    assert sctl_amd.plan_transpose(name, 1, 40000, 64)["splits"] > 1
    a = sctl_amd.eval_transpose_host(name, *as_dt(np.float32, xt, xs, xn, w))
    b = sctl_amd.eval_transpose_host(name, *as_dt(np.float32, xt, xs, xn, w))
    assert np.array_equal(a, b)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_owners_cut_into_several_launches(name, dt, monkeypatch):
    """The cut of the owners that keeps the partial sums under 2 GB, on small shapes: SCTL_AMD_TRANSPOSE_WORKSPACE lowers the bound so far that a
    launch holds one workgroup's 256 owners.  300 owners run as 256 + 44 over 4 splits, 513 as 256 + 256 + 1 over 2: the second and later launches
    offset x_s, n_s and g and reuse the workspace block with their own stride.  The result is M . w within the tolerance, and, the points being
    distinct, bit for bit the single launch's: an owner's sum does not depend on which launch computed it."""
    real = 0 if dt == np.float64 else 1
    for shape, splits in (((300, 1000), 4), ((513, 257), 2)):
        Ns, Nt = shape
        xt, xs, xn, w, ctx, ref = case(name, shape)
        args = as_dt(dt, xt, xs, xn, w)
        whole = sctl_amd.eval_transpose_host(name, *args, ctx=ctx)
        one = sctl_amd.plan_transpose(name, real, Nt, Ns)
        assert one["splits"] == splits and one["workspace_bytes"] == splits * ref.size * dt().itemsize, one
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", "1")
        try:
            pl = sctl_amd.plan_transpose(name, real, Nt, Ns)
            assert pl["splits"] == splits and pl["workspace_bytes"] == splits * 256 * (ref.size // Ns) * dt().itemsize, pl
            g = sctl_amd.eval_transpose_host(name, *args, ctx=ctx)
        finally:
            monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
        err = rel_l2(g, ref)
        print("%s %s owners %d in launches of 256, %d splits: rel-L2 %.2e" % (name, dt.__name__, Ns, splits, err))
        assert err <= TOL[dt] and np.array_equal(g, whole), (name, shape, err)


def test_owners_cut_with_two_owners_per_lane(monkeypatch):
    """the same cut where a workgroup holds 512 owners: 33068 owners in 64 launches of 512 and one of 300, against the single launch and M . w"""
    import torch
    name = "Stokes3D-FxUP"
    xt, xs, xn, w, f, ctx, Af, rows, gsub = _t2_case(name, False)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, w)]
    whole = sctl_amd.eval_transpose_device(name, *d, ctx=ctx).cpu().numpy()
    k0 = sctl_amd.kernel_info(name)["k0"]
    monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", "1")
    try:
        pl = sctl_amd.plan_transpose(name, 0, T2_NT, T2_NS)
        assert pl["src_per_lane"] == 2 and pl["workspace_bytes"] == pl["splits"] * 512 * k0 * 8, pl
        g = sctl_amd.eval_transpose_device(name, *d, ctx=ctx).cpu().numpy()
    finally:
        monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
    assert rel_l2(g[rows], gsub) <= 1e-12 and np.array_equal(g, whole)


@pytest.mark.parametrize("k", [(7.5, 0.3), (7.5, 0.0), (-3.0, 2.5), (0.0, 0.7)], ids=["complex-one-reduction", "real-one-reduction", "complex-two-reductions", "re0-two-reductions"])
def test_helmholtz_wavenumbers(k):
    """complex and real wavenumbers; Re k > 0 with small decay takes the one-reduction tables in fp64, the others the two-reduction form"""
    name = "Helmholtz3D-FxU"
    for shape in ((300, 1000), (64, 4096)):
        xt, xs, xn, w, ctx, ref = case(name, shape, k)
        for dt in (np.float64, np.float32):
            g = sctl_amd.eval_transpose_host(name, *as_dt(dt, xt, xs, xn, w), ctx=ctx)
            assert rel_l2(g, ref) <= TOL[dt], (k, shape, dt, rel_l2(g, ref))


def test_side_stream_device_entry():
    import torch
    name = "Laplace3D-FDxUdU"
    xt, xs, xn, w, ctx, ref = case(name, (513, 257))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, w)]
        g = sctl_amd.eval_transpose_device(name, *d, stream=st)
    st.synchronize()
    assert rel_l2(g.cpu().numpy(), ref) <= 1e-12


# ---- plugins ------------------------------------------------------------------------------------------------------------------------
LAM = 2.5


def _build_plugin(tmp, src):
    so = str(tmp / ("lib%s.so" % src))
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "plugin", src + ".hip"), "-o", so, "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir], check=True)
    return so


def _ensure(tmp_path_factory, name, src):
    try:
        sctl_amd.kernel_id(name)
    except KeyError:
        assert sctl_amd.load_plugin(_build_plugin(tmp_path_factory.mktemp(src), src)) == [name]


def numpy_yukawa_matrix(xt, xs, lam):
    d = xt.reshape(1, -1, 3) - xs.reshape(-1, 1, 3)
    r = np.sqrt((d * d).sum(-1)).astype(np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > 0, np.exp(-lam * r) / (4 * np.longdouble(np.pi) * r), 0)


def test_plugin_with_pair_t_matches_its_numpy_functor(tmp_path_factory):
    name = "Yukawa3D-FxU-T"
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    for Ns, Nt in ((257, 1000), (64, 4096)):
        xt, xs, _, w = cloud(31, Nt, Ns, info)
        xt[:3] = xs[3:6]
        M = numpy_yukawa_matrix(xt, xs, LAM)
        ref = (M @ w.astype(np.longdouble)).astype(np.float64)
        assert rel_l2(sctl_amd.eval_transpose_host(name, xt, xs, None, w, ctx=ctx), ref) <= 1e-12
        assert rel_l2(sctl_amd.eval_transpose_host(name, *as_dt(np.float32, xt, xs), None, w.astype(np.float32), ctx=ctx), ref) <= 2e-5
        f = np.random.default_rng(2).random(Ns) - 0.5
        assert rel_l2(sctl_amd.eval_host(name, xt, xs, None, f, ctx=ctx), (M.T @ f.astype(np.longdouble)).astype(np.float64)) <= 1e-12


def test_plugin_without_pair_t_is_refused_and_still_evaluates_forward(tmp_path_factory):
    name = "Yukawa3D-FxU"
    _ensure(tmp_path_factory, name, "yukawa_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    xt, xs, _, w = cloud(32, 200, 100, info)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        sctl_amd.eval_transpose_host(name, xt, xs, None, w, ctx=ctx)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):
        sctl_amd.plan_transpose(name, 0, 200, 100)
    f = np.random.default_rng(3).random(100) - 0.5
    ref = (numpy_yukawa_matrix(xt, xs, LAM).T @ f.astype(np.longdouble)).astype(np.float64)
    assert rel_l2(sctl_amd.eval_host(name, xt, xs, None, f, ctx=ctx), ref) <= 1e-12


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Stokes3D-FxU", "Laplace3D-FDxUdU"])
def test_autograd_gradcheck(name):
    """finite differences of a scalar function of kernel_sum's output against its backward (the transposed sum): 40 targets x 50 sources, fp64"""
    import torch
    from sctl_amd.autograd import kernel_sum
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, _ = cloud(11, 40, 50, info)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn)]
    v = torch.from_numpy(np.random.default_rng(4).random(50 * info["k0"]) - 0.5).cuda().requires_grad_(True)
    fn = lambda v_: kernel_sum(name, d[0], d[1], d[2], v_)
    assert torch.autograd.gradcheck(fn, (v,), eps=1e-3, atol=1e-7, rtol=1e-7, nondet_tol=0.0)     # (linear in v: a large step has no truncation error)
    u = fn(v)
    c = torch.from_numpy(np.random.default_rng(6).random(u.numel()) - 0.5).cuda()
    (u * c).sum().backward()
    ref = expected(name, xt, xs, xn, c.cpu().numpy())
    assert rel_l2(v.grad.cpu().numpy(), ref) <= 1e-12


def test_autograd_refuses_coordinate_gradients():
    import torch
    from sctl_amd.autograd import kernel_sum
    x = torch.rand(30, dtype=torch.float64, device="cuda")
    v = torch.rand(10, dtype=torch.float64, device="cuda", requires_grad=True)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_src requires grad"):
        kernel_sum("Laplace3D-FxU", x, x.clone().requires_grad_(True), None, v)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="r_trg requires grad"):
        kernel_sum("Laplace3D-FxU", x.clone().requires_grad_(True), x, None, v)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="n_src requires grad"):
        kernel_sum("Laplace3D-DxU", x, x, x.clone().requires_grad_(True), v)


def test_autograd_refuses_a_double_backward():
    """the backward is the transposed kernel, outside the graph: asking for a graph through it raises instead of giving a gradient without one"""
    import torch
    from sctl_amd.autograd import kernel_sum
    x = torch.rand(30, dtype=torch.float64, device="cuda")
    v = torch.rand(10, dtype=torch.float64, device="cuda", requires_grad=True)
    (gv,) = torch.autograd.grad(kernel_sum("Laplace3D-FxU", x, x + 2.0, None, v).square().sum(), v, create_graph=True)    # grad_u = 2 u has a graph
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gv.sum().backward()


# ---- C++ ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_transpose_adjoint_identity(tmp_path):
    """tests/cpp/transpose_driver.cpp: GenericKernel<...>::EvalTranspose against Eval through the adjoint identity (g++ -Wall -Werror)"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "transpose_driver")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
