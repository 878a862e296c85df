"""Coordinate and normal gradients of a kernel sum (sctl_amd_eval_grad_*, include/sctl_amd/device/eval_grad_kernel.hpp) on the GPU.

Expected value throughout: torch's CPU autograd of the dense fp64 formula of tests/grad_truth.py, which tests/test_grad_cpu.py ties to the
reference's KernelMatrix.  Every test compares g_trg, g_src and g_nrm separately, each as rel-L2 against its own norm.  The inputs are
fp32-representable doubles, so one truth serves the fp64 and the fp32 run of a shape.  Bounds: fp64 <= 1e-12 at full precision and 10 * 10^-d at
digits = d.  fp32 has no fitted number: the same formula and its autograd in torch float32 on the same inputs has some rel-L2
against the fp64 truth, and the kernel is allowed 4 times that (the rule of test_hip_fp32_kernel_values_one_pair_at_a_time_against_long_double:
an approximate reciprocal square root and more multiplications per power)."""
import os
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2
from grad_truth import HELMHOLTZ_KS, gradients

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
OUT = ("g_trg", "g_src", "g_nrm")


def cloud(seed, Nt, Ns, info):
    """fp32-representable doubles: targets, sources, normals, densities, target weights"""
    rng = np.random.default_rng(seed)
    r32 = lambda n, shift=0.5: (rng.random(n) - shift).astype(np.float32).astype(np.float64)
    xt, xs = r32(Nt * 3, 0.0), r32(Ns * 3, 0.0)
    xn = r32(Ns * 3) if info["nd"] else None
    return xt, xs, xn, r32(Ns * info["k0"]), r32(Nt * info["k1"])


def share_points(xt, xs, n, seed):
    """n targets become copies of n sources (distinct ones on both sides, spread over both sets)"""
    rng = np.random.default_rng(seed)
    t, s = rng.choice(xt.size // 3, n, replace=False), rng.choice(xs.size // 3, n, replace=False)
    xt.reshape(-1, 3)[t] = xs.reshape(-1, 3)[s]
    return t, s


_CASES = {}


def case(name, Nt, Ns, ctx_key="default", shared=0):
    """inputs, the fp64 truth and torch-fp32's error against it, computed once per (kernel, shape) and shared by the tests"""
    key = (name, Nt, Ns, ctx_key, shared)
    if key not in _CASES:
        info = sctl_amd.kernel_info(name)
        xt, xs, xn, f, w = cloud(2000 + 17 * KERNELS.index(name) + Nt + Ns, Nt, Ns, info)
        if shared:
            share_points(xt, xs, shared, 5)
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        c = None if ctx is None else tuple(ctx)
        ref = gradients(name, xt, xs, xn, f, w, c)[:3]
        import torch
        ref32 = gradients(name, xt, xs, xn, f, w, c, dtype=torch.float32)[:3]
        err32 = [None if r is None else rel_l2(r32, r) for r, r32 in zip(ref, ref32)]
        _CASES[key] = (xt, xs, xn, f, w, ctx, ref, err32)
    return _CASES[key]


def as_dt(dt, *arrays):
    return [None if a is None else a.astype(dt) for a in arrays]


def check(tag, got, ref, bounds):
    """each output against its own truth and bound; prints every figure before it asserts"""
    errs = []
    for what, g, r, b in zip(OUT, got, ref, bounds):
        assert (g is None) == (r is None), (tag, what)
        if g is not None:
            errs.append((what, rel_l2(g, r), b, bool(np.all(np.isfinite(g)))))
    print("%s: %s" % (tag, ", ".join("%s rel-L2 %.2e (bound %.2e)" % e[:3] for e in errs)))
    for what, err, b, finite in errs:
        assert finite and err <= b, (tag, what, err, b)


def bounds_for(dt, digits, err32):
    if dt == np.float64:
        return [1e-12 if digits < 0 else 10.0 * 10.0 ** -digits] * 3
    return [None if e is None else 4.0 * e for e in err32]


@pytest.mark.parametrize("dt,digits", [(np.float64, -1), (np.float64, 10), (np.float32, -1), (np.float32, 9)], ids=["f64", "f64-d10", "f32", "f32-d9"])
@pytest.mark.parametrize("name", KERNELS)
def test_small_shape(name, dt, digits):
    """300 targets x 50 sources: one tile per split, the always-masked path"""
    xt, xs, xn, f, w, ctx, ref, err32 = case(name, 300, 50)
    got = sctl_amd.eval_grad_host(name, *as_dt(dt, xt, xs, xn, f, w), digits=digits, ctx=ctx)
    assert all(g is None or g.dtype == dt for g in got)
    check("%s %s digits %d 300 x 50" % (name, dt.__name__, digits), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_ragged_shapes_with_shared_points(name, dt):
    """513 owners against 1100 streamed points on each side, 40 points shared between the sets: a ragged last tile, a ragged last workgroup, several
    splits through the reduce; the shared pairs contribute exactly 0, as in the truth.  (The planner gives such a shape one tile per split, so
    its tiles run masked: test_unmasked_pass_and_repair has the shape at which they do not.)"""
    for Nt, Ns in ((513, 1100), (1100, 513)):
        xt, xs, xn, f, w, ctx, ref, err32 = case(name, Nt, Ns, shared=40)
        got = sctl_amd.eval_grad_host(name, *as_dt(dt, xt, xs, xn, f, w), ctx=ctx)
        check("%s %s %d x %d, 40 shared" % (name, dt.__name__, Nt, Ns), got, ref, bounds_for(dt, -1, err32))


@pytest.mark.parametrize("name", KERNELS)
def test_several_splits(name):
    """300 owners against enough streamed points for more than one split, by the plan, on each side"""
    for Nt, Ns in ((300, 2000), (2000, 300)):
        pl = sctl_amd.plan_grad(name, 0, Nt, Ns)
        assert pl["trg" if Nt == 300 else "src"]["splits"] > 1, pl
        xt, xs, xn, f, w, ctx, ref, err32 = case(name, Nt, Ns)
        for dt in (np.float64, np.float32):
            got = sctl_amd.eval_grad_host(name, *as_dt(dt, xt, xs, xn, f, w), ctx=ctx)
            check("%s %s %d x %d %s" % (name, dt.__name__, Nt, Ns, pl), got, ref, bounds_for(dt, -1, err32))


# ---- the unmasked pass and its repair -----------------------------------------------------------------------------------------------------
SPEC_OWNERS, SPEC_STREAMED = 20000 + 77, 13 * 4 * 256 + 300     # 79 workgroups -> 13 splits of >= 4 tiles (asserted from the plan)
_SPEC = {}


def _spec_case(name, side):
    """inputs, and the truth for a subset of the owners against all streamed points (the dense truth of the whole shape is out of reach)"""
    if (name, side) not in _SPEC:
        info = sctl_amd.kernel_info(name)
        Nt, Ns = (SPEC_OWNERS, SPEC_STREAMED) if side == 0 else (SPEC_STREAMED, SPEC_OWNERS)
        xt, xs, xn, f, w = cloud(300 + KERNELS.index(name) + side, Nt, Ns, info)
        t, s = share_points(xt, xs, 40, 7)
        own = t if side == 0 else s
        sub = np.unique(np.r_[own, 0:8, 254:258, SPEC_OWNERS - 20:SPEC_OWNERS])       # the shared owners, a workgroup boundary, the ragged last workgroup
        ctx = ctx_for(name)
        c = None if ctx is None else tuple(ctx)
        pick = lambda a, k: None if a is None else a.reshape(-1, k)[sub].ravel().copy()
        import torch
        sub_args = (pick(xt, 3), xs, xn, f, pick(w, info["k1"])) if side == 0 else (xt, pick(xs, 3), pick(xn, 3), pick(f, info["k0"]), w)
        keep = (lambda g: (g[0], None, None)) if side == 0 else (lambda g: (None, g[1], g[2]))
        ref = keep(gradients(name, *sub_args, c))
        ref32 = keep(gradients(name, *sub_args, c, dtype=torch.float32))
        err32 = [None if r is None else rel_l2(r32, r) for r, r32 in zip(ref, ref32)]
        _SPEC[(name, side)] = (xt, xs, xn, f, w, ctx, sub, ref, err32)
    return _SPEC[(name, side)]


@pytest.mark.parametrize("side", [0, 1], ids=["target-owned", "source-owned"])
@pytest.mark.parametrize("name", KERNELS)
def test_unmasked_pass_and_repair(name, side):
    """Each split holds at least four tiles, so tiles run unmasked, and 40 shared points send some of them through the compare and the masked
    re-run.  Both precisions against the truth of some 70 owners (all shared ones among them) over all streamed points, the dense truth of the
    whole shape being out of reach; the rest of the fp64 result must be finite."""
    import torch
    Nt, Ns = (SPEC_OWNERS, SPEC_STREAMED) if side == 0 else (SPEC_STREAMED, SPEC_OWNERS)
    pl = sctl_amd.plan_grad(name, 0, Nt, Ns)["trg" if side == 0 else "src"]
    assert -(-(-(-SPEC_STREAMED // 256)) // pl["splits"]) >= 4, pl
    xt, xs, xn, f, w, ctx, sub, ref, err32 = _spec_case(name, side)
    want = ("trg",) if side == 0 else (("src", "nrm") if xn is not None else ("src",))
    rows = (sub[:, None] * 3 + np.arange(3)).ravel()
    for dt in (np.float64, np.float32):
        d = [None if a is None else torch.from_numpy(a.astype(dt)).cuda() for a in (xt, xs, xn, f, w)]
        res = [None if g is None else g.cpu().numpy() for g in sctl_amd.eval_grad_device(name, *d, want=want, ctx=ctx)]
        assert all(g is None or np.all(np.isfinite(g)) for g in res)
        check("%s side %d %s %s" % (name, side, dt.__name__, pl), [None if g is None else g[rows] for g in res], ref, bounds_for(dt, -1, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_owners_cut_into_several_launches(name, dt, monkeypatch):
    """The cut of the owners that keeps the partial sums under 2 GB, with the bound lowered to one workgroup's 256 owners: bit for bit the single launch"""
    real = 0 if dt == np.float64 else 1
    for Nt, Ns in ((513, 1100), (1100, 513)):
        xt, xs, xn, f, w, ctx, ref, err32 = case(name, Nt, Ns, shared=40)
        args = as_dt(dt, xt, xs, xn, f, w)
        whole = sctl_amd.eval_grad_host(name, *args, ctx=ctx)
        one = sctl_amd.plan_grad(name, real, Nt, Ns)
        assert one["trg"]["splits"] > 1 and one["src"]["splits"] > 1, one
        monkeypatch.setenv("SCTL_AMD_TRANSPOSE_WORKSPACE", "1")
        try:
            pl = sctl_amd.plan_grad(name, real, Nt, Ns)
            assert pl["trg"]["workspace_bytes"] == pl["trg"]["splits"] * 256 * 3 * dt().itemsize, pl
            assert pl["src"]["workspace_bytes"] == pl["src"]["splits"] * 256 * (6 if xn is not None else 3) * dt().itemsize, pl
            cut = sctl_amd.eval_grad_host(name, *args, ctx=ctx)
        finally:
            monkeypatch.delenv("SCTL_AMD_TRANSPOSE_WORKSPACE")
        for what, a, b in zip(OUT, cut, whole):
            assert (a is None and b is None) or np.array_equal(a, b), (name, what, Nt, Ns)


@pytest.mark.parametrize("k", HELMHOLTZ_KS, ids=["complex-one-reduction", "real-one-reduction", "complex-two-reductions", "re0-two-reductions"])
def test_helmholtz_wavenumbers(k):
    """the wavenumbers of the transposed tests: every table form and variant the forward kernel has"""
    name = "Helmholtz3D-FxU"
    for Nt, Ns in ((300, 50), (513, 1100)):
        xt, xs, xn, f, w, ctx, ref, err32 = case(name, Nt, Ns, k, shared=0 if Nt == 300 else 40)
        for dt, digits in ((np.float64, -1), (np.float64, 10), (np.float32, -1)):
            got = sctl_amd.eval_grad_host(name, *as_dt(dt, xt, xs, xn, f, w), digits=digits, ctx=ctx)
            check("Helmholtz k %s %s digits %d %d x %d" % (k, dt.__name__, digits, Nt, Ns), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("name", KERNELS)
def test_translation_invariance(name):
    """L depends on differences of coordinates only: sum_t g_trg + sum_s g_src = 0, to 1e-12 of sum |g_trg| + sum |g_src| in fp64"""
    xt, xs, xn, f, w, ctx, ref, _ = case(name, 1100, 513, shared=40)
    g_trg, g_src, _ = sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, ctx=ctx)
    total = g_trg.reshape(-1, 3).astype(np.longdouble).sum(0) + g_src.reshape(-1, 3).astype(np.longdouble).sum(0)
    mag = np.abs(g_trg).sum() + np.abs(g_src).sum()
    print("%s: |sum| %s of %.3e" % (name, np.abs(total).astype(np.float64), mag))
    assert np.all(np.abs(total) <= 1e-12 * mag), (name, total, mag)


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-DxU", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"])
def test_null_outputs(name):
    """each output alone is bit for bit the same output of the full call, and a buffer not asked for stays untouched"""
    import torch
    xt, xs, xn, f, w, ctx, ref, _ = case(name, 513, 1100, shared=40)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, w)]
    full = sctl_amd.eval_grad_device(name, *d, ctx=ctx)
    for i, what in enumerate(("trg", "src", "nrm")):
        if full[i] is None:
            continue
        bufs = [torch.full_like(g, 7.0) if g is not None else None for g in full]
        bufs[i] = torch.zeros_like(full[i])
        one = sctl_amd.eval_grad_device(name, *d, g_trg=bufs[0], g_src=bufs[1], g_nrm=bufs[2], want=(what,), ctx=ctx)
        assert [j for j, g in enumerate(one) if g is not None] == [i]
        assert one[i] is bufs[i] and torch.equal(one[i], full[i]), (name, what)
        assert all(b is None or j == i or bool((b == 7.0).all()) for j, b in enumerate(bufs)), (name, what)


def test_accumulate_overwrite_empty_and_counters():
    import torch
    name = "Stokes3D-DxU"
    xt, xs, xn, f, w, ctx, ref, _ = case(name, 300, 50)
    rng = np.random.default_rng(5)
    g0 = [rng.random(r.size) - 0.5 for r in ref]
    acc = sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, *[g.copy() for g in g0])
    check("host, accumulate", acc, [a + b for a, b in zip(g0, ref)], [1e-12] * 3)
    check("host, overwrite", sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, *[g.copy() for g in g0], accumulate=False), ref, [1e-12] * 3)
    check("GenericKernel.EvalGrad", sctl_amd.GenericKernel(name).EvalGrad(xt, xs, xn, f, w), ref, [1e-12] * 3)
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, w)]
    g = [torch.from_numpy(a).cuda() for a in g0]
    out = sctl_amd.eval_grad_device(name, *d, *g)
    assert all(a is b for a, b in zip(out, g))
    check("device, into pre-filled outputs", [a.cpu().numpy() for a in g], [a + b for a, b in zip(g0, ref)], [1e-12] * 3)
    # empty sets: nothing is touched
    e = np.zeros(0)
    keep = [a.copy() for a in g0]
    got = sctl_amd.eval_grad_host(name, e, xs, xn, f, e, None, keep[1], keep[2], want=("src", "nrm"))               # Nt = 0
    assert np.array_equal(got[1], g0[1]) and np.array_equal(got[2], g0[2])
    got = sctl_amd.eval_grad_host(name, e, xs, xn, f, e, None, keep[1], keep[2], want=("src", "nrm"), accumulate=False)
    assert np.array_equal(got[1], g0[1]) and np.array_equal(got[2], g0[2])
    got = sctl_amd.eval_grad_host(name, xt, e, e, e, w, keep[0], want=("trg",))                                      # Ns = 0
    assert np.array_equal(got[0], g0[0])
    # counters: Nt * Ns pairs per pass launched
    flops = sctl_amd.kernel_info(name)["flops"]
    for want, passes in ((("trg",), 1), (("src",), 1), (("nrm",), 1), (("src", "nrm"), 1), (("trg", "src", "nrm"), 2)):
        sctl_amd.reset_counters()
        sctl_amd.eval_grad_host(name, xt, xs, xn, f, w, want=want)
        c = sctl_amd.counters()
        assert c["pair_interactions"] == passes * 300 * 50 and c["sctl_flops"] == passes * 300 * 50 * flops, (want, c)


def test_side_stream_and_bit_identical_repeat():
    """the device entry on a side stream; two runs with another kernel between them give the same bits"""
    import torch
    name = "Laplace3D-FDxUdU"
    xt, xs, xn, f, w, ctx, ref, _ = case(name, 513, 1100, shared=40)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, w)]
        a = sctl_amd.eval_grad_device(name, *d, stream=st)
        other = sctl_amd.eval_grad_device("Stokes3D-FxU", d[0], d[1], None, torch.ones(1100 * 3, dtype=torch.float64, device="cuda"),
                                          torch.ones(513 * 3, dtype=torch.float64, device="cuda"), stream=st)
        b = sctl_amd.eval_grad_device(name, *d, stream=st)
    st.synchronize()
    assert all(bool(torch.isfinite(g).all()) for g in other if g is not None)
    check("side stream", [g.cpu().numpy() for g in a], ref, [1e-12] * 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxUP", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"])
def test_kernel_sum_geometry(name):
    """the gradients of u.square().sum() with respect to r_trg, r_src, n_src and v_src on 60 x 50 points against torch's autograd of the dense
    formula; v_src.grad bit for bit kernel_sum's; a double backward raises"""
    import torch
    from grad_truth import kernel_blocks
    from sctl_amd.autograd import kernel_sum, kernel_sum_geometry
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, f, _ = cloud(11, 60, 50, info)
    ctx = ctx_for(name)
    c = None if ctx is None else tuple(ctx)
    cpu = [None if a is None else torch.from_numpy(a).view(-1, k).clone().requires_grad_(True) for a, k in ((xt, 3), (xs, 3), (xn, 3), (f, info["k0"]))]
    u = torch.einsum("tsjk,sj->tk", kernel_blocks(name, cpu[0], cpu[1], cpu[2], c), cpu[3])
    u.square().sum().backward()
    dev = [None if a is None else torch.from_numpy(a).cuda().requires_grad_(True) for a in (xt, xs, xn, f)]
    ug = kernel_sum_geometry(name, *dev, ctx=ctx)
    assert rel_l2(ug.detach().cpu().numpy(), u.detach().numpy()) <= 1e-12
    ug.square().sum().backward()
    for what, a, b in zip(("r_trg", "r_src", "n_src", "v_src"), dev, cpu):
        if a is not None:
            err = rel_l2(a.grad.cpu().numpy(), b.grad.numpy())
            print("%s d/d%s: rel-L2 %.2e" % (name, what, err))
            assert a.grad.shape == a.shape and err <= 1e-12, (name, what, err)
    v = dev[3].detach().clone().requires_grad_(True)
    kernel_sum(name, dev[0].detach(), dev[1].detach(), None if dev[2] is None else dev[2].detach(), v, ctx=ctx).square().sum().backward()
    assert torch.equal(v.grad, dev[3].grad)
    x = dev[0].detach().clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(kernel_sum_geometry(name, x, dev[1].detach(), None if dev[2] is None else dev[2].detach(), v, ctx=ctx).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ---- plugins ----------------------------------------------------------------------------------------------------------------------------------
LAM = 2.5
YUKAWA_G = r"""
// The screened Coulomb (Yukawa) functor with a gradient form: phi = w f e^{-lambda r} / r, d phi / d d = -w f (lambda + 1/r) e^{-lambda r} / r^2 d
#include <sctl_amd/device/kernel_plugin.hpp>
struct Yukawa3D_FxU_G {
  static constexpr int ID = -1, K0 = 1, K1 = 1, ND = 0, NREC = 4, FLOPS = 10;
  static constexpr const char* NAME = "Yukawa3D-FxU-G";
  template <class R> using Consts = sctl_amd::DefaultConsts<R>;
  static constexpr double scale() { return 1 / (4 * sctl_amd::kPi); }
  static constexpr double acc_factor(int) { return 1; }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) { rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; }
  template <class R, int MODE, bool MASKED>
  static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const sctl_amd::KerCtx& ctx, const Consts<R>& K) {
    const R r2 = sctl_amd::len2(d);
    const R rinv = sctl_amd::rsqrt_masked<MODE, MASKED>(r2, K.rsq);
    acc[0] = sctl_amd::fma_(rec[3], rinv * exp_(-R(ctx.v[0]) * (r2 * rinv)), acc[0]);
  }
  template <class R, int MODE, bool MASKED, bool WANT_N>
  static __device__ __forceinline__ void pair_g(R (&G)[3], R (&)[1], const R (&d)[3], const R (&)[1], const R (&f)[K0], const R (&w)[K1], const sctl_amd::KerCtx& ctx,
                                                const Consts<R>& K) {
    const R r2 = sctl_amd::len2(d);
    const R y = sctl_amd::rsqrt_masked<MODE, MASKED>(r2, K.rsq);
    const R t = -(f[0] * w[0]) * (R(ctx.v[0]) + y) * (y * y) * exp_(-R(ctx.v[0]) * (r2 * y));
    for (int j = 0; j < 3; j++) G[j] = sctl_amd::fma_(t, d[j], G[j]);
  }
  static __device__ __forceinline__ double exp_(double x) { return ::exp(x); }
  static __device__ __forceinline__ float exp_(float x) { return ::expf(x); }
};
SCTL_AMD_REGISTER_KERNEL(Yukawa3D_FxU_G, /*context: lambda*/ 8)
"""


def test_plugin_with_pair_g_matches_its_torch_formula(tmp_path):
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
    for Nt, Ns in ((300, 50), (1100, 513)):
        xt, xs, _, f, w = cloud(31, Nt, Ns, info)
        xt[:3] = xs[3:6]
        ref = gradients(name, xt, xs, None, f, w, lam=LAM)[:3]
        check("plugin %d x %d" % (Nt, Ns), sctl_amd.eval_grad_host(name, xt, xs, None, f, w, ctx=ctx), ref, [1e-12] * 3)
        with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_t"):      # it has no transposed form, and needs none for this
            sctl_amd.eval_transpose_host(name, xt, xs, None, w, ctx=ctx)


def test_plugin_without_pair_g_is_refused_and_still_evaluates(tmp_path_factory):
    from test_gpu_transpose import _ensure, numpy_yukawa_matrix
    name = "Yukawa3D-FxU-T"                       # pair and pair_t, no pair_g
    _ensure(tmp_path_factory, name, "yukawa_t_kernel")
    info = sctl_amd.kernel_info(name)
    ctx = np.array([LAM])
    xt, xs, _, f, w = cloud(32, 200, 100, info)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_g"):
        sctl_amd.eval_grad_host(name, xt, xs, None, f, w, ctx=ctx)
    with pytest.raises(sctl_amd.api.SctlAmdError, match="status -1.*pair_g"):
        sctl_amd.plan_grad(name, 0, 200, 100)
    M = numpy_yukawa_matrix(xt, xs, LAM)
    assert rel_l2(sctl_amd.eval_host(name, xt, xs, None, f, ctx=ctx), (M.T @ f.astype(np.longdouble)).astype(np.float64)) <= 1e-12
    assert rel_l2(sctl_amd.eval_transpose_host(name, xt, xs, None, w, ctx=ctx), (M @ w.astype(np.longdouble)).astype(np.float64)) <= 1e-12


# ---- C++ --------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_eval_grad_against_the_python_entry(tmp_path):
    """tests/cpp/grad_driver.cpp: GenericKernel<Stokes3D_DxU>::EvalGrad (g++ -Wall -Werror) writes its inputs and its three gradients; the Python
    entry on the same inputs gives the same bits, and a second call accumulated"""
    from test_cpp_host import _build
    exe = _build(tmp_path, "grad_driver")
    out = str(tmp_path / "grad.bin")
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    Nt, Ns = 700, 450
    a = np.fromfile(out, dtype=np.float64)
    sizes = [Nt * 3, Ns * 3, Ns * 3, Ns * 3, Nt * 3, Nt * 3, Ns * 3, Ns * 3]
    assert a.size == sum(sizes)
    xt, xs, xn, f, w, g_trg, g_src, g_nrm = np.split(a, np.cumsum(sizes)[:-1])
    got = sctl_amd.eval_grad_host("Stokes3D-DxU", xt.copy(), xs.copy(), xn.copy(), f.copy(), w.copy())
    assert np.array_equal(got[0], g_trg) and np.array_equal(got[1], g_src) and np.array_equal(got[2], g_nrm)
