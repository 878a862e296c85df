"""Geometry gradients of kernel sums over P2P lists (sctl_amd_lists_eval_grad_*, include/sctl_amd/device/lists_grad_kernel.hpp) on the GPU.

Expected value throughout: torch's CPU autograd of the dense fp64 formula of tests/grad_truth.py with the pairs that no list names left out
(gradients(..., zero=mask)); a list that is given twice adds its own truth once more.  g_trg, g_src and g_nrm are compared separately, each as
rel-L2 against its own norm, and every value must be finite.  Inputs are fp32-representable doubles (cloud of tests/test_gpu_grad.py), so one
truth serves both precisions.  Bounds, those of tests/test_gpu_grad.py: fp64 <= 1e-12 at full precision and 10 * 10^-d at digits = d; fp32 <= 4 x
the rel-L2 of the same formula and its autograd in torch float32 against the fp64 truth.

The lists.  RANGES are the owner sizes that reach every item shape of the plan under the three packing settings: the four packed classes (up
to 8, 16, 32, 64 owners), the replica widths 8 / 16 / 32, one and two owners per lane, a range cut into several items (129, 200).  Owner range i
streams pattern i mod 4 of PATTERNS — ranges of the other set whose lengths sum to 3 (a partial tile out of three 1-point ranges), 64 (an exact
tile spanning four short ranges), 65 (a full tile spanning two ranges and a ragged second one) and 202 (several tiles, five ranges).  `lists_a`
gives the TARGET ranges these patterns (side 0 under control), `lists_b` the SOURCE ranges, shifted by two (side 1 under control); both are planned
in both directions and all three outputs are checked on both.  20 targets are copies of sources they are listed against (the repair, without the
own-points shortcut), and one list is given twice."""
import ctypes
import os

import numpy as np
import pytest

import sctl_amd
from conftest import ctx_for, rel_l2
from grad_truth import HELMHOLTZ_KS, gradients
from test_gpu_grad import OUT, as_dt, bounds_for, check, cloud
from test_plugin import LAM, NAME as PLUGIN_NAME, plugin  # noqa: F401  (the fixture that builds and loads the Yukawa plugin)

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
BAD_ARGUMENT, UNKNOWN_KERNEL = -2, -1
RANGES = [1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 200, 1, 1]          # 711 points per set; the two extra 1-point ranges only serve pattern 0
OFF = np.concatenate([[0], np.cumsum(RANGES)[:-1]]).astype(np.int64)
N = int(np.sum(RANGES))
_R = {n: i for i, n in enumerate(RANGES[:13])}
PATTERNS = [[0, 13, 14], [_R[7], _R[8], _R[16], _R[33]], [0, _R[64]], [_R[9], _R[17], _R[32], _R[128], _R[16]]]
assert [sum(RANGES[r] for r in p) for p in PATTERNS] == [3, 64, 65, 202]


@pytest.fixture(params=["packed", "packed up to 64", "one range per wave"])
def small_ranges(request):
    """the three packing settings of tests/test_lists.py (read at plan creation)"""
    if request.param == "packed":
        os.environ.pop("SCTL_AMD_LISTS_PACK", None)
        yield request.param
    else:
        os.environ["SCTL_AMD_LISTS_PACK"] = "64" if request.param.endswith("64") else "0"
        try:
            yield request.param
        finally:
            del os.environ["SCTL_AMD_LISTS_PACK"]


def pattern_lists(shift, owners_are_targets):
    """owner range i (the 13 sizes) against the ranges of pattern (i + shift) mod 4; the list of the 33-point owner range's first pattern entry twice"""
    own, strm = [], []
    for i in range(13):
        for r in PATTERNS[(i + shift) % 4]:
            own.append(i)
            strm.append(r)
    k = own.index(_R[33])
    own.append(own[k])
    strm.append(strm[k])
    own, strm = np.array(own), np.array(strm)
    cnt = np.array(RANGES, dtype=np.int64)
    t, s = (own, strm) if owners_are_targets else (strm, own)
    return OFF[t], cnt[t], OFF[s], cnt[s]


def pair_counts(lists, Nt, Ns):
    """how many lists name the pair (t, s)"""
    m = np.zeros((Nt, Ns), dtype=np.int64)
    for t0, tc, s0, sc in zip(*lists):
        m[t0:t0 + tc, s0:s0 + sc] += 1
    return m


def lists_truth(name, lists, xt, xs, xn, f, w, c, dtype):
    """(g_trg, g_src, g_nrm or None): the dense gradients with the unlisted pairs left out, plus the own truth of every list beyond a pair's first"""
    import torch
    Nt, Ns = xt.size // 3, xs.size // 3
    info = sctl_amd.kernel_info(name)
    m = pair_counts(lists, Nt, Ns)
    ref = [None if g is None else g.copy() for g in gradients(name, xt, xs, xn, f, w, c, dtype=dtype, zero=torch.from_numpy(m == 0))[:3]]
    seen = set()
    for l in zip(*(a.tolist() for a in lists)):
        if l in seen:                       # a repeated list: its pairs count once more
            t0, tc, s0, sc = l
            cut = lambda a, k, o, n: None if a is None else a.reshape(-1, k)[o:o + n].ravel().copy()
            g = gradients(name, cut(xt, 3, t0, tc), cut(xs, 3, s0, sc), cut(xn, 3, s0, sc), cut(f, info["k0"], s0, sc), cut(w, info["k1"], t0, tc), c, dtype=dtype)
            ref[0][t0 * 3:(t0 + tc) * 3] += g[0]
            ref[1][s0 * 3:(s0 + sc) * 3] += g[1]
            if ref[2] is not None:
                ref[2][s0 * 3:(s0 + sc) * 3] += g[2]
        seen.add(l)
    assert m.max() <= 2
    return ref


_CASES = {}


def case(name, which, ctx_key="default"):
    """inputs, lists, the fp64 truth and torch-fp32's error against it, computed once per (kernel, list set) and shared by the tests.
    which: "a" / "b" (separate arrays, 20 shared points, the pattern lists), "self" (one array, every box against itself and its neighbours in the
    array), "dense" (one list of 300 x 200 points)"""
    key = (name, which, ctx_key)
    if key not in _CASES:
        import torch
        info = sctl_amd.kernel_info(name)
        Nt, Ns = (300, 200) if which == "dense" else (N, N)
        xt, xs, xn, f, w = cloud(4000 + 13 * KERNELS.index(name) + len(which), Nt, Ns, info)
        if which in ("a", "b"):
            lists = pattern_lists(0 if which == "a" else 2, which == "a")
            step = lists[0].size // 20
            for k in range(20):             # 20 targets become copies of sources they are listed against
                t0, tc, s0, sc = (int(a[k * step]) for a in lists)
                xt.reshape(-1, 3)[t0 + k % tc] = xs.reshape(-1, 3)[s0 + (7 * k) % sc]
        elif which == "self":
            xs = xt
            nb = [(i, j) for i in range(13) for j in (i - 1, i, i + 1) if 0 <= j < 13]
            cnt = np.array(RANGES, dtype=np.int64)
            ti, si = np.array([p[0] for p in nb]), np.array([p[1] for p in nb])
            lists = (OFF[ti], cnt[ti], OFF[si], cnt[si])
            Nt = Ns = int(np.sum(RANGES[:13]))
            xt = xs = xt[:Nt * 3].copy()
            xn = None if xn is None else xn[:Ns * 3].copy()
            f, w = f[:Ns * info["k0"]].copy(), w[:Nt * info["k1"]].copy()
        else:
            i8 = lambda v: np.array([v], dtype=np.int64)
            lists = (i8(0), i8(Nt), i8(0), i8(Ns))
        ctx = ctx_for(name) if ctx_key == "default" else np.array(ctx_key)
        c = None if ctx is None else tuple(ctx)
        ref = lists_truth(name, lists, xt, xs, xn, f, w, c, torch.float64)
        ref32 = lists_truth(name, lists, xt, xs, xn, f, w, c, torch.float32)
        err32 = [None if r is None else rel_l2(r32, r) for r, r32 in zip(ref, ref32)]
        _CASES[key] = (lists, xt, xs, xn, f, w, ctx, ref, err32)
    return _CASES[key]


def run_host(name, dt, lists, xt, xs, xn, f, w, ctx, digits=-1, same=False, **kw):
    a = as_dt(dt, xt, xs, xn, f, w)
    if same:
        a[1] = a[0]                         # ONE array for both sets: the packed items' own-points shortcut
    plan = sctl_amd.ListsPlan(name, dt, *lists, a[0].size // 3, a[1].size // 3, ctx=ctx, directions="both")
    try:
        return plan.eval_grad_host(*a, digits=digits, **kw)
    finally:
        plan.close()


@pytest.mark.parametrize("dt,digits", [(np.float64, -1), (np.float64, 10), (np.float32, -1)], ids=["f64", "f64-d10", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_every_item_shape_on_both_sides(name, dt, digits, small_ranges):
    """the pattern lists: the target ranges under control (a), the source ranges under control (b)"""
    for which in ("a", "b"):
        lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, which)
        got = run_host(name, dt, lists, xt, xs, xn, f, w, ctx, digits)
        assert all(g is None or g.dtype == dt for g in got)
        check("%s %s digits %d lists %s, %s" % (name, dt.__name__, digits, which, small_ranges), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_sources_that_are_the_targets(name, dt, small_ranges):
    """one array for both sets, every box against itself and its neighbours: the packed own-points shortcut and the repair; coincident pairs give 0"""
    lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, "self")
    got = run_host(name, dt, lists, xt, xs, xn, f, w, ctx, same=True)
    check("%s %s self, %s" % (name, dt.__name__, small_ranges), got, ref, bounds_for(dt, -1, err32))


@pytest.mark.parametrize("k", HELMHOLTZ_KS, ids=lambda k: "k=%g+%gi" % k)
def test_helmholtz_wavenumbers(k):
    name = "Helmholtz3D-FxU"
    for which in ("a", "self"):
        lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, which, ctx_key=k)
        for dt, digits in ((np.float64, -1), (np.float64, 10), (np.float32, -1)):
            got = run_host(name, dt, lists, xt, xs, xn, f, w, ctx, digits, same=which == "self")
            check("%s %s digits %d lists %s k %s" % (name, dt.__name__, digits, which, k), got, ref, bounds_for(dt, digits, err32))


@pytest.mark.parametrize("name", ["Laplace3D-DxU", "Stokes3D-FxUP", "Helmholtz3D-FxU"])
def test_runs_and_entries_agree_bit_for_bit(name):
    """two runs of the device entry; the host entry, the device entry and the one-shot; one side alone leaves the other side's arrays untouched"""
    import torch
    lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, "a")
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, N, N, ctx=ctx, directions="both")
    host = plan.eval_grad_host(xt, xs, xn, f, w)
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (xt, xs, xn, f, w)]
    dev1 = [None if g is None else g.cpu().numpy() for g in plan.eval_grad_device(*d)]
    dev2 = [None if g is None else g.cpu().numpy() for g in plan.eval_grad_device(*d)]
    shot = sctl_amd.eval_lists_grad_host(name, *lists, xt, xs, xn, f, w, ctx=ctx)
    for what, h, a, b, s in zip(OUT, host, dev1, dev2, shot):
        if h is not None:
            assert np.array_equal(a, b), what
            assert np.array_equal(h, a) and np.array_equal(h, s), what
    # want: only the named outputs exist, and they are the full call's
    only_trg = plan.eval_grad_host(xt, xs, xn, f, w, want=["trg"])
    assert only_trg[1] is None and only_trg[2] is None and np.array_equal(only_trg[0], host[0])
    only_src = plan.eval_grad_host(xt, xs, xn, f, w, want=["src", "nrm"] if xn is not None else ["src"])
    assert only_src[0] is None and np.array_equal(only_src[1], host[1]) and (xn is None or np.array_equal(only_src[2], host[2]))
    # null outputs through the C entry: the arrays of the side that is not asked for are not touched
    L = sctl_amd.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    keep, cp, cb = sctl_amd.api._ctx_blob(plan.info, ctx)
    mark = [torch.full((N * 3,), 0.0 if i == 0 else 7.0, dtype=torch.float64, device="cuda") for i in range(3)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.sctl_amd_lists_eval_grad_device(plan._h, *[p(t) for t in d], p(mark[0]), None, None, -1, cp, cb, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(mark[0].cpu().numpy(), host[0]) and bool((mark[1] == 7.0).all()) and bool((mark[2] == 7.0).all())
    plan.close()


@pytest.mark.parametrize("name", ["Laplace3D-FDxUdU", "Stokes3D-FxU"])
def test_outputs_are_accumulated_into(name):
    lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, "b")
    rng = np.random.default_rng(3)
    pre = [None if r is None else rng.random(r.size) - 0.5 for r in ref]
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, N, N, ctx=ctx, directions="both")
    got = plan.eval_grad_host(xt, xs, xn, f, w, *[None if q is None else q.copy() for q in pre])
    plan.close()
    check("%s accumulate" % name, [None if g is None else g - q for g, q in zip(got, pre)], ref, bounds_for(np.float64, -1, err32))


def test_errors_name_what_is_wrong():
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = lambda v: np.array([v], dtype=np.int64)
    lists = (one(0), one(4), one(0), one(4))

    def expect(plan, g, rc, word):
        got = L.sctl_amd_lists_eval_grad_device(plan._h, p(z), p(z), p(z), p(z), p(z), *[p(z) if x else None for x in g], -1, None, 0, None)
        msg = L.sctl_amd_last_error().decode()
        assert got == rc and msg and word in msg, (got, msg)
        got = L.sctl_amd_lists_eval_grad_host(plan._h, p(z), p(z), p(z), p(z), p(z), *[p(z) if x else None for x in g], -1, None, 0)
        assert got == rc and L.sctl_amd_last_error().decode(), got

    fwd = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *lists, 4, 4)
    expect(fwd, (0, 1, 0), BAD_ARGUMENT, "TRANSPOSE")
    tr = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *lists, 4, 4, directions="transpose")
    expect(tr, (1, 0, 0), BAD_ARGUMENT, "FORWARD")
    both = sctl_amd.ListsPlan("Laplace3D-FxU", np.float64, *lists, 4, 4, directions="both")
    expect(both, (0, 0, 1), BAD_ARGUMENT, "normal")
    for q in (fwd, tr, both):
        q.close()


def test_a_plugin_kernel_is_refused(plugin):  # noqa: F811
    """the Yukawa plugin of tests/test_plugin.py, built and loaded by that module's own fixture"""
    L = sctl_amd.lib()
    z = np.zeros(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = lambda v: np.array([v], dtype=np.int64)
    plan = sctl_amd.ListsPlan(PLUGIN_NAME, np.float64, one(0), one(4), one(0), one(4), 4, 4, ctx=np.array([LAM]))
    keep, cp, cb = sctl_amd.api._ctx_blob(plan.info, plan.ctx)
    rc = L.sctl_amd_lists_eval_grad_device(plan._h, p(z), p(z), None, p(z), p(z), p(z), None, None, -1, cp, cb, None)
    assert rc == UNKNOWN_KERNEL and "plugin" in L.sctl_amd_last_error().decode()
    plan.close()


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Laplace3D-DxU", "Stokes3D-FxU", "Helmholtz3D-FxU"])
def test_autograd_lists_sum_geometry(name):
    """(u * w).sum() through lists_sum_geometry: coordinates, normals and density against the truth, with one tensor for both point sets (torch adds
    the two coordinate gradients) and with separate tensors; with requires_grad on the density only no gradient side is launched"""
    import torch
    from sctl_amd.autograd import lists_sum_geometry
    for which in ("self", "a"):
        lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, which)
        Nt = xt.size // 3
        info = sctl_amd.kernel_info(name)
        # the density gradient: the truth's fourth output, restricted to the listed pairs
        m = pair_counts(lists, Nt, xs.size // 3)
        c = None if ctx is None else tuple(ctx)
        g_f = gradients(name, xt, xs, xn, f, w, c, zero=torch.from_numpy(m == 0))[3]
        if which == "a":                    # (its repeated list counts once more)
            t0, tc, s0, sc = (int(a[-1]) for a in lists)
            cut = lambda a, k, o, n: None if a is None else a.reshape(-1, k)[o:o + n].ravel().copy()
            g_f[s0 * info["k0"]:(s0 + sc) * info["k0"]] += gradients(name, cut(xt, 3, t0, tc), cut(xs, 3, s0, sc), cut(xn, 3, s0, sc), cut(f, info["k0"], s0, sc),
                                                                     cut(w, info["k1"], t0, tc), c)[3]
        plan = sctl_amd.ListsPlan(name, np.float64, *lists, Nt, xs.size // 3, ctx=ctx, directions="both")
        T = lambda a: None if a is None else torch.from_numpy(a).cuda().requires_grad_(True)
        t_xt, t_xn, t_f = T(xt), T(xn), T(f)
        t_xs = t_xt if which == "self" else T(xs)
        t_w = torch.from_numpy(w).cuda()
        u = lists_sum_geometry(plan, t_xt, t_xs, t_xn, t_f)
        (u * t_w).sum().backward()
        b = bounds_for(np.float64, -1, err32)
        if which == "self":
            got_x = t_xt.grad.cpu().numpy()
            err = rel_l2(got_x, ref[0] + ref[1])
            print("%s self: x.grad rel-L2 %.2e against g_trg + g_src" % (name, err))
            assert np.all(np.isfinite(got_x)) and err <= b[0]
        else:
            check("%s autograd coordinates" % name, (t_xt.grad.cpu().numpy(), t_xs.grad.cpu().numpy(), None), (ref[0], ref[1], None), b)
        if xn is not None:
            check("%s autograd normals" % name, (None, None, t_xn.grad.cpu().numpy()), (None, None, ref[2]), b)
        err = rel_l2(t_f.grad.cpu().numpy(), g_f)
        print("%s %s: v_src.grad rel-L2 %.2e" % (name, which, err))
        assert err <= 1e-12
        # the density alone: the backward is the transposed list sum and nothing else
        t_f2 = torch.from_numpy(f).cuda().requires_grad_(True)
        u = lists_sum_geometry(plan, t_xt.detach(), t_xs.detach(), None if t_xn is None else t_xn.detach(), t_f2)
        sctl_amd.api.reset_counters()
        (u * t_w).sum().backward()
        torch.cuda.synchronize()
        assert sctl_amd.counters()["pair_interactions"] == plan.transpose_info()["pairs"]
        assert rel_l2(t_f2.grad.cpu().numpy(), g_f) <= 1e-12
        plan.close()


@pytest.mark.parametrize("name", KERNELS)
def test_one_list_of_everything_is_the_dense_gradient(name):
    """one list covering 300 x 200 points against sctl_amd.eval_grad_host, within the sum of both bounds"""
    lists, xt, xs, xn, f, w, ctx, ref, err32 = case(name, "dense")
    for dt in (np.float64, np.float32):
        a = as_dt(dt, xt, xs, xn, f, w)
        got = sctl_amd.eval_lists_grad_host(name, *lists, *a, ctx=ctx)
        dense = sctl_amd.eval_grad_host(name, *a, ctx=ctx)
        b = bounds_for(dt, -1, err32)
        check("%s %s one list against the truth" % (name, dt.__name__), got, ref, b)
        check("%s %s one list against eval_grad_host" % (name, dt.__name__), got, dense, [None if x is None else 2 * x for x in b])
