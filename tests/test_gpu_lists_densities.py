"""Several densities over the P2P lists in one launch (sctl_amd_lists_eval_densities_*, sctl_amd/csrc/lists_rows_kernel.hpp) on the GPU: every kernel through
every shape of a work item at every pass width against the CPU oracle's per-list loop and the single-density entry, the reference's goldens
(tests/golden/p2p_lists.npz), accumulate / nd == 1 / untouched targets / run-to-run / counters / one-shot / side-stream semantics, the accuracy
ladder, the plugin fallback and the C++ host surface."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2
from sctl_amd.lists import grid_neighbour_lists, points_in_boxes

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
MAN = json.load(open(os.path.join(GOLD, "lists_manifest.json")))
CASES = MAN["cases"]
IDS = ["%s-%s" % (c["kernel"], c["key"]) for c in CASES]
NDS = (2, 3, 5, 8, 9)        # every width, a partly filled form, the one-left-over single pass, two passes
FP32_KERNELS = ("Laplace3D-FxU", "Stokes3D-FxT", "Helmholtz3D-FxU")
TOL = {np.float64: 1e-12, np.float32: 2e-5}
_NPZ = None


@pytest.fixture(params=["packed", "packed up to 64", "one range per wave"])
def small_ranges(request):
    """The three SCTL_AMD_LISTS_PACK settings of tests/test_lists.py (read at plan creation): small target ranges packed up to 32 points (default),
    up to 64, or not at all (one range per wave, lane replicas)."""
    if request.param == "packed":
        os.environ.pop("SCTL_AMD_LISTS_PACK", None)
        yield True
    else:
        os.environ["SCTL_AMD_LISTS_PACK"] = "64" if request.param.endswith("64") else "0"
        try:
            yield request.param.endswith("64")
        finally:
            del os.environ["SCTL_AMD_LISTS_PACK"]


def oracle_lists(O, name, lists, xt, xs, xn, f, ctx=None, u=None):
    """The oracle = a loop of O.eval over the lists, each accumulating into its target range (f64 arithmetic)."""
    info = O.info(name)
    k0, k1, nd = info["k0"], info["k1"], info["nd"]
    x64 = [a.astype(np.float64) for a in (xt, xs, xn, f)]
    if u is None:
        u = np.zeros(xt.size // 3 * k1)
    for t0, tc, s0, sc in zip(*lists):
        t1, s1 = t0 + tc, s0 + sc
        if tc == 0 or sc == 0:
            continue
        O.eval(name, x64[0][t0 * 3:t1 * 3].copy(), x64[1][s0 * 3:s1 * 3].copy(), x64[2][s0 * nd:s1 * nd].copy(), x64[3][s0 * k0:s1 * k0].copy(),
               v_trg=u[t0 * k1:t1 * k1], ctx=ctx, nthreads=1)
    return u


# ---- 1. every kernel, every item shape ---------------------------------------------------------------------------------------------------
def _item_shape_layout(info):
    """The layout of test_hip_lists_every_kernel_every_item_shape: two targets per lane (200 targets), the four packed classes or, unpacked, one
    target per lane and lane replicas (50, 5, 20, 12, 33, 64, 1), every box against itself and two or three other ranges (173, 64 and 3 sources)."""
    rng = np.random.default_rng(77)
    tlen = np.array([200, 50, 5, 20, 12, 33, 64, 1], dtype=np.int64)
    tstart = np.concatenate([[0], np.cumsum(tlen)[:-1]])
    Nt, Ns = int(tlen.sum()), 700
    xt = rng.random(Nt * 3)
    xs = np.concatenate([xt, rng.random((Ns - Nt) * 3)])      # the first Nt sources ARE the targets (r = 0 pairs in the "self" lists)
    xn = rng.random(Ns * info["nd"]) - 0.5
    F = rng.random((max(NDS), Ns * info["k0"])) - 0.5
    to, tc, so, sc = [], [], [], []
    for b in range(tlen.size):
        for s0, n in ((int(tstart[b]), int(tlen[b])), (300, 173), (473, 64), (650, 3))[:4 if b % 3 else 3]:
            to.append(tstart[b]); tc.append(tlen[b]); so.append(s0); sc.append(n)
    return [np.array(a, dtype=np.int64) for a in (to, tc, so, sc)], Nt, Ns, xt, xs, xn, F


_REF = {}


def _item_shape_reference(O, name):
    """the oracle's rows, computed once per kernel and shared by the precisions and the packing settings"""
    if name not in _REF:
        lists, Nt, Ns, xt, xs, xn, F = _item_shape_layout(sctl_amd.kernel_info(name))
        _REF[name] = [oracle_lists(O, name, lists, xt, xs, xn, F[m], ctx_for(name)) for m in range(max(NDS))]
    return _REF[name]


@pytest.mark.parametrize("name,dt", [(n, np.float64) for n in sctl_amd.KERNEL_NAMES] + [(n, np.float32) for n in FP32_KERNELS],
                         ids=[n + "-f64" for n in sctl_amd.KERNEL_NAMES] + [n + "-f32" for n in FP32_KERNELS])
def test_every_kernel_every_item_shape(O, name, dt, small_ranges):
    info = sctl_amd.kernel_info(name)
    lists, Nt, Ns, xt, xs, xn, F = _item_shape_layout(info)
    ref = _item_shape_reference(O, name)
    xt, xs, xn, F = [a.astype(dt) for a in (xt, xs, xn, F)]
    ctx = ctx_for(name)
    plan = sctl_amd.ListsPlan(name, dt, *lists, Nt, Ns, ctx=ctx)
    single = [plan.eval_host(xt, xs, xn, F[m].copy()) for m in range(max(NDS))] if dt == np.float64 else None
    for nd in NDS:
        U = plan.eval_densities_host(xt, xs, xn, np.ascontiguousarray(F[:nd]))
        assert U.shape == (nd, Nt * info["k1"]) and U.dtype == dt and np.all(np.isfinite(U))
        errs = [rel_l2(U[m], ref[m]) for m in range(nd)]
        print("%s %s nd=%d rel-L2 vs oracle: %s" % (name, np.dtype(dt).name, nd, " ".join("%.1e" % e for e in errs)))
        assert max(errs) <= TOL[dt], (name, nd, errs)
        if dt == np.float64:
            diffs = [rel_l2(U[m], single[m]) for m in range(nd)]
            print("%s nd=%d rel-L2 vs eval_host: %s" % (name, nd, " ".join("%.1e" % e for e in diffs)))
            assert max(diffs) <= 1e-14, (name, nd, diffs)
        if name == "Stokes3D-FxT":
            m9 = U.reshape(nd, Nt, 3, 3)
            assert np.array_equal(m9, m9.transpose(0, 1, 3, 2))                               # each row's 3x3 output is exactly symmetric
    plan.close()


# ---- 2. the reference's goldens ----------------------------------------------------------------------------------------------------------
def gold(case):
    global _NPZ
    if _NPZ is None:
        _NPZ = np.load(os.path.join(GOLD, "p2p_lists.npz"))
    return _NPZ[case["key"]]


def case_data(case, info):
    """tests/test_lists.py: case_data (oracle/gen_golden_lists.py: list_case_inputs), the inputs regenerated from the seed"""
    dt = np.float64 if case["dtype"] == "f64" else np.float32
    rng = np.random.default_rng(case["seed"])
    nb = case["grid"] ** 3
    cs = rng.integers(1, case["max_pts"] + 1, nb)
    ct = cs if case["self_targets"] else rng.integers(1, case["max_pts"] + 1, nb)
    xs = points_in_boxes(case["grid"], cs, rng, dt)
    xt = xs if case["self_targets"] else points_in_boxes(case["grid"], ct, rng, dt)
    ns = int(cs.sum())
    xn = (rng.random(ns * info["nd"]) - 0.5).astype(dt)
    f = (rng.random(ns * info["k0"]) - 0.5).astype(dt)
    lists = grid_neighbour_lists(case["grid"], ct, cs)
    assert lists[0].size == case["nlists"] and int((lists[1] * lists[3]).sum()) == case["pairs"]
    ctx = np.array(MAN["helmholtz_k"]) if case["kernel"].startswith("Helmholtz") else None
    return lists, xt, xs, xn, f, ctx


def tol(case):
    if case["digits"] >= 0:
        return 10.0 * 10.0 ** (-case["digits"])
    return 1e-12 if case["dtype"] == "f64" else 2e-5


_GOLD_REF = {}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_goldens(O, case, small_ranges):
    import torch
    name = case["kernel"]
    info = sctl_amd.kernel_info(name)
    lists, xt, xs, xn, f, ctx = case_data(case, info)
    dt = xt.dtype
    F = np.stack([f] + [(np.random.default_rng(case["seed"] + 100 + m).random(f.size) - 0.5).astype(dt) for m in (1, 2)])
    if case["key"] not in _GOLD_REF:
        _GOLD_REF[case["key"]] = [oracle_lists(O, name, lists, xt, xs, xn, F[m], ctx) for m in (1, 2)]
    ref = _GOLD_REF[case["key"]]
    plan = sctl_amd.ListsPlan(name, dt, *lists, case["Nt"], case["Ns"], ctx=ctx)
    U = plan.eval_densities_host(xt, xs, xn, F, digits=case["digits"])
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, F)]
    if case["self_targets"]:
        d[1] = d[0]                                           # one array on the device too
    Ud = plan.eval_densities_device(*d, digits=case["digits"])
    torch.cuda.synchronize()
    for what, V in (("host", U), ("device", Ud.cpu().numpy())):
        assert V.shape == (3, case["Nt"] * info["k1"]) and np.all(np.isfinite(V))
        errs = [rel_l2(V[0], gold(case))] + [rel_l2(V[m], ref[m - 1]) for m in (1, 2)]
        print("%s %s: row 0 vs reference %.1e, rows 1-2 vs oracle %.1e %.1e (tol %.0e)" % (case["key"], what, errs[0], errs[1], errs[2], tol(case)))
        assert max(errs) <= tol(case), (what, errs)
    plan.close()


# ---- 3. semantics -------------------------------------------------------------------------------------------------------------------------
def _ragged(seed):
    """tests/test_lists.py: test_hip_lists_random_ragged — target ranges of random lengths with gaps between them, each with a random number of
    source ranges of random lengths (many of 1-3 points), random kernel and precision."""
    rng = np.random.default_rng(4000 + seed)
    name = sctl_amd.KERNEL_NAMES[int(rng.integers(0, len(sctl_amd.KERNEL_NAMES)))]
    info = sctl_amd.kernel_info(name)
    dt = np.float64 if rng.random() < 0.7 else np.float32
    Ns = int(rng.integers(50, 3000))
    nbox = int(rng.integers(1, 60))
    tlen = rng.integers(0, 700, nbox) if seed % 2 else rng.integers(0, 40, nbox)
    gaps = rng.integers(0, 5, nbox)
    tstart = np.cumsum(gaps + np.concatenate([[0], tlen[:-1]]))
    Nt = int(tstart[-1] + tlen[-1] + 3)
    to, tc, so, sc = [], [], [], []
    for b in range(nbox):
        for _ in range(int(rng.integers(0, 41))):
            n = int(rng.integers(0, 4)) if rng.random() < 0.5 else int(rng.integers(0, min(300, Ns)))
            s0 = int(rng.integers(0, Ns - n + 1))
            to.append(tstart[b]); tc.append(tlen[b]); so.append(s0); sc.append(n)
    order = rng.permutation(len(to))
    lists = [np.array(a, dtype=np.int64)[order] for a in (to, tc, so, sc)]
    xt, xs = rng.random(Nt * 3).astype(dt), rng.random(Ns * 3).astype(dt)
    xn = (rng.random(Ns * info["nd"]) - 0.5).astype(dt)
    return rng, name, info, dt, lists, Nt, Ns, xt, xs, xn


@pytest.mark.parametrize("seed", [0, 1])
def test_ragged_accumulate_untouched_targets_run_to_run_and_one_shot(O, seed, small_ranges):
    rng, name, info, dt, lists, Nt, Ns, xt, xs, xn = _ragged(seed)
    nd = 5
    F = (rng.random((nd, Ns * info["k0"])) - 0.5).astype(dt)
    V0 = rng.random((nd, Nt * info["k1"])).astype(dt)
    ctx = ctx_for(name)
    plan = sctl_amd.ListsPlan(name, dt, *lists, Nt, Ns, ctx=ctx)
    fresh = plan.eval_densities_host(xt, xs, xn, F)
    U = plan.eval_densities_host(xt, xs, xn, F, V_trg=V0.copy())
    assert np.array_equal(U, V0 + fresh)                                                      # accumulated into: one addition per entry
    assert np.array_equal(plan.eval_densities_host(xt, xs, xn, F), fresh)                     # bit-identical from run to run
    covered = np.zeros(Nt, dtype=bool)
    for t0, n, m in zip(lists[0], lists[1], lists[3]):
        if n and m:
            covered[t0:t0 + n] = True
    assert (~covered).any()
    for m in range(nd):
        ref = oracle_lists(O, name, lists, xt, xs, xn, F[m], ctx)
        assert rel_l2(fresh[m], ref) <= (1e-12 if dt == np.float64 else 3e-5), (name, dt, m, rel_l2(fresh[m], ref))
        assert np.array_equal(U[m].reshape(Nt, -1)[~covered], V0[m].reshape(Nt, -1)[~covered])   # targets of no list keep their bits in every row
    pc0 = sctl_amd.counters()["pair_interactions"]
    one_shot = sctl_amd.eval_lists_densities_host(name, *lists, xt, xs, xn, F, ctx=ctx)
    assert np.array_equal(one_shot, fresh)                                                    # the one-shot entry equals the plan entry
    assert sctl_amd.counters()["pair_interactions"] - pc0 == nd * plan.pairs                  # counters grow by nd x pairs
    one = plan.eval_densities_host(xt, xs, xn, F[:1].copy(), V_trg=V0[:1].copy())            # nd == 1 IS the single-density entry
    assert np.array_equal(one[0], plan.eval_host(xt, xs, xn, F[0].copy(), v_trg=V0[0].copy()))
    plan.close()


def test_device_entry_on_a_side_stream_and_argument_errors_with_work():
    import torch
    rng = np.random.default_rng(5)
    name = "Stokes3D-FxU"
    Nt, Ns, nd = 900, 1200, 6
    xt, xs = rng.random(Nt * 3), rng.random(Ns * 3)
    F = rng.random((nd, Ns * 3)) - 0.5
    lists = [np.array(v, dtype=np.int64) for v in ([0, 0, 300, 700, 310], [300, 300, 10, 200, 40], [0, 600, 100, 0, 5], [600, 600, 900, 1200, 77])]
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, Nt, Ns)
    U = plan.eval_densities_host(xt, xs, None, F)
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, F)]
    side = torch.cuda.Stream()
    V = torch.full((nd, Nt * 3), 0.5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        plan.eval_densities_device(d[0], d[1], None, d[2], V_trg=V)                           # torch's current stream: the side stream
    plan.eval_densities_device(d[0], d[1], None, d[2], V_trg=V, stream=side)                  # ... and named explicitly, ordered after the first
    side.synchronize()
    assert rel_l2(V.cpu().numpy(), 0.5 + 2 * U) <= 1e-15                                      # (the device adds on the device, rounding once per call)
    expect = V.cpu().numpy()
    # with work present, null arrays and a negative nd are refused before any launch
    L = sctl_amd.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = [p(d[0]), p(d[1]), None, p(d[2]), p(V)]
    for i in (0, 1, 3, 4):
        a = list(args)
        a[i] = None
        assert L.sctl_amd_lists_eval_densities_device(plan._h, nd, *a, -1, None, 0, None) == -2
        assert b"null coordinate" in L.sctl_amd_last_error()
    assert L.sctl_amd_lists_eval_densities_device(plan._h, -1, *args, -1, None, 0, None) == -2
    assert L.sctl_amd_lists_eval_densities_host(plan._h, nd, None, None, None, None, None, -1, None, 0) == -2
    assert L.sctl_amd_lists_eval_densities_device(plan._h, 0, *args, -1, None, 0, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(V.cpu().numpy(), expect)                                            # nd == 0 and the refused calls did nothing
    plan.close()


# ---- 4. digits ladder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-FxU"])
def test_digits_ladder(O, name):
    """each digits request within the bound of test_digits_ladder in tests/test_gpu_densities.py"""
    info = sctl_amd.kernel_info(name)
    lists, Nt, Ns, xt, xs, xn, F = _item_shape_layout(info)
    F = np.ascontiguousarray(F[:4])
    exact = _item_shape_reference(O, name)
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, Nt, Ns)
    for dg in (3, 7, 10, -1):
        U = plan.eval_densities_host(xt, xs, xn, F, digits=dg)
        errs = [rel_l2(U[m], exact[m]) for m in range(4)]
        print("%s digits %d: %s" % (name, dg, " ".join("%.1e" % e for e in errs)))
        assert max(errs) <= (10.0 * 10.0 ** (-dg) if dg >= 0 else 5e-15), (dg, errs)
    plan.close()


# ---- 5. plugin fallback -------------------------------------------------------------------------------------------------------------------
def test_plugin_kernel_falls_back_to_single_density_calls(tmp_path):
    name = "Yukawa3D-FxU"
    try:
        sctl_amd.kernel_id(name)
    except KeyError:
        so = str(tmp_path / "libyukawa_kernel.so")
        libdir = os.path.join(ROOT, "sctl_amd")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "plugin", "yukawa_kernel.hip"), "-o", so, "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir], check=True)
        assert sctl_amd.load_plugin(so) == [name]
    info = sctl_amd.kernel_info(name)
    lists, Nt, Ns, xt, xs, xn, F = _item_shape_layout(info)
    F = np.ascontiguousarray(F[:3])
    lam = np.array([2.5])
    plan = sctl_amd.ListsPlan(name, np.float64, *lists, Nt, Ns, ctx=lam)
    pc0 = sctl_amd.counters()["pair_interactions"]
    U = plan.eval_densities_host(xt, xs, xn, F)
    assert sctl_amd.counters()["pair_interactions"] - pc0 == 3 * plan.pairs
    for m in range(3):
        assert np.array_equal(U[m], plan.eval_host(xt, xs, xn, F[m].copy()))                  # three single calls, bit for bit
    plan.close()


# ---- 6. the C++ host surface ----------------------------------------------------------------------------------------------------------------
def test_cpp_host_surface_eval_lists_densities_matches_eval_lists(tmp_path):
    exe = str(tmp_path / "lists_densities_driver")
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lists_densities_driver.cpp"),
                    "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    nd = 5
    out = str(tmp_path / "o.bin")
    p = subprocess.run([exe, "40", str(nd), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    raw = np.fromfile(out, dtype=np.float64).reshape(2, nd, -1)
    for m in range(nd):
        assert rel_l2(raw[0, m], raw[1, m]) <= 1e-14, (m, rel_l2(raw[0, m], raw[1, m]))
