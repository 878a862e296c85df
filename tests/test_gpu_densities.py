"""Several densities against one geometry (sctl_amd_eval_densities_*) on the GPU: every built-in kernel in fp64 and fp32 against the CPU oracle
and against the single-density entry row by row, accumulate / nd == 0 / nd == 1 semantics, coincident points, the accuracy ladder, a split-heavy
and a target-cut plan, Helmholtz, a side stream, the operator handle with weights and target normals, and the plugin fallback."""
import os

import numpy as np
import pytest

import sctl_amd
from conftest import ROOT, ctx_for, rel_l2

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (63, 257), (513, 1025), (3000, 4099)]
TOL = {np.float64: 1e-12, np.float32: 2e-5}


def _inputs(rng, Nt, Ns, info, nd, dt):
    xt, xs = rng.random(Nt * 3).astype(dt), rng.random(Ns * 3).astype(dt)
    xn = (rng.random(Ns * info["nd"]) - 0.5).astype(dt) if info["nd"] else None
    F = (rng.random((nd, Ns * info["k0"])) - 0.5).astype(dt)
    return xt, xs, xn, F


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_every_row_matches_the_oracle_and_the_single_density_entry(O, name, dt):
    info = sctl_amd.kernel_info(name)
    ctx = ctx_for(name)
    rng = np.random.default_rng(sctl_amd.KERNEL_NAMES.index(name) * 2 + (dt == np.float32))
    for nd in (2, 3, 8, 11):
        for Nt, Ns in SIZES:
            xt, xs, xn, F = _inputs(rng, Nt, Ns, info, nd, dt)
            U = sctl_amd.eval_densities_host(name, xt, xs, xn, F, ctx=ctx)
            assert U.shape == (nd, Nt * info["k1"]) and U.dtype == dt
            for m in range(nd):
                ref = O.eval(name, xt, xs, xn, F[m].copy(), ctx=ctx)
                assert rel_l2(U[m], ref) <= TOL[dt], (name, nd, Nt, Ns, m, rel_l2(U[m], ref))
                if dt == np.float64:
                    one = sctl_amd.eval_host(name, xt, xs, xn, F[m].copy(), ctx=ctx)
                    assert rel_l2(U[m], one) <= 1e-14, (name, nd, Nt, Ns, m, rel_l2(U[m], one))


def test_accumulate_nd1_is_bit_identical_and_nd0_is_a_no_op():
    rng = np.random.default_rng(1)
    for name in ("Laplace3D-FxU", "Stokes3D-DxU", "Helmholtz3D-FxU"):
        info = sctl_amd.kernel_info(name)
        for dt in (np.float64, np.float32):
            xt, xs, xn, F = _inputs(rng, 700, 900, info, 3, dt)
            V0 = (rng.random((3, 700 * info["k1"])) - 0.5).astype(dt)
            U = sctl_amd.eval_densities_host(name, xt, xs, xn, F, V_trg=V0.copy(), ctx=ctx_for(name))
            fresh = sctl_amd.eval_densities_host(name, xt, xs, xn, F, ctx=ctx_for(name))
            assert np.array_equal(U, V0 + fresh)                                                # accumulated into, one addition per entry
            one = sctl_amd.eval_densities_host(name, xt, xs, xn, F[:1].copy(), V_trg=V0[:1].copy(), ctx=ctx_for(name))
            assert np.array_equal(one[0], sctl_amd.eval_host(name, xt, xs, xn, F[0].copy(), v_trg=V0[0].copy(), ctx=ctx_for(name)))
            empty = np.zeros((0, 700 * info["k1"]), dtype=dt)
            assert sctl_amd.eval_densities_host(name, xt, xs, xn, np.zeros((0, 900 * info["k0"]), dtype=dt), V_trg=empty, ctx=ctx_for(name)).shape == (0, 700 * info["k1"])
    # nd == 0 through the C ABI leaves whatever v_trg holds untouched
    import ctypes
    x = np.random.default_rng(2).random(300)
    v = np.full(100, 7.0)
    assert sctl_amd.lib().sctl_amd_eval_densities_host(0, 0, 0, 100, 100, x.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), None,
                                                       x.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p), -1, None, 0, 0) == 0
    assert np.all(v == 7.0)


def test_counters_grow_as_nd_single_calls():
    rng = np.random.default_rng(3)
    info = sctl_amd.kernel_info("Stokes3D-FxU")
    xt, xs, xn, F = _inputs(rng, 1000, 2000, info, 11, np.float64)
    sctl_amd.reset_counters()
    sctl_amd.eval_densities_host("Stokes3D-FxU", xt, xs, xn, F)
    c = sctl_amd.counters()
    assert c["pair_interactions"] == 11 * 1000 * 2000 and c["sctl_flops"] == 11 * 1000 * 2000 * info["flops"]


def test_self_evaluation_is_finite_and_matches_the_oracle(O):
    rng = np.random.default_rng(5)
    for name in sctl_amd.KERNEL_NAMES:
        info = sctl_amd.kernel_info(name)
        for dt in (np.float64, np.float32):
            _, xs, xn, F = _inputs(rng, 1, 2000, info, 5, dt)
            U = sctl_amd.eval_densities_host(name, xs, xs, xn, F, ctx=ctx_for(name))
            assert np.all(np.isfinite(U)), name
            for m in range(5):
                assert rel_l2(U[m], O.eval(name, xs, xs, xn, F[m].copy(), ctx=ctx_for(name))) <= TOL[dt], (name, dt, m)


@pytest.mark.parametrize("name", ["Laplace3D-FxU", "Stokes3D-FxU"])
def test_digits_ladder(O, name):
    """each digits request within the bound the single-density path meets (tests/test_gpu_parity.py: test_digits_accuracy_ladder)"""
    info = sctl_amd.kernel_info(name)
    rng = np.random.default_rng(11)
    xt, xs, xn, F = _inputs(rng, 700, 1500, info, 4, np.float64)
    exact = [O.eval(name, xt, xs, xn, F[m].copy()) for m in range(4)]
    for d in (3, 7, 10, -1):
        U = sctl_amd.eval_densities_host(name, xt, xs, xn, F, digits=d)
        for m in range(4):
            assert rel_l2(U[m], exact[m]) <= (10.0 * 10.0 ** (-d) if d >= 0 else 5e-15), (d, m)
    # fp32 runs the exact pair at every digits: full fp32 accuracy also at digits 3
    U = sctl_amd.eval_densities_host(name, xt.astype(np.float32), xs.astype(np.float32), None, F.astype(np.float32), digits=3)
    for m in range(4):
        assert rel_l2(U[m], exact[m]) <= 2e-5


def _subset_check(O, name, xt, xs, xn, F, U, sel, tol):
    xsel = xt.reshape(-1, 3)[sel].ravel().astype(np.float64)
    k1 = sctl_amd.kernel_info(name)["k1"]
    for m in range(F.shape[0]):
        ref = O.eval(name, xsel, xs.astype(np.float64), None if xn is None else xn.astype(np.float64), F[m].astype(np.float64))
        got = U[m].reshape(-1, k1)[sel].ravel()
        assert rel_l2(got, ref) <= tol, (name, m, rel_l2(got, ref))


def test_split_heavy_plan_on_a_target_subset(O):
    """Laplace3D-FxU fp64, 8 densities, 2^14 targets against 2^20 sources: many source splits, reduced in order"""
    name, nd, Nt, Ns = "Laplace3D-FxU", 8, 1 << 14, 1 << 20
    pl = sctl_amd.plan_densities(name, 0, nd, Nt, Ns)
    assert pl["src_splits"] >= 8 and pl["src_splits"] % 8 == 0, pl
    rng = np.random.default_rng(21)
    xt, xs, xn, F = _inputs(rng, Nt, Ns, sctl_amd.kernel_info(name), nd, np.float64)
    U = sctl_amd.eval_densities_host(name, xt, xs, xn, F)
    _subset_check(O, name, xt, xs, xn, F, U, np.arange(0, Nt, Nt // 512), 1e-12)


def test_target_cut_plan_on_a_target_subset(O):
    """Stokes3D-FxT fp32, 8 densities at 2^20 x 2^20: the partial sums of all targets would pass 2 GB, so each pass cuts its targets into several
    launches (tests/test_densities_cpu.py checks the plan).  fp32 sums over 2^20 sources: bound 1e-4."""
    name, nd, N = "Stokes3D-FxT", 8, 1 << 20
    info = sctl_amd.kernel_info(name)
    pl = sctl_amd.plan_densities(name, 1, nd, N, N)
    assert pl["densities_per_pass"] * pl["src_splits"] * N * info["k1"] * 4 > 2 << 30 and pl["workspace_bytes"] <= 2 << 30, pl
    import torch
    g = torch.Generator(device="cuda").manual_seed(7)
    xt = torch.rand(N * 3, device="cuda", dtype=torch.float32, generator=g)
    xs = torch.rand(N * 3, device="cuda", dtype=torch.float32, generator=g)
    F = torch.rand((nd, N * 3), device="cuda", dtype=torch.float32, generator=g) - 0.5
    U = sctl_amd.eval_densities_device(name, xt, xs, None, F)
    torch.cuda.synchronize()
    sel = np.arange(0, N, N // 128) + 17
    _subset_check(O, name, xt.cpu().numpy(), xs.cpu().numpy(), None, F.cpu().numpy(), U.cpu().numpy(), sel, 1e-4)


def test_helmholtz_with_the_conftest_wavenumbers(O):
    from conftest import HELMHOLTZ_K
    rng = np.random.default_rng(9)
    info = sctl_amd.kernel_info("Helmholtz3D-FxU")
    for ctx in (np.array(HELMHOLTZ_K), np.array([HELMHOLTZ_K[0], 0.0])):   # complex and real wavenumber
        xt, xs, xn, F = _inputs(rng, 1500, 2500, info, 8, np.float64)
        U = sctl_amd.eval_densities_host("Helmholtz3D-FxU", xt, xs, xn, F, ctx=ctx)
        for m in range(8):
            assert rel_l2(U[m], O.eval("Helmholtz3D-FxU", xt, xs, xn, F[m].copy(), ctx=ctx)) <= 1e-12


def test_device_entry_on_a_side_stream():
    import torch
    rng = np.random.default_rng(13)
    name = "Stokes3D-DxU"
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, F = _inputs(rng, 3000, 5000, info, 6, np.float64)
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, xn, F)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        U = sctl_amd.eval_densities_device(name, *d)
    side.synchronize()
    Uh = sctl_amd.eval_densities_host(name, xt, xs, xn, F)
    assert np.array_equal(U.cpu().numpy(), Uh)


def test_operator_with_weights_and_target_normals_equals_per_row_eval():
    import torch
    devs = list(range(torch.cuda.device_count()))
    rng = np.random.default_rng(17)
    for name, dt in (("Stokes3D-DxU", np.float64), ("Stokes3D-FxU", np.float32), ("Laplace3D-FxU", np.float64)):
        info = sctl_amd.kernel_info(name)
        Nt, Ns, nd = 5000, 4000, 5
        xt, xs, xn, F = _inputs(rng, Nt, Ns, info, nd, dt)
        w = rng.random(Ns).astype(dt)
        op = sctl_amd.DirectOp(name, dtype=dt, devices=devs)
        op.set_targets(xt)
        op.set_sources(xs, xn)
        op.set_source_weights(w)
        if info["k1"] % 3 == 0:
            op.set_target_normals((rng.random(Nt * 3) - 0.5).astype(dt))
        U = op.eval_densities(F)
        V0 = (rng.random(U.shape) - 0.5).astype(dt)
        Uacc = op.eval_densities(F, V_trg=V0.copy(), accumulate=True)
        for m in range(nd):
            one = op.eval(F[m].copy())
            assert rel_l2(U[m], one) <= (1e-14 if dt == np.float64 else 1e-6), (name, m, rel_l2(U[m], one))
        assert np.array_equal(Uacc, V0 + U)
        op.close()


def test_plugin_kernel_falls_back_to_single_density_calls(tmp_path):
    import subprocess
    name = "Yukawa3D-FxU"
    try:
        sctl_amd.kernel_id(name)
    except KeyError:
        so = str(tmp_path / "libyukawa_kernel.so")
        libdir = os.path.join(ROOT, "sctl_amd")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "plugin", "yukawa_kernel.hip"), "-o", so, "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir], check=True)
        assert sctl_amd.load_plugin(so) == [name]
    rng = np.random.default_rng(19)
    info = sctl_amd.kernel_info(name)
    xt, xs, xn, F = _inputs(rng, 800, 1200, info, 4, np.float64)
    lam = np.array([2.5])
    pl = sctl_amd.plan_densities(name, 0, 4, 800, 1200)
    assert pl["densities_per_pass"] == 1 and pl["passes"] == 4
    U = sctl_amd.eval_densities_host(name, xt, xs, xn, F, ctx=lam)
    for m in range(4):
        assert np.array_equal(U[m], sctl_amd.eval_host(name, xt, xs, xn, F[m].copy(), ctx=lam))


def test_fp32_run_twice_is_bit_identical():
    rng = np.random.default_rng(23)
    info = sctl_amd.kernel_info("Stokes3D-FxUP")
    xt, xs, xn, F = _inputs(rng, 20000, 30000, info, 7, np.float32)
    a = sctl_amd.eval_densities_host("Stokes3D-FxUP", xt, xs, xn, F)
    b = sctl_amd.eval_densities_host("Stokes3D-FxUP", xt, xs, xn, F)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_cpp_host_surface_eval_densities_matches_eval(tmp_path):
    import subprocess
    exe = str(tmp_path / "densities_driver")
    libdir = os.path.join(ROOT, "sctl_amd")
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "densities_driver.cpp"),
                    "-L" + libdir, "-lsctl_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    N, nd = 2000, 6
    out = str(tmp_path / "o.bin")
    p = subprocess.run([exe, str(N), str(nd), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    raw = np.fromfile(out, dtype=np.float64).reshape(2, nd, N * 3)
    for m in range(nd):
        assert rel_l2(raw[0, m], raw[1, m]) <= 1e-14
