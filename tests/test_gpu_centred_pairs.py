"""The tile-centred kernels (sctl_amd/csrc/centered_kernel.hpp, centered_mfma_kernel.hpp) one pair at a time, at the near / far edge, against long
double: all thirteen (kernel, precision) forms of tests/test_gpu_centered.py::_CENTRED_FORMS in every accuracy mode they serve.

The sums the other tests of these kernels compare (rel-L2 over 1e2 - 1e5 sources) cannot see one far pair that is wrong by 1e-10, a source just
inside the near radius that is treated as far, or a folded record on the wrong side of the band test.  Here ONE source carries the density and
every other source an exact zero, so each target's output is the device's value of one pair; the dead sources still fill the tiles, the 32-row
contraction block and the carried leftovers.  SCTL_AMD_CENTERED=1 sends these small problems down the tile-centred path, which every launch
asserts through sctl_amd.plan first.

tests/centred_pair_shapes.py holds the geometry (one wave whose centre the test restates, then several waves whose centres it does not know), the
truth, the measure q, the derivation of the bars and the reason for the one factor the measure takes out (the conditioning kappa of the pair's own
formula).  In short, full precision: per zone of rho = |x_s - c| / Rt the device may have FACTOR(zone) times the largest q of a yardstick that is
not the code under test — the CPU oracle in fp64, the exact fp32 kernel in fp32 — with FACTOR = worst-case rounding count of the device in that
zone / that of the yardstick; near-zone pairs get the exact kernel's count, so a near pair that only meets the far bar fails.  Lower modes: the
project's 10 * 10^-digits per pair.  A coincident pair must be exactly 0 in every output; a non-finite value fails.

Each case prints, per zone, the derived worst case, the factor, the yardstick's q, the exact device kernel's q (SCTL_AMD_CENTERED=0, the same
launches) and the tile-centred kernel's q; profiles/r22_centred_pairs.txt is that output from an MI355X.

What one live source cannot reach: the fp64 single layer drops sources of density 0 before its far lists are made, so its live record is always
the single leftover of its sign's list.  Its unrolled groups of 4 are probed with dead densities of +-2^-200 instead, which fill both lists and
stay 2^-140 below the live term (centred_pair_shapes.launches_a)."""
import contextlib
import os

import numpy as np
import pytest

import sctl_amd
import centred_pair_shapes as S
from test_gpu_centered import _CENTRED_FORMS

pytestmark = pytest.mark.gpu

CASES = [(name, dt, pipe, digits) for name, dt in _CENTRED_FORMS for pipe, digits in S.modes_of(name, dt)]


def _id(c):
    return "%s-%s-%s-d%d" % (c[0], np.dtype(c[1]).name, c[2], c[3])


def test_long_double_is_wider_than_the_device():
    assert np.finfo(np.longdouble).eps < 2e-19


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _flat(a):
    return None if a is None else np.ascontiguousarray(a).reshape(-1)


def _run(name, dt, pipe, digits, L, centred):
    """the launch's K1 values per target from the tile-centred kernel of the case, or from the exact kernel"""
    real = 0 if np.dtype(dt) == np.float64 else 1
    env = {"SCTL_AMD_CENTERED": "1" if centred else "0"}
    if real == 1 and pipe == "valu":
        env["SCTL_AMD_MFMA_F32"] = "0"
    with _env(**env):
        pl = sctl_amd.plan(name, real, L.xt.shape[0], L.xs.shape[0], digits=digits)
        if centred:
            assert pl["path"] == "tile-centred", pl
            assert pl["pipe"].startswith("bf16 matrix cores") == (pipe == "mfma"), pl
        else:
            assert pl["path"] == "exact", pl
        u = sctl_amd.eval_host(name, _flat(L.xt), _flat(L.xs), _flat(L.xn), _flat(L.f), digits=digits)
    return u.reshape(L.xt.shape[0], -1)


def _launches(name, dt):
    return S.launches_a(name, dt, S.waves_for(dt)) + S.launches_b(name, dt)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_pair_of_the_tile_centred_forms(O, case):
    name, dt, pipe, digits = case
    f64 = np.dtype(dt) == np.float64
    full = S.full_precision(dt, digits)
    zones = S.ZONES + ("any",)
    q_dev, q_yard, q_exact, e_dev, worst = ({z: 0.0 for z in zones} for _ in range(5))
    where = {z: "" for z in zones}
    routes = []
    for L in _launches(name, dt):
        x, n, f = L.xs[L.live], None if L.xn is None else L.xn[L.live], L.f[L.live]
        u, ua = S.pair_values(name, L.xt, x, n, f)
        dev = _run(name, dt, pipe, digits, L, True)
        exact = _run(name, dt, pipe, digits, L, False)
        if L.probe.kind == "coincident":
            assert np.all(dev[S.T_REF] == 0) and np.all(u[S.T_REF] == 0), (L.label, dev[S.T_REF])
        qd, ed = S.measure(dev, u, ua, dt)
        qx, _ = S.measure(exact, u, ua, dt)
        if f64:
            ref = O.eval(name, _flat(L.xt), _flat(x), _flat(n), _flat(f)).reshape(dev.shape)
            qy, _ = S.measure(ref, u, ua, dt)
        else:
            qy = qx
        z = L.zone
        if qd.max() > q_dev[z]:
            where[z] = "%s, live source %d, target %d" % (L.label, L.live, int(np.argmax(qd)))
        q_dev[z], q_yard[z], q_exact[z], e_dev[z] = max(q_dev[z], qd.max()), max(q_yard[z], qy.max()), max(q_exact[z], qx.max()), max(e_dev[z], ed.max())
        if L.route is not None:
            routes.append("%s -> %s (q %.2f)" % (L.label, L.route, qd.max()))
    failed = []
    for z in zones:
        zb = "just_far" if z == "any" else z          # Geometry B: the wave's own centre is not known here, so the largest bar
        w_dev, w_yard, fac = S.w_device(name, dt, pipe, zb), S.w_yardstick(name, dt), S.factor(name, dt, pipe, zb)
        print("CPAIRS %-34s %-9s W_dev %6.2f W_yard %6.2f FACTOR %5.2f | yardstick q %8.2f  exact kernel q %8.2f  tile-centred q %8.2f  e %.2e | %s"
              % (_id(case), z, w_dev, w_yard, fac, q_yard[z], q_exact[z], q_dev[z], e_dev[z], where[z]))
        if full:
            if q_dev[z] > fac * q_yard[z]:
                failed.append((z, q_dev[z], fac * q_yard[z], where[z]))
        elif e_dev[z] > 10.0 * 10.0 ** -digits:
            failed.append((z, e_dev[z], 10.0 * 10.0 ** -digits, where[z]))
    for r in routes:
        print("CPAIRS %-34s route  %s" % (_id(case), r))
    assert not failed, failed


@pytest.mark.parametrize("name,dt,pipe", [("Laplace3D-DxU", np.float64, "valu"), ("Stokes3D-FxU", np.float32, "mfma")], ids=["DxU-f64", "Stokeslet-f32"])
def test_a_pair_does_not_depend_on_its_neighbours(name, dt, pipe):
    """Two launches that differ only in WHERE the dead sources are (all of them far both times, so the tile layout, the far ranks and the near list
    are the same): the live pair's values must agree bit for bit.  A lane that read another row's record or contraction would show here."""
    w = S.waves_for(dt)["cube"]
    info = sctl_amd.kernel_info(name)
    rt = np.sqrt(w.rt2_ld)
    deads = [S.dead_sources(w.c_ld, rt, S.NS_A, dt, np.random.default_rng([31, k]), near=()) for k in range(2)]
    assert not np.array_equal(deads[0], deads[1])
    dens = S.density_cycle(info["k0"], dt)
    bits = np.int64 if np.dtype(dt) == np.float64 else np.int32
    for j, p in enumerate([q for q in w.probes if q.direction == "random" and q.rho in (1.0, "2+", 2.1, 10.0, 1e4)]):
        idx = S.INDEX_CYCLE[j]
        out = []
        for dead in deads:
            assert all(S.is_far_ld(x, w) and S.is_far(x, w) for x in dead)
            xs, xn, F = S._sources(dead, p, idx, info, dens[j % len(dens)], S.normal_for(0, w.xt[S.T_REF], p.x, dt), dt)
            L = S.Launch("A", "cube", w.xt, xs, xn, F, idx, p, p.zone, "independence", None)
            out.append(_run(name, dt, pipe, -1, L, True))
        assert np.count_nonzero(out[0]) >= out[0].size - 2
        assert np.array_equal(out[0].view(bits), out[1].view(bits)), (name, p.rho)
