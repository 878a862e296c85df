"""What tests/test_gpu_centred_pairs.py rests on that can be wrong without a device: the long-double pair formulas (against the CPU oracle, all
ten kernels), the probes of tests/centred_pair_shapes.py (each on the side of the near radius it claims, in long double and in the form's own
precision with the device's worst rounding against it; the fold's band densities on the side of 2^+-600 they claim), where the live source lands
among the tiles, groups and leftovers, and the planner's word that every launch runs tile-centred."""
import os

import numpy as np
import pytest

import sctl_amd
import centred_pair_shapes as S
from conftest import ctx_for
from test_gpu_centered import _CENTRED_FORMS

LD = np.longdouble
FORM_IDS = ["%s-%s" % (n, np.dtype(d).name) for n, d in _CENTRED_FORMS]


def test_long_double_is_wider_than_the_device():
    assert np.finfo(LD).eps < 2e-19


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_long_double_formulas_agree_with_the_oracle(O, name):
    """300 random pairs per kernel, one source at a time with a generic density.  Bound: the oracle's own worst case in units of 2^-53
    (centred_pair_shapes: 4.5 per power of 1 / r, the products of the power, the numerator's roundings), relative to the pair's own conditioning;
    Helmholtz: the 16 half-ulps of tests/test_gpu_helmholtz_pairs.py times 1 + |k| r, the weight of r's error in e^{ikr}."""
    info = sctl_amd.kernel_info(name)
    rng = np.random.default_rng(sctl_amd.KERNEL_NAMES.index(name))
    ctx = ctx_for(name)
    xt = rng.random((300, 3))
    worst = 0.0
    for s in range(3):
        x = rng.random(3) * (1.0, 1e-3, 10.0)[s]
        n = rng.random(3) - 0.5 if info["nd"] else None
        f = rng.random(info["k0"]) - 0.5
        u, ua = S.pair_values(name, xt, x, n, f, ctx)
        ref = O.eval(name, xt.ravel().copy(), x.copy(), n, f, ctx=ctx).reshape(300, -1)
        q, _ = S.measure(ref, u, ua, np.float64)
        if name.startswith("Helmholtz"):
            r = np.sqrt(((xt - x) ** 2).sum(-1))
            bound = 16.0 * (1 + (abs(ctx[0]) + abs(ctx[1])) * r)
        else:
            bound = S.w_yardstick(name, np.float64)
        worst = max(worst, float((q / bound).max()))
        assert np.all(q <= bound), (name, s, float((q / bound).max()))
    print("oracle q / worst case: %.2f  %s" % (worst, name))


@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_coincident_pairs_give_zero(name):
    info = sctl_amd.kernel_info(name)
    xt = np.random.default_rng(3).random((5, 3))
    u, ua = S.pair_values(name, xt, xt[2], np.array([0.1, 0.2, 0.3]) if info["nd"] else None, np.ones(info["k0"]), ctx_for(name))
    assert np.all(u[2] == 0) and np.all(ua[2] == 0) and np.all(u[[0, 1, 3, 4]] != 0) and np.all(np.isfinite(u))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_probes_are_on_the_side_of_the_near_radius_they_claim(dt):
    u = float(S.unit_of(dt))
    for kind, w in S.waves_for(dt).items():
        # the centre is the kernel's expression; one bounding-box extent of the flat cloud is 0
        assert np.array_equal(w.c, dt(0.5) * w.xt.min(0) + dt(0.5) * w.xt.max(0)) and w.xt.dtype == dt and w.xt.shape == (S.NT_A, 3)
        assert (w.xt[:, 2].min() == w.xt[:, 2].max()) == (kind == "flat")
        assert abs(float(w.rt2) / float(w.rt2_ld) - 1) <= 5 * u
        assert len(w.probes) == 3 * len(S.RHOS) + 2
        seen = set()
        for p in w.probes:
            ss, ss_ld = S.ss_of(p.x, w.c), ((p.x.astype(LD) - w.c_ld) ** 2).sum()
            lim, lim_ld = dt(S.NEAR_FACTOR2) * w.rt2, LD(S.NEAR_FACTOR2) * w.rt2_ld
            # the device's |x_s'|^2 and Rt^2 are within 5 u each of these: 10 u of slack against the claim (module docstring of the shapes)
            if p.zone == "near":
                assert ss_ld <= lim_ld and float(ss) * (1 + 10 * u) <= float(lim), (kind, p)
                assert not S.is_far(p.x, w) and not S.is_far_ld(p.x, w)
            else:
                assert ss_ld > lim_ld and float(ss) * (1 - 10 * u) > float(lim), (kind, p)
                assert S.is_far(p.x, w) and S.is_far_ld(p.x, w)
            if p.kind == "rho":
                rho = float(np.sqrt(ss_ld / w.rt2_ld))
                want = float(S.rho_value(p.rho, dt))
                assert abs(rho / want - 1) <= (2.0 ** -12 if kind == "offset" else 1e-6) and p.zone == S.zone_of(p.rho), (kind, p, rho)
                if p.rho in ("2-", "2+"):                # the edge probes: within 4 eps of the radius, and still resolved
                    assert 0.5 * S.eps_of(dt) < abs(rho / 2 - 1) < 2 * S.eps_of(dt), (kind, p, rho)
                seen.add((p.rho, p.direction))
            elif p.kind == "coincident":
                assert np.array_equal(p.x, w.xt[S.T_REF])
            else:
                r = float(np.sqrt(((p.x.astype(LD) - w.xt[S.T_REF].astype(LD)) ** 2).sum()))
                rt = float(np.sqrt(w.rt2_ld))
                assert 0 < r <= max(3 * S.close_distance(dt) * rt, 2 * float(np.spacing(np.abs(w.xt[S.T_REF]).max()))), (kind, r)
        assert seen == {(rho, d) for rho in S.RHOS for d in ("axis", "diagonal", "random")}
        far = np.array([bool(S.is_far(x, w)) for x in w.dead])
        assert np.array_equal(np.flatnonzero(~far), np.array(S.DEAD_NEAR)) and all(S.is_far_ld(x, w) == f for x, f in zip(w.dead, far))


def test_fold_band_densities_straddle_the_band():
    w = S.waves_for(np.float64)["cube"]
    p = [q for q in w.probes if q.rho == 3.0 and q.direction == "random"][0]
    ss = ((p.x.astype(LD) - w.c_ld) ** 2).sum()
    got = S.fold_band_densities(p.x, w)
    assert [r for _, _, r in got[:4]] == ["fold", "exact", "exact", "fold"] and {r for _, _, r in got[4:]} == {"exact"}
    for label, f, route in got:
        kss = ss / (LD(f) * LD(f))
        inside = LD(2) ** -600 <= kss <= LD(2) ** 600
        assert inside == (route == "fold") == (S.fold_route(f, p.x, w) == "fold"), (label, f)
        k = 1.0 / (f * f)
        assert 2.0 ** -900 <= k <= 2.0 ** 900                 # fold_prepass.hpp: a record, not an exception: the wave decides
        if "edge" in label:                                   # just inside or just outside: 2^-9 from the edge, far above the roundings of k |x_s'|^2
            edge = LD(2) ** (600 if "low" in label else -600)
            assert 2.0 ** -10 < abs(float(kss / edge) - 1) < 2.0 ** -8, (label, float(kss / edge))
    assert {np.sign(f) for _, f, _ in got} == {1.0, -1.0}      # both sign lists


@pytest.mark.parametrize("form", _CENTRED_FORMS, ids=FORM_IDS)
def test_live_sources_reach_tiles_groups_and_leftovers(form):
    name, dt = form
    f64 = np.dtype(dt) == np.float64
    info = sctl_amd.kernel_info(name)
    waves = S.waves_for(dt)
    la = S.launches_a(name, dt, waves)
    assert 60 <= len(la) <= 85 and len(S.launches_b(name, dt)) == len(S.RHOS) + 1
    assert S.NS_A % 64 and S.NS_A % 32 and 64 <= S.NS_A <= 193 and S.NS_B % 64 and S.NS_B % 32
    fold = name == "Laplace3D-FxU" and f64
    for pipe in sorted({p for p, _ in S.modes_of(name, dt)}):
        slots, zones, dens, near_tiles = set(), set(), set(), set()
        for L in la:
            assert L.xs.shape == (S.NS_A, 3) and L.xs.dtype == dt and L.f.shape == (S.NS_A, info["k0"]) and (L.xn is None) == (info["nd"] == 0)
            assert np.array_equal(L.xs[L.live], L.probe.x)
            filled = L.label.startswith("filled")
            if not filled:
                assert np.count_nonzero(L.f.any(axis=1)) == 1 and L.f[L.live].any()      # exactly one live source
            w = waves[L.cloud]
            zones.add(L.zone)
            dens.add(tuple(np.sign(L.f[L.live])) + (float(np.abs(L.f[L.live]).max()),))
            if L.zone == "near":
                near_tiles.add(L.live // S.WAVE_TILE)
            elif L.route != "exact":
                slots.add(S.far_slot(L.xs, L.live, w, pipe, f64, L.f if fold else None) + (np.sign(L.f[L.live, 0]) if fold else 0,))
        assert zones == set(S.ZONES) and near_tiles == {0, 1, 2}
        kinds = {(t, k) for t, k, _ in slots}
        if fold:      # one live record per list is its leftover; the filled launches reach the groups of 4 and a later tile; both sign lists
            assert {(0, "leftover"), (0, "group")} <= kinds and {s for _, _, s in slots} == {1.0, -1.0}
            assert any(t > 0 for t, _ in kinds) or S.NS_A * 2 // 3 < S.WAVE_TILE + 30
        else:         # first and last tile; a full group and the leftovers
            assert {t for t, _ in kinds} == {0, 1, 2} and {k for _, k in kinds} == {"group", "leftover"}, (pipe, sorted(kinds))
        mags = {m for *_, m in dens}
        if info["k0"] == 1:
            assert {(1.0, 1.0), (-1.0, 1.0)} <= dens and {np.float64(dt(3e-7)), np.float64(dt(2.5e9))} <= mags
        else:
            for k in range(info["k0"]):      # every unit vector, and a generic one
                assert any(np.count_nonzero(s[:-1]) == 1 and s[k] != 0 for s in dens)
            assert any(np.count_nonzero(s[:-1]) == info["k0"] for s in dens)


@pytest.mark.parametrize("form", _CENTRED_FORMS, ids=FORM_IDS)
def test_every_launch_is_planned_tile_centred(form):
    name, dt = form
    real = 0 if np.dtype(dt) == np.float64 else 1
    old = {k: os.environ.get(k) for k in ("SCTL_AMD_CENTERED", "SCTL_AMD_MFMA_F32")}
    try:
        for pipe, digits in S.modes_of(name, dt):
            for nt, ns in ((S.NT_A, S.NS_A), (S.NT_B, S.NS_B)):
                os.environ["SCTL_AMD_CENTERED"] = "1"
                os.environ.pop("SCTL_AMD_MFMA_F32", None)
                if real == 1 and pipe == "valu":
                    os.environ["SCTL_AMD_MFMA_F32"] = "0"
                pl = sctl_amd.plan(name, real, nt, ns, digits=digits)
                assert pl["path"] == "tile-centred" and pl["pipe"].startswith("bf16 matrix cores") == (pipe == "mfma"), (name, pipe, digits, pl)
                assert pl["src_splits"] == 1                                     # one split: the live index is the index within the wave's source stream
                assert (pl["workgroups"] == 1) == (nt == S.NT_A), pl            # Geometry A is ONE wave, Geometry B several
                os.environ["SCTL_AMD_CENTERED"] = "0"
                assert sctl_amd.plan(name, real, nt, ns, digits=digits)["path"] == "exact"
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    # every form has a case, and the default mode of every fp32 form runs on the matrix cores
    assert ("mfma", -1) in S.modes_of(name, dt) or real == 0
