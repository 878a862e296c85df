"""What tests/test_gpu_derivative_pairs.py rests on, checked without a GPU: the symbolic truth of tests/pair_truth.py against the project's own formulas
and against 40-digit arithmetic, the probe geometry, and that the measure with its bar of 4 x the yardstick sees a planted fault."""
import numpy as np
import pytest

import pair_truth as pt
import sctl_amd
from grad_truth import HELMHOLTZ_KS, gradients
from pair_truth import LD

KERNELS = sctl_amd.KERNEL_NAMES
DTYPES = [np.float64, np.float32]


def cases():
    """(kernel, wavenumber) pairs: Helmholtz at its four wavenumbers"""
    return [(n, None) for n in KERNELS if not n.startswith("Helmholtz")] + [("Helmholtz3D-FxU", k) for k in HELMHOLTZ_KS]


CASE_IDS = ["%s%s" % (n, "" if k is None else "-k=%g%+gi" % k) for n, k in cases()]


def test_kernel_table_is_the_library_s():
    assert list(pt.KERNELS) == list(KERNELS)
    for name, (K0, K1, has_n, _) in pt.KERNELS.items():
        info = sctl_amd.kernel_info(name)
        assert (info["k0"], info["k1"], info["nd"]) == (K0, K1, 3 if has_n else 0), name


def test_long_double_and_constants():
    """the 64-bit significand; pi and the scale factors are long doubles, not doubles; the expressions hold integers and dyadic rationals only"""
    import sympy as sp
    assert np.finfo(LD).nmant >= 63 and np.finfo(LD).eps < 2e-19
    assert pt.PI.dtype == LD and pt.PI != LD(np.pi) and abs(pt.PI - LD(np.pi)) < LD(2.0) ** -52
    for name in KERNELS:
        s = pt.scale_of(name, LD)
        assert s.dtype == LD and s != LD(float(s))
        assert pt.scale_of(name, np.float32).dtype == np.float32
        U, DU, NU, _ = pt.symbolic(name)            # (symbolic() itself asserts the constants)
        flat = list(U) + [x for r in DU for c in r for x in c]
        assert not any(e.has(sp.pi) or e.atoms(sp.Float) for e in flat)
    with pytest.raises(AssertionError):
        pt._dyadic_only(sp.Symbol("x") / 3)
    with pytest.raises(AssertionError):
        pt._dyadic_only(sp.Symbol("x") * sp.pi)


@pytest.mark.parametrize("dt", [LD, np.float64, np.float32], ids=["ld", "f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_every_array_keeps_the_type_it_was_called_with(name, dt):
    """truth in long double, yardstick in the working precision: no expression falls back to double on the way"""
    k = HELMHOLTZ_KS[0] if name.startswith("Helmholtz") else None
    c = pt.launch(name, np.float32, "trg", 0, 3, k=k)
    cast = lambda a: None if a is None else a.astype(dt)
    v = pt.pair_values(name, cast(c["d"]), cast(c["n"]), cast(c["e"]), cast(c["m"]), cast(c["f_pair"]), cast(c["w_pair"]), k=k)
    for key, a in v.items():
        assert a is None or a.dtype == dt, (key, a.dtype)
    for a in pt.tensors(name, cast(c["d"]), cast(c["n"]), k):
        assert a is None or a.dtype == dt


# ---- the truth is the project's formula -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", cases(), ids=CASE_IDS)
def test_truth_equals_the_project_s_autograd_truth(name, k):
    """Contracted over the probe pairs of one launch (all three zones, r from 2^-40 to 2^10), the symbolic truth equals torch autograd of
    grad_truth.kernel_blocks (gradients) and torch.func.jvp of it (test_gpu_jvp.truth) to 1e-13 of the majorant"""
    from test_gpu_jvp import truth as jvp_truth
    ctx = None if k is None else np.array(k)
    # targets around one source: g_trg and the tangent per pair
    c = pt.launch(name, np.float64, "trg", 0, 11, n_streamed=1, k=k)
    tr, _ = pt.truth_and_yardstick(name, c)
    g_trg, g_src, _, _ = gradients(name, c["xt"], c["xs"], c["xn"], c["f"], c["w"], ctx)
    du = jvp_truth(name, c["xt"], c["xs"], c["xn"], c["f"], c["dxt"], c["dxs"], c["dxn"], ctx)
    worst = {}
    worst["g_trg"] = pt.q_of(g_trg.reshape(-1, 3), tr["g_trg"], tr["maj_g"], 1.0).max()
    worst["du"] = pt.q_of(du.reshape(c["Nt"], -1), tr["du"], tr["maj_du"], 1.0, pt.tangent_groups(name)).max()
    total = tr["g_trg"].sum(axis=0)
    assert np.all(np.abs(g_src.astype(LD) + total) <= 1e-12 * np.abs(tr["g_trg"]).sum(axis=0))
    # sources around one target: g_src and g_nrm per pair
    c = pt.launch(name, np.float64, "src", 0, 12, n_streamed=1, k=k)
    tr, _ = pt.truth_and_yardstick(name, c)
    _, g_src, g_nrm, _ = gradients(name, c["xt"], c["xs"], c["xn"], c["f"], c["w"], ctx)
    worst["g_src"] = pt.q_of(-g_src.reshape(-1, 3), tr["g_trg"], tr["maj_g"], 1.0).max()
    if g_nrm is not None:
        worst["g_nrm"] = pt.q_of(g_nrm.reshape(-1, 3), tr["g_nrm"], tr["maj_n"], 1.0).max()
    print(name, k, {a: "%.1e" % b for a, b in worst.items()})
    assert all(v <= 1e-13 for v in worst.values()), worst


@pytest.mark.parametrize("name,k", cases(), ids=CASE_IDS)
def test_long_double_truth_against_40_digits(name, k):
    """a dozen pairs per kernel, the nearest and the farthest among them: the same sympy expressions in mpmath at 40 digits agree with the long-double
    arrays to 1e-17 of the majorant"""
    c = pt.launch(name, np.float64, "src", 0, 21, k=k)
    tr, _ = pt.truth_and_yardstick(name, c)
    order = np.argsort(c["r"])
    order = order[c["r"][order] > 0]
    pick = order[np.unique(np.linspace(0, order.size - 1, 12).astype(int))]
    assert pick.size == 12 and pick[0] == order[0] and pick[-1] == order[-1]
    L = lambda key, i: None if c[key] is None else c[key][i].astype(LD)
    worst = 0.0
    for i in pick:
        du, g, gn = pt.mp_pair_values(name, L("d", i), L("n", i), L("e", i), L("m", i), L("f_pair", i), L("w_pair", i), k)
        for mp, val, maj, groups in ((du, tr["du"][i], tr["maj_du"][i], pt.tangent_groups(name)), (g, tr["g_trg"][i], tr["maj_g"][i], None),
                                     (gn, None if gn is None else tr["g_nrm"][i], None if gn is None else tr["maj_n"][i], None)):
            if mp is None:
                continue
            for cols in groups or (list(range(len(mp))),):
                a = max(maj[j] for j in cols)
                # the difference is taken in mpmath: the long double enters exactly as two doubles
                import mpmath
                with mpmath.workdps(40):
                    for j in cols:
                        x = mpmath.mpf(float(val[j])) + mpmath.mpf(float(val[j] - LD(float(val[j]))))
                        worst = max(worst, float(abs(x - mp[j]) / mpmath.mpf(float(a))))
    print(name, k, "largest difference / majorant %.2e" % worst)
    assert worst <= 1e-17


# ---- the geometry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["Laplace3D-FDxUdU", "Stokes3D-FxT", "Helmholtz3D-FxU"])
def test_probe_geometry(name, dt):
    """every launch of the masked shape: 300 owners x 600 streamed points, live slots {0, 255, 256, 599}, at least 64 probes per zone, exactly one
    coincident owner, every d and e formed exactly, every dead density or weight +0.0 with nonzero tangents and normals beside it, nothing excluded,
    and a yardstick q that is finite and nonzero in every zone"""
    k = HELMHOLTZ_KS[0] if name.startswith("Helmholtz") else None
    assert pt.LIVE_SLOTS(pt.N_STREAMED) == (0, 255, 256, 599)
    lo = 2.0 ** (-14 if dt == np.float32 else -40)
    for side in ("trg", "src"):
        for i, slot in enumerate(pt.LIVE_SLOTS(pt.N_STREAMED)):
            c = pt.launch(name, dt, side, slot, 100 + i, k=k)
            assert (c["Nt"], c["Ns"]) == ((300, 600) if side == "trg" else (600, 300))
            assert c["exact"] and c["live"] == slot
            z = pt.zones_of(c["r"])
            assert (z == -1).sum() == 1 and all((z == j).sum() >= 64 for j in range(3)), np.bincount(z + 1)
            r = c["r"][c["r"] > 0]
            assert r.min() >= lo * 0.99 and r.max() <= (8.0 if k else 1024.0) * 1.01
            assert np.all((c["d"] == 0).all(axis=1) == (c["r"] == 0))
            dead = c["f"] if side == "trg" else c["w"]
            per = dead.size // pt.N_STREAMED
            dead = np.delete(dead.reshape(-1, per), slot, axis=0)
            assert np.all(dead == 0) and not np.signbit(dead).any()
            assert np.all((c["f"] if side == "trg" else c["w"]).reshape(-1, per)[slot] != 0)
            for key in ("dxt", "dxs", "dxn", "xn"):
                assert c[key] is None or np.all(c[key] != 0)
            tr, ya = pt.truth_and_yardstick(name, c)
            amp = pt.helmholtz_amp(k, c["r"]) if k else None
            for key, mk, groups in (("du", "maj_du", pt.tangent_groups(name)), ("g_trg", "maj_g", None), ("g_nrm", "maj_n", None)):
                if tr[key] is None:
                    continue
                q = pt.q_of(ya[key], tr[key], tr[mk], pt.EPS[np.dtype(dt)], groups, amp)
                assert q.shape == (300,) and np.all(np.isfinite(q)) and q[z == -1][0] == 0          # every owner has a q: no probe is excluded
                assert all(q[z == j].max() > 0 for j in range(3))


def test_unmasked_geometry():
    """the 20077-owner set of the unmasked shape: thousands of probes per zone, one coincident owner, exact differences in both precisions"""
    for dt in DTYPES:
        x, r = pt.owners(dt, 20077, 9)
        z = pt.zones_of(r)
        assert (z == -1).sum() == 1 and all((z == j).sum() >= 6000 for j in range(3))
        assert pt.differences_exact(x, np.ascontiguousarray(np.broadcast_to(pt.P.astype(dt), x.shape)))


# ---- the measure has teeth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name,k", cases(), ids=CASE_IDS)
def test_planted_faults_exceed_the_bar(name, k, dt):
    """The yardstick with a fault planted into it lies above 4 x the clean yardstick, the bar of the GPU test, in every zone and every output that
    contains the faulty term: (a) the root (R and 1/R) carrying a relative error of 8 eps (eps = 2^-52 or 2^-23, the type's epsilon), in every
    output; (b) the radial coefficient of the derivative, the -p of every term P r^-p (the 5 of Laplace3D-FDxUdU's 5 P5 y^2 among them), off by
    2^-30 (fp64) or 2^-12 (fp32), in the tangent and the coordinate gradient (the normal gradient has no such term)."""
    eps_type = float(np.finfo(dt).eps)
    c = pt.launch(name, dt, "trg", 256, 31, k=k)
    tr, ya = pt.truth_and_yardstick(name, c)
    args = (c["d"], c["n"], c["e"], c["m"], c["f_pair"], c["w_pair"])
    z = pt.zones_of(c["r"])
    amp = pt.helmholtz_amp(k, c["r"]) if k else None
    faults = {"root 8 eps": (dict(root_error=8 * eps_type), ("du", "g_trg", "g_nrm")),
              "radial coefficient": (dict(c=1 + (2.0 ** -30 if dt == np.float64 else 2.0 ** -12)), ("du", "g_trg"))}
    for what, (kw, keys) in faults.items():
        bad = pt.pair_values(name, *args, k=k, **kw)
        for key in keys:
            if tr[key] is None:
                continue
            mk = {"du": "maj_du", "g_trg": "maj_g", "g_nrm": "maj_n"}[key]
            groups = pt.tangent_groups(name) if key == "du" else None
            q0 = pt.q_of(ya[key], tr[key], tr[mk], pt.EPS[np.dtype(dt)], groups, amp)
            q1 = pt.q_of(bad[key], tr[key], tr[mk], pt.EPS[np.dtype(dt)], groups, amp)
            for j in range(3):
                a, b = q0[z == j].max(), q1[z == j].max()
                print("%s %s %s %s, %s: clean %.2f, faulty %.3g" % (name, k, dt.__name__, what, pt.ZONE_NAMES[j], a, b))
                assert b > 4 * a, (what, key, pt.ZONE_NAMES[j], a, b)
