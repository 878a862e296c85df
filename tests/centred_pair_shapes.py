"""Shapes, truth and bars of the pair-by-pair probe of the tile-centred kernels (tests/test_gpu_centred_pairs.py; checked without a GPU by
tests/test_centred_pairs_cpu.py).

A launch has ONE live source; every other source has a density of exactly 0, so a target's output is the device's value of one pair.

Geometry A is one wave: Nt = 128 targets (every form's wave owns 128, 192 or 256; tail lanes repeat the last target, which does not move the
bounding box), so this module can restate what the kernel computes (centered_kernel.hpp, "targets of this lane, cluster centre and radius"):
    c = 0.5 min + 0.5 max per axis,   Rt^2 = max |x_t - c|^2,   near  <=>  |x_s - c|^2 <= 4 Rt^2
in the form's own precision and in long double.  c is restated BIT FOR BIT: 0.5 x is exact and the sum is one correctly rounded operation, fused
or not, so the device's centre is the value computed here and its rounding is no error at all (any point serves as a centre).  What the device
may round differently is p = x - c (one rounding per component: relative u each, 2 u on a square) and |p|^2 (three more roundings, fused or not:
3 u), 5 u on Rt^2 and 5 u on |x_s'|^2, u the unit roundoff of the precision.  A probe at rho = 2 (1 -+ eps) has |x_s'|^2 / (4 Rt^2) = 1 -+ 2 eps,
so the device cannot decide otherwise than this module once 2 eps > 10 u plus the relative spacing of the coordinate grid at the source (the
probe is rounded to the grid after it is placed; at the offset clouds that spacing is u |offset| / Rt ~ 1e-10 in fp64 and ~ 1e-5 in fp32).
EPS = 2^-24 (fp64) and 2^-9 (fp32) are 2^8 and more above both; nothing was tuned, and the CPU test verifies each probe's side in long double and
in the form's precision with the 10 u of slack applied against it.

Measure (per pair, the norm over the pair's K1 outputs):
    q = |u_dev - u_true| / (max(|u_true|, smallest normal) unit kappa),     unit = 2^-53 or 2^-24,
    kappa = |u_abs| / |u_true| >= 1,  u_abs the same formula with every factor replaced by its absolute value and every sum taken unsigned.
kappa is the condition number of the pair's own formula under rounding of its factors (the running error bound of a sum of products).  It is 1
for the single layer and 1 - 3 for nearly every other pair, but no arithmetic, the oracle's included, can do better than kappa units where
(x_t - x_s).n or (x_t - x_s).f cancels: the probes with a normal ORTHOGONAL to x_t - x_s have kappa ~ 1e16 at the probed target by construction.
Taking kappa out is what keeps those pairs in the maximum (the Helmholtz probe takes out 1 + |k| r in the same way).  Cancellation that the
tile-centred forms ADD (the expanded r^2, x_t' sum A - sum A x_s', x_t'.nf - x_s'.nf) is not in kappa: it is in the bars below.

Truth: tests/test_independent_math.py::_kernel_values (the reference's formulas, written once, independent of the device code) in np.longdouble
on the inputs as the device gets them (fp32 inputs widened), r from the exact coordinate differences; Helmholtz, which has no tile-centred form
and is only compared with the oracle on the CPU, is added here.

Bars, in units of `unit`, worst case of every rounding (nothing measured on the device enters):
  per power of 1 / r   oracle 4.5: d = x_t - x_s 1 per component -> 2 on r^2, its three products and two sums 3, sqrt halves (2.5) and adds 1,
                         the division 1;
                       exact device kernel 7.5 (fp64): r^2 as above with FMAs (5 -> 2.5) + the refined reciprocal square root, 2.5 ulp = 5
                         (profiles/r03_rsq_refine_accuracy.txt); fp32 4.5: 2.5 + v_rsq_f32's 1 ulp = 2;
                       far, vector pipe 12.25 (fp64) / 9.25 (fp32): the header's 14.5 on the expanded four-FMA r^2 -> 7.25, + 5 or 2;
                       far, matrix cores 6: the header's 2^-21 = 8 units on the split-bf16 r^2 -> 4, + 2.
  powers               y^P from one y: P times the above + (P - 1) products.
  numerator            N roundings on the exact route (N_NUM: components of d, the products and sums of the dot products, the products with the
                       density and the normal, the scale).  On a far pair every numerator term is formed from x_t' and x_s' separately (moments
                       x_t' S0 - S_j; dot products x_t'.g - x_s'.g), each rounded relative to its own size: amplified by
                       AMP = (|x_t'| + |x_s'|) / r <= (rho + 1) / (rho - 1): 3 at rho = 2, 2 from rho = 3, 1.02 from rho = 100; two more roundings
                       (x_s' and x_t' themselves) and, on the matrix cores, 8 units for each contracted dot product join them.
  fold                 +3: k = 1 / f^2 (two roundings, halved by the square root: 1), k x_s' and k |x_s'|^2 (1 each on r2': 1 on 1 / r).
  last                 +1 for the accumulation factor of the device's mode.
FACTOR(zone) = W_device(zone) / W_yardstick.  fp64: the yardstick is the CPU oracle on the same pairs (W = 4.5 P + P - 1 + N); fp32: the exact
fp32 device kernel (SCTL_AMD_CENTERED=0; W = 4.5 P + P - 1 + N + 1).  Near-zone pairs get the exact kernel's W in either precision.  Lower
accuracy modes: the project's 10 * 10^-digits on |u_dev - u_true| / (|u_true| kappa), per pair."""
from collections import namedtuple

import numpy as np

import sctl_amd
from test_independent_math import _kernel_values

LD = np.longdouble
WAVE_TILE = 64        # centered_kernel.hpp: kWaveTile
MFMA_ROWS = 32        # centered_mfma_kernel.hpp: kMfmaRows
FAR_UNROLL = 4        # centered_kernel.hpp: UNR, the fold's groups of 4 as well
NEAR_FACTOR2 = 4.0    # centered_kernel.hpp: kNearFactor2
NT_A, NS_A = 128, 131
NT_B, NS_B = 513, 193
DEAD_NEAR = (10, 20, 74, 100)          # dead sources of Geometry A inside the near zone: the near list is never empty, 127 sources are far
INDEX_CYCLE = (1, 70, NS_A - 1, 33, NS_A - 3, 64, 127, 128)

POWERS = {"Laplace3D-FxU": 1, "Laplace3D-DxU": 3, "Laplace3D-FxdU": 3, "Stokes3D-FxU": 3, "Stokes3D-DxU": 5, "Stokes3D-FxT": 5, "Stokes3D-FSxU": 3,
          "Stokes3D-FxUP": 3, "Laplace3D-FDxUdU": 5}
# roundings of the numerator on the exact route, per output: components of d (1), dot products (3 products and sums + the component's 1 = 4), further
# products with d, the density or the normal (1 each), the sum of two terms (1), the scale (1)
N_NUM = {"Laplace3D-FxU": 2, "Laplace3D-DxU": 7, "Laplace3D-FxdU": 4, "Stokes3D-FxU": 9, "Stokes3D-FSxU": 10, "Stokes3D-FxUP": 9, "Stokes3D-DxU": 10,
         "Stokes3D-FxT": 8, "Laplace3D-FDxUdU": 12}
# forms whose far numerators hold a contracted dot product on the matrix cores (centered_mfma_kernel.hpp: NNUM >= 1)
MFMA_DOTS = {"Laplace3D-FxU": 0, "Laplace3D-DxU": 1, "Laplace3D-FxdU": 0, "Stokes3D-FxU": 1, "Stokes3D-FSxU": 1, "Stokes3D-FxUP": 1, "Stokes3D-DxU": 2,
             "Stokes3D-FxT": 1, "Laplace3D-FDxUdU": 2}
ZONES = ("near", "just_far", "mid", "very_far")
AMP = {"just_far": 3.0, "mid": 2.0, "very_far": 101.0 / 99.0}      # (rho + 1) / (rho - 1) at the zone's smallest rho: 2, 3, 100


def unit_of(dt):
    return LD(2.0) ** (-53 if np.dtype(dt) == np.float64 else -24)


def eps_of(dt):
    return 2.0 ** (-24 if np.dtype(dt) == np.float64 else -9)


def modes_of(name, dt):
    """(pipe, digits) every tile-centred form of (kernel, precision) serves; pipe "valu" for an fp32 form means SCTL_AMD_MFMA_F32=0"""
    if np.dtype(dt) == np.float64:
        return [("valu", -1), ("valu", 10), ("valu", 5)]
    if name in ("Laplace3D-FxU", "Laplace3D-DxU"):      # the packed vector-pipe kernel too: the default's mode, its bar at 5 digits, the Newton step
        return [("mfma", -1), ("valu", -1), ("valu", 5), ("valu", 10)]
    return [("mfma", -1)]


def full_precision(dt, digits):
    return digits < 0 or (np.dtype(dt) == np.float32 and digits > 7)      # fp32 at 10 digits: the most the precision gives, measured like -1


def w_yardstick(name, dt):
    P = POWERS[name]
    return 4.5 * P + (P - 1) + N_NUM[name] + (0 if np.dtype(dt) == np.float64 else 1)


def w_device(name, dt, pipe, zone):
    """worst case of a device pair in units (module docstring)"""
    P, N, f64 = POWERS[name], N_NUM[name], np.dtype(dt) == np.float64
    rsq = 5.0 if f64 else 2.0
    if zone == "near":
        return (2.5 + rsq) * P + (P - 1) + N + 1
    per = 4.0 + rsq if pipe == "mfma" else 7.25 + rsq
    dots = 8.0 * MFMA_DOTS[name] if pipe == "mfma" else 0.0
    fold = 3.0 if (name == "Laplace3D-FxU" and f64) else 0.0
    return per * P + (P - 1) + AMP[zone] * (N + 2 + dots) + fold + 1


def factor(name, dt, pipe, zone):
    return w_device(name, dt, pipe, zone) / w_yardstick(name, dt)


# ---- truth and measure ------------------------------------------------------------------------------------------------------------------
_PI = LD("3.14159265358979323846264338327950288")


def blocks(name, d, n, ctx=None):
    """U[pair][k0][k1] in long double, the scale factor included; d = x_t - x_s (P, 3), n (P, 3) or None"""
    if name == "Helmholtz3D-FxU":
        d = d.astype(LD)
        r = np.sqrt((d * d).sum(-1))
        amp = np.exp(-LD(ctx[1]) * r) / (4 * _PI * r)
        gr, gi = amp * np.cos(LD(ctx[0]) * r), amp * np.sin(LD(ctx[0]) * r)
        return np.stack([np.stack([gr, gi], axis=-1), np.stack([-gi, gr], axis=-1)], axis=-2)
    return _kernel_values(name, d, n, LD)


def abs_blocks(name, d, n):
    """the blocks with every factor replaced by its absolute value and every sum unsigned: what the roundings of a pair are relative to"""
    da, na = np.abs(d.astype(LD)), None if n is None else np.abs(n.astype(LD))
    U = np.abs(_kernel_values(name, da, na, LD))
    if name == "Laplace3D-FDxUdU":      # the one difference among the formulas: n_j / r^3 - 3 r_j (r.n) / r^5
        r2 = (da * da).sum(-1)
        ri = 1 / np.sqrt(r2)
        ri3 = ri * ri * ri
        U[:, 1, 1:] = (na * ri3[:, None] + 3 * da * ((da * na).sum(-1) * ri3 * ri * ri)[:, None]) / (4 * _PI)
    return U


def pair_values(name, xt, x, n, f, ctx=None):
    """(u_true (P, K1), u_abs (P, K1)) in long double of the targets xt (P, 3) against ONE source x (3,) with normal n (3,) or None and density f (K0,)"""
    d = xt.astype(LD) - x.astype(LD)[None, :]
    nn = None if n is None else np.tile(n.astype(LD), (d.shape[0], 1))
    fl = f.astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        U = blocks(name, d, nn, ctx)
        u = np.einsum("pjk,j->pk", U, fl)
        ua = u if name == "Helmholtz3D-FxU" else np.einsum("pjk,j->pk", abs_blocks(name, d, nn), np.abs(fl))
    hit = (d == 0).all(axis=1)
    u[hit] = 0
    ua = np.abs(ua)
    ua[hit] = 0
    return u, ua


def measure(got, u, ua, dt):
    """(q, e) per pair of the values got (P, K1) against the truth: module docstring.  A pair whose truth is exactly 0 must be exactly 0."""
    nu, na = np.sqrt((u * u).sum(-1)), np.sqrt((ua * ua).sum(-1))
    zero = nu == 0
    assert np.all(got[zero] == 0), "a coincident pair must contribute exactly 0: %r" % (got[zero][:4],)
    assert np.all(np.isfinite(got)), "non-finite values where the truth is finite"
    err = np.sqrt(((got.astype(LD) - u) ** 2).sum(-1))
    tiny = LD(np.finfo(np.dtype(dt)).tiny)
    q, e = np.zeros(nu.size), np.zeros(nu.size)
    ok = ~zero
    kappa = na[ok] / nu[ok]
    q[ok] = (err[ok] / (np.maximum(nu[ok], tiny) * unit_of(dt) * kappa)).astype(np.float64)
    e[ok] = (err[ok] / (nu[ok] * kappa)).astype(np.float64)
    return q, e


# ---- Geometry A: one wave -----------------------------------------------------------------------------------------------------------------
CLOUDS = ("cube", "offset", "flat")
RHO_NEAR = (0.3, 1.0, 1.5, "2-")
RHO_JUST_FAR = ("2+", 2.01, 2.1)
RHO_MID = (3.0, 10.0)
RHO_VERY_FAR = (1e2, 1e4, 1e8)
RHOS = RHO_NEAR + RHO_JUST_FAR + RHO_MID + RHO_VERY_FAR
T_REF = 77            # the target the coincident and the close probe sit at, and the one the parallel / orthogonal normals refer to

Probe = namedtuple("Probe", "x rho zone direction kind")      # kind: "rho", "coincident", "close"
Wave = namedtuple("Wave", "xt c rt2 c_ld rt2_ld probes dead")


def zone_of(rho):
    v = {"2-": 1.99, "2+": 2.001}.get(rho, rho)
    return "near" if v < 2 else "just_far" if v <= 2.1 else "mid" if v <= 10 else "very_far"


def rho_value(rho, dt):
    return LD(2) * (1 - LD(eps_of(dt))) if rho == "2-" else LD(2) * (1 + LD(eps_of(dt))) if rho == "2+" else LD(rho)


def targets(kind, dt, n=NT_A, seed=1):
    """the three target clouds; fp32: a cube of side 0.1 (r^-5 of every probed distance, 1e-5 Rt .. 1e8 Rt, stays a normal fp32) and an offset of 8,
    which the fp32 grid resolves to 1e-5 Rt; fp64: the unit cube, and 1e4 + 1e-2 cube"""
    rng = np.random.default_rng([seed, CLOUDS.index(kind)])
    f64 = np.dtype(dt) == np.float64
    x = rng.random((n, 3))
    if kind == "flat":
        x[:, 2] = 0.37
    x *= 1.0 if f64 else 0.1
    if kind == "offset":
        x = (1.0e4 + 1e-2 * x) if f64 else (8.0 + x)
    return np.ascontiguousarray(x.astype(dt))


def centre_and_radius(xt):
    """(c, Rt^2) as the kernel computes them, in xt's precision, and (c widened, Rt^2) in long double about the SAME centre"""
    dt = xt.dtype.type
    c = dt(0.5) * xt.min(axis=0) + dt(0.5) * xt.max(axis=0)
    p = xt - c[None, :]
    rt2 = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).max()
    pl = xt.astype(LD) - c.astype(LD)[None, :]
    return c, rt2, c.astype(LD), (pl * pl).sum(-1).max()


def ss_of(x, c):
    """|x - c|^2 in the precision of x and c (the kernel's len2 of p = x - c)"""
    p = x - c
    return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]


def directions(rng):
    v = rng.normal(size=3)
    return {"axis": np.array([1.0, 0.0, 0.0]), "diagonal": np.ones(3) / np.sqrt(3.0), "random": v / np.linalg.norm(v)}


def close_distance(dt):
    """of the close probe, in units of Rt: 1e-8 in fp64; 1e-5 in fp32, where r^-5 of 1e-8 Rt overflows"""
    return 1e-8 if np.dtype(dt) == np.float64 else 1e-5


def _place(c_ld, rt_ld, rho, u, dt):
    return (c_ld + rho * rt_ld * u.astype(LD)).astype(dt)


def wave(kind, dt, seed=1):
    """Geometry A for one cloud: targets, centre, radius and the probes — every rho in the three directions, the coincident and the close probe —
    and NS_A dead positions: far (rho in 2.5 .. 6) but for the four of DEAD_NEAR"""
    xt = targets(kind, dt, NT_A, seed)
    c, rt2, c_ld, rt2_ld = centre_and_radius(xt)
    rt = np.sqrt(rt2_ld)
    rng = np.random.default_rng([seed, 7, CLOUDS.index(kind)])
    dirs = directions(rng)
    probes = [Probe(_place(c_ld, rt, rho_value(rho, dt), u, dt), rho, zone_of(rho), dn, "rho") for rho in RHOS for dn, u in dirs.items()]
    probes.append(Probe(xt[T_REF].copy(), None, "near", None, "coincident"))
    v = rng.normal(size=3)
    x = (xt[T_REF].astype(LD) + LD(close_distance(dt)) * rt * (v / np.linalg.norm(v)).astype(LD)).astype(dt)
    if np.array_equal(x, xt[T_REF]):       # the grid is coarser than the distance (the fp32 offset cloud): the next number
        x[0] = np.nextafter(x[0], dt(np.inf))
    probes.append(Probe(x, None, "near", None, "close"))
    dead = dead_sources(c_ld, rt, NS_A, dt, rng)
    return Wave(xt, c, rt2, c_ld, rt2_ld, probes, dead)


def dead_sources(c_ld, rt, n, dt, rng, near=DEAD_NEAR):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    rho = rng.uniform(2.5, 6.0, n)
    rho[list(near)] = rng.uniform(0.2, 1.5, len(near))
    return np.ascontiguousarray((c_ld[None, :] + (LD(1) * rho[:, None]) * rt * v.astype(LD)).astype(dt))


def is_far(x, w):
    """the kernel's decision restated in the form's precision"""
    return ss_of(x, w.c) > x.dtype.type(NEAR_FACTOR2) * w.rt2


def is_far_ld(x, w):
    p = x.astype(LD) - w.c_ld
    return (p * p).sum() > LD(NEAR_FACTOR2) * w.rt2_ld


# ---- densities and normals ------------------------------------------------------------------------------------------------------------------
SCALARS = (1.0, -1.0, 3e-7, -2.5e9)


def density_cycle(k0, dt):
    """K0 = 1: +-1, 3e-7, -2.5e9; K0 > 1: each unit vector (times one of those) in turn, then a generic vector times each of them"""
    if k0 == 1:
        return [np.array([s], dtype=dt) for s in SCALARS]
    g = np.array([0.6, -0.35, 0.8, 0.45][:k0])
    return [(np.eye(k0)[k] * SCALARS[k % 4]).astype(dt) for k in range(k0)] + [(g * s).astype(dt) for s in SCALARS]


def normal_for(which, xt_ref, x, dt):
    """generic, parallel or orthogonal to x_t - x_s for the reference target"""
    d = (xt_ref.astype(LD) - x.astype(LD)).astype(np.float64)
    if which == 0 or not np.any(d):
        return np.array([0.31, -0.52, 0.44], dtype=dt)
    d /= np.linalg.norm(d)
    if which == 1:
        return (0.7 * d).astype(dt)
    o = np.cross(d, np.array([0.2, 0.9, -0.4]))
    return (0.7 * o / np.linalg.norm(o)).astype(dt)


def fold_band_densities(x, w):
    """Laplace3D-FxU fp64: densities at the edges of the fold's band k |x_s'|^2 in [2^-600, 2^600] for this wave's centre (k = 1 / f^2, so
    |f| = 2^-+300 |x_s'| sits on an edge) and four fixed ones.  (label, f, route the header predicts): "fold", or "exact" for a record out of the
    band (all of these have k within [2^-900, 2^900]: none goes to the pre-pass's exception list; the decision is the wave's)."""
    s = float(np.sqrt(ss_of(x, w.c)))
    out = []
    for label, base, inside in (("low edge", 2.0 ** -300 * s, +1), ("high edge", 2.0 ** 300 * s, -1)):
        for side in (+1, -1):
            f = base * (1 + side * 2.0 ** -10)
            out.append(("%s %s" % (label, "inside" if side == inside else "outside"), f if side > 0 else -f, "fold" if side == inside else "exact"))
    for f in (1e-100, -1e-130, -1e100, 1e130):
        out.append(("|f| = %g" % abs(f), f, fold_route(f, x, w)))
    return out


def fold_route(f, x, w):
    """the route centered_kernel.hpp's stage_rec takes for a far source x of density f: its tests restated in fp64"""
    k = 1.0 / (f * f)
    ss = ss_of(x, w.c)
    kss = k * ss
    return "fold" if (2.0 ** -600 <= kss <= 2.0 ** 600 and 2.0 ** -300 <= ss <= 2.0 ** 300) else "exact"


# ---- launches -------------------------------------------------------------------------------------------------------------------------------
Launch = namedtuple("Launch", "geometry cloud xt xs xn f live probe zone label route")


def _sources(dead, probe, idx, info, f, nrm, dt):
    xs = dead.copy()
    xs[idx] = probe.x
    ns = xs.shape[0]
    F = np.zeros((ns, info["k0"]), dtype=dt)
    F[idx] = f
    xn = None
    if info["nd"]:
        xn = np.tile(np.array([0.3, 0.5, -0.2], dtype=dt), (ns, 1))
        xn[idx] = nrm
    return xs, xn, F


def _limit_range(f, probe, dt):
    """fp32: the 1e8 Rt and the close probe take densities of size 1 (r^-5 times 3e-7, or r^-5 itself at 1e-8 Rt, would leave the normal fp32 range
    in the exact kernel as in any other)"""
    if np.dtype(dt) == np.float32 and (probe.kind == "close" or probe.rho == 1e8):
        m = np.abs(f).max()
        return (f / m).astype(dt)
    return f


def launches_a(name, dt, waves):
    """Geometry A: the cube cloud with every probe (38), the offset and the flat cloud with every rho in rotating directions and the two special
    probes (14 each); the live index, the density and the normal rotate.  Laplace3D-FxU fp64 adds the band densities at a rho = 3 probe (8) and, with
    dead densities of +-2^-200 that fill the fold's lists without reaching the last bit of the sum (2^-140 of the live term), 8 far probes whose
    record then sits in a full group of 4 or in a later tile's leftovers."""
    info = sctl_amd.kernel_info(name)
    dens = density_cycle(info["k0"], dt)
    out, i = [], 0
    for cloud in CLOUDS:
        w = waves[cloud]
        rho_probes = [p for p in w.probes if p.kind == "rho"]
        if cloud == "cube":
            chosen = list(w.probes)
        else:
            names = ("axis", "diagonal", "random")
            chosen = [p for j, rho in enumerate(RHOS) for p in rho_probes if p.rho == rho and p.direction == names[(j + CLOUDS.index(cloud)) % 3]]
            chosen += [p for p in w.probes if p.kind != "rho"]
        for p in chosen:
            idx = INDEX_CYCLE[i % len(INDEX_CYCLE)]
            f = _limit_range(dens[i % len(dens)], p, dt)
            nrm = normal_for(i % 3, w.xt[T_REF], p.x, dt)
            xs, xn, F = _sources(w.dead, p, idx, info, f, nrm, dt)
            out.append(Launch("A", cloud, w.xt, xs, xn, F, idx, p, p.zone, "%s %s %s" % (cloud, p.kind if p.kind != "rho" else "rho=%s" % p.rho, p.direction), None))
            i += 1
    if name == "Laplace3D-FxU" and np.dtype(dt) == np.float64:
        w = waves["cube"]
        p = [q for q in w.probes if q.rho == 3.0 and q.direction == "random"][0]
        for j, (label, f, route) in enumerate(fold_band_densities(p.x, w)):
            idx = INDEX_CYCLE[j % len(INDEX_CYCLE)]
            xs, xn, F = _sources(w.dead, p, idx, info, np.array([f]), None, dt)
            out.append(Launch("A", "cube", w.xt, xs, xn, F, idx, p, p.zone, "band %s" % label, route))
        far = [q for q in w.probes if q.kind == "rho" and q.zone != "near" and q.direction == "diagonal"]
        for j, p in enumerate(far):
            idx = INDEX_CYCLE[j % len(INDEX_CYCLE)]
            xs, xn, F = _sources(w.dead, p, idx, info, np.array([SCALARS[j % 2]]), None, dt)
            fill = 2.0 ** -200 * np.where(np.arange(NS_A) % 3 == 0, -1.0, 1.0)
            fill[idx] = F[idx, 0]
            out.append(Launch("A", "cube", w.xt, xs, xn, fill.reshape(-1, 1).astype(dt), idx, p, p.zone, "filled rho=%s" % p.rho, "fold"))
    return out


def far_slot(xs, live, w, pipe, f64, F=None):
    """(tile, "group" | "leftover") of a live far source among the far records of its launch: fp64 consumes the far list 4 at a time and carries
    the rest (the last n % 4 records of the launch are the leftovers), the fp32 vector-pipe kernel pads each tile (the last n_tile % 4 of the
    live source's tile), the matrix-core kernels consume 32 rows at a time and carry.  F: the densities when the form folds them (records of the
    live source's sign only, zeros dropped)."""
    far = np.array([bool(is_far(x, w)) for x in xs])
    assert far[live]
    if F is not None:
        far &= (np.sign(F[:, 0]) == np.sign(F[live, 0]))
    tile = live // WAVE_TILE
    if F is not None:
        tile = int(far[:live].sum()) // WAVE_TILE          # (the pre-pass groups by sign: the tile is the rank's)
    if pipe == "valu" and not f64:
        sel = far[tile * WAVE_TILE:(tile + 1) * WAVE_TILE]
        rank, n = int(sel[:live - tile * WAVE_TILE].sum()), int(sel.sum())
    else:
        rank, n = int(far[:live].sum()), int(far.sum())
    g = MFMA_ROWS if pipe == "mfma" else FAR_UNROLL
    return tile, "leftover" if rank >= n - n % g else "group"


# ---- Geometry B: several waves ----------------------------------------------------------------------------------------------------------------
def launches_b(name, dt, seed=2):
    """513 clustered targets (five waves of 128, three of 192 or 256, each with a centre of its own that this module does not know), 193 sources;
    every rho about the cloud's own midpoint and radius in rotating directions, and a copy of a target"""
    info = sctl_amd.kernel_info(name)
    rng = np.random.default_rng([seed, 11])
    f64 = np.dtype(dt) == np.float64
    centres = rng.random((4, 3))
    xt = (centres[rng.integers(0, 4, NT_B)] + 0.03 * rng.normal(size=(NT_B, 3))) * (1.0 if f64 else 0.1)
    xt = np.ascontiguousarray(xt.astype(dt))
    c, rt2, c_ld, rt2_ld = centre_and_radius(xt)
    rt = np.sqrt(rt2_ld)
    dirs = directions(rng)
    names = ("axis", "diagonal", "random")
    dead = dead_sources(c_ld, rt, NS_B, dt, rng, near=(5, 50, 66, 130, 190))
    dens = density_cycle(info["k0"], dt)
    out = []
    for j, rho in enumerate(RHOS + (None,)):
        if rho is None:
            p = Probe(xt[T_REF].copy(), None, "any", None, "coincident")
        else:
            p = Probe(_place(c_ld, rt, rho_value(rho, dt), dirs[names[j % 3]], dt), rho, "any", names[j % 3], "rho")
        idx = (3, 64 + 31, NS_B - 1, 128 + 5, 190)[j % 5]
        f = _limit_range(dens[j % len(dens)], p, dt)
        xs, xn, F = _sources(dead, p, idx, info, f, normal_for(j % 3, xt[T_REF], p.x, dt), dt)
        out.append(Launch("B", "clusters", xt, xs, xn, F, idx, p, "any", "B %s" % (p.kind if rho is None else "rho=%s" % rho), None))
    return out


_WAVES = {}


def waves_for(dt):
    key = np.dtype(dt).name
    if key not in _WAVES:
        _WAVES[key] = {kind: wave(kind, dt) for kind in CLOUDS}
    return _WAVES[key]
