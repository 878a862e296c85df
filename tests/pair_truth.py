"""Truth, measure and probe geometry of the per-pair tests of the derivative kernels (tests/test_pair_truth_cpu.py, tests/test_gpu_derivative_pairs.py).

Truth.  For ONE pair the K0 x K1 block U(d, n) of each of the ten kernels and its derivative tensors
    DU[k0, k1, j] = dU / dd_j,    NU[k0, k1, j] = dU / dn_j,    d = x_trg - x_src, n the source normal, j = 0..2,
in np.longdouble (64-bit significand, asserted on import).  Nothing is derived by hand: the ten blocks are written once as sympy expressions of
d0..d2, n0..n2, the distance R, its reciprocal Y and, for Helmholtz, the wavenumber kr + i ki, and sympy differentiates them; the only rule supplied is
dR/dd_j = d_j Y, dY/dd_j = -Y^3 d_j.  The expressions are lambdified with the numpy module, so one function per kernel runs vectorised on arrays of any
float type.  Three traps, each asserted: 1/(4 pi), 1/(8 pi) and 3/(4 pi) are not in the expressions (a printed numpy.pi is a double) but applied
afterwards in the arrays' own type from a long-double pi; the only constants in the expressions are integers and dyadic rationals; every array
returned has the type of the arrays passed in.  A coincident pair (r = 0) is 0 in every tensor, as everywhere in this library.

Everything the device returns is a contraction of these tensors over one pair (sctl_amd/csrc/jvp_kernel.hpp, include/sctl_amd/device/eval_grad_kernel.hpp):
    tangent   du[k1]   = sum_k0 f[k0] sum_j (DU[k0,k1,j] e[j] + NU[k0,k1,j] m[j]),      e = dx_trg - dx_src, m = dn_src
    gradient  g_trg[j] = sum_{k0,k1} w[k1] f[k0] DU[k0,k1,j],   g_src = -g_trg,   g_nrm[j] = sum_{k0,k1} w[k1] f[k0] NU[k0,k1,j]
d and e are the differences AS THE KERNEL FORMS THEM, in the working precision: both sides of eval_grad_kernel form d = x_trg - x_src per component
from the owner's registers and the streamed record (SIDE 0: xo - rec, SIDE 1: rec - xo), eval_jvp_kernel forms d = xo - rec and e = eo - rec[3..5]
the same way, one rounding each.  The probe geometry below is built so that every one of these subtractions is exact, and checks it.

Yardstick.  The same lambdified functions called on np.float64 / np.float32 arrays are the plain formula in that precision, with R = sqrt(r2) and
Y = 1 / R correctly rounded and the integer powers by numpy's power; the contraction and the scale factor are then done in that precision too.

Measure.  Per pair and per homogeneous output group (g_trg, g_src, g_nrm, the tangent's K1 values, split where their degree in r differs),
    q = max_j |dev_j - true_j| / (eps_R a),      eps_R = 2^-53 or 2^-24,
where a is the largest component over the group of the MAJORANT: the same contraction with absolute values on every factor,
sum |f| (|DU| |e| + |NU| |m|) or sum |w| |f| |DU|.  A tangent or a normal that happens to be orthogonal to d cannot blow the measure up, so no probe is
ever left out.  Helmholtz divides further by 1 + (|Re k| + |Im k|) r: the amplification of a few-ulp error in r by dG/dr = (ik - 1/r) G
(tests/test_gpu_helmholtz_pairs.py).

Probe geometry.  Owners sit at p + r u around the live point p, r log-spaced over 2^-40 .. 2^10 (fp64) or 2^-14 .. 2^10 (fp32: the highest power of
1/r any form takes is y^7 = 2^98, inside the fp32 range), Helmholtz r <= 8; one owner coincides with p.  Zones: r < 2^-8, 2^-8 <= r < 2, r >= 2."""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit significand here: it cannot serve as the truth"

PI = 4 * np.arctan(LD(1))
EPS = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}

# name: (K0, K1, has a normal, (numerator, multiple of pi in the denominator) of the scale factor)
KERNELS = {
    "Laplace3D-FxU": (1, 1, False, (1, 4)), "Laplace3D-DxU": (1, 1, True, (1, 4)), "Laplace3D-FxdU": (1, 3, False, (1, 4)),
    "Stokes3D-FxU": (3, 3, False, (1, 8)), "Stokes3D-DxU": (3, 3, True, (3, 4)), "Stokes3D-FxT": (3, 9, False, (3, 4)),
    "Stokes3D-FSxU": (4, 3, False, (1, 8)), "Stokes3D-FxUP": (3, 4, False, (1, 8)), "Laplace3D-FDxUdU": (2, 4, True, (1, 4)),
    "Helmholtz3D-FxU": (2, 2, False, (1, 4)),
}
# the tangent's K1 values by degree in r: u against grad u, velocity against pressure
TANGENT_GROUPS = {"Laplace3D-FDxUdU": ([0], [1, 2, 3]), "Stokes3D-FxUP": ([0, 1, 2], [3])}
ZONE_EDGES = (2.0 ** -8, 2.0)
ZONE_NAMES = ("r < 2^-8", "2^-8 <= r < 2", "r >= 2")


def scale_of(name, dtype):
    """the kernel's scale factor, formed in long double and rounded once to `dtype`"""
    num, den = KERNELS[name][3]
    return np.dtype(dtype).type(LD(num) / (LD(den) * PI))


# ---- the blocks, symbolically ------------------------------------------------------------------------------------------------------------
def _blocks(name):
    """(sympy Matrix K0 x K1 without the scale factor, symbols): the formulas of tests/grad_truth.py, with R = r and Y = 1 / r as symbols of their own"""
    import sympy as sp
    d = sp.symbols("d0:3", real=True)
    n = sp.symbols("n0:3", real=True)
    R, Y = sp.symbols("R Y", positive=True)
    kr, ki = sp.symbols("kr ki", real=True)
    dn = sum(a * b for a, b in zip(d, n))
    eye = lambda i, k: 1 if i == k else 0
    stokeslet = [[eye(i, k) * Y + d[i] * d[k] * Y ** 3 for k in range(3)] for i in range(3)]
    if name == "Laplace3D-FxU":
        U = [[Y]]
    elif name == "Laplace3D-DxU":
        U = [[dn * Y ** 3]]
    elif name == "Laplace3D-FxdU":
        U = [[-d[k] * Y ** 3 for k in range(3)]]
    elif name == "Stokes3D-FxU":
        U = stokeslet
    elif name == "Stokes3D-DxU":
        U = [[d[i] * d[k] * dn * Y ** 5 for k in range(3)] for i in range(3)]
    elif name == "Stokes3D-FxT":
        U = [[-d[i] * d[j] * d[k] * Y ** 5 for j in range(3) for k in range(3)] for i in range(3)]
    elif name == "Stokes3D-FSxU":
        U = stokeslet + [[d[k] * Y ** 3 for k in range(3)]]
    elif name == "Stokes3D-FxUP":
        U = [stokeslet[i] + [d[i] * Y ** 3] for i in range(3)]
    elif name == "Laplace3D-FDxUdU":
        U = [[Y] + [-d[k] * Y ** 3 for k in range(3)], [dn * Y ** 3] + [n[k] * Y ** 3 - 3 * d[k] * dn * Y ** 5 for k in range(3)]]
    elif name == "Helmholtz3D-FxU":
        gr, gi = Y * sp.exp(-ki * R) * sp.cos(kr * R), Y * sp.exp(-ki * R) * sp.sin(kr * R)
        U = [[gr, gi], [-gi, gr]]
    else:
        raise ValueError(name)
    return sp.Matrix(U), dict(d=d, n=n, R=R, Y=Y, kr=kr, ki=ki)


def _dyadic_only(expr):
    """the only numbers in the expression are integers and rationals with a power of two below: what every float type holds exactly"""
    import sympy as sp
    for a in expr.atoms(sp.Number):
        assert a.is_Rational and (a.q & (a.q - 1)) == 0, "a constant that is not dyadic: %r" % (a,)
    assert not expr.has(sp.pi) and not expr.atoms(sp.Float)


@functools.lru_cache(maxsize=None)
def symbolic(name):
    """(U, DU, NU, symbols): U[k0][k1], DU[k0][k1][j], NU[k0][k1][j] as sympy expressions without the scale factor; NU is None without a normal.  `c`
    multiplies the radial part of DU (1 for the truth; the planted coefficient fault of the CPU tests sets it off 1)."""
    import sympy as sp
    U, s = _blocks(name)
    K0, K1, has_n, _ = KERNELS[name]
    assert U.shape == (K0, K1)
    c = sp.Symbol("c", positive=True)
    d, n, R, Y = s["d"], s["n"], s["R"], s["Y"]
    DU = [[[sp.diff(U[a, b], d[j]) + c * (sp.diff(U[a, b], R) * d[j] * Y - sp.diff(U[a, b], Y) * Y ** 3 * d[j]) for j in range(3)]
           for b in range(K1)] for a in range(K0)]
    NU = [[[sp.diff(U[a, b], n[j]) for j in range(3)] for b in range(K1)] for a in range(K0)] if has_n else None
    for e in list(U) + [x for row in DU for col in row for x in col] + ([x for row in NU for col in row for x in col] if NU else []):
        _dyadic_only(e)
    s = dict(s, c=c)
    return U, DU, NU, s


def _args(s):
    return list(s["d"]) + list(s["n"]) + [s["R"], s["Y"], s["kr"], s["ki"], s["c"]]


@functools.lru_cache(maxsize=None)
def _lambdified(name):
    import sympy as sp
    U, DU, NU, s = symbolic(name)
    flat = list(U) + [x for row in DU for col in row for x in col] + ([x for row in NU for col in row for x in col] if NU else [])
    return sp.lambdify(_args(s), flat, modules="numpy", cse=True)


def tensors(name, d, n=None, k=None, root_error=0.0, c=1.0):
    """(U, DU, NU, r) for the pairs d (N, 3), n (N, 3) or None, in d's own type and WITHOUT the scale factor: shapes (N, K0, K1), (N, K0, K1, 3),
    (N, K0, K1, 3) or None, (N,).  k = (Re k, Im k) for Helmholtz.  A coincident pair is 0 throughout.  root_error and c plant the faults of the CPU
    tests: R and Y off by that relative error, the radial coefficient off 1."""
    K0, K1, has_n, _ = KERNELS[name]
    dt = d.dtype
    T = dt.type
    N = d.shape[0]
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    r2 = d0 * d0 + d1 * d1 + d2 * d2
    hit = r2 == 0
    R = np.sqrt(np.where(hit, T(1), r2))
    Y = T(1) / R
    if root_error:
        R, Y = R * T(1 + root_error), Y * T(1 - root_error)
    nn = n if has_n else np.zeros((N, 3), dtype=dt)
    kr, ki = (T(0), T(0)) if k is None else (T(LD(k[0])), T(LD(k[1])))
    assert nn.dtype == dt and r2.dtype == dt and R.dtype == dt and Y.dtype == dt
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        out = _lambdified(name)(d0, d1, d2, nn[:, 0], nn[:, 1], nn[:, 2], R, Y, kr, ki, T(c))
    arr = []
    for o in out:
        if isinstance(o, np.ndarray) and o.shape == (N,):
            assert o.dtype == dt, "an expression left the working type: %s" % o.dtype
            arr.append(np.where(hit, T(0), o))
        else:                                   # a constant entry (0 or an integer): exact in every type
            assert float(o) == int(o)
            arr.append(np.where(hit, T(0), np.full(N, T(int(o)))))
    nU, nD = K0 * K1, K0 * K1 * 3
    U = np.stack(arr[:nU], axis=1).reshape(N, K0, K1)
    DU = np.stack(arr[nU:nU + nD], axis=1).reshape(N, K0, K1, 3)
    NU = np.stack(arr[nU + nD:], axis=1).reshape(N, K0, K1, 3) if has_n else None
    for a in (U, DU, NU):
        assert a is None or a.dtype == dt
    return U, DU, NU, np.where(hit, T(0), R)


def pair_values(name, d, n, e, m, f, w, k=None, **fault):
    """The per-pair values and their majorants in d's own type, scale factor included: dict with du (N, K1), g_trg (N, 3), g_nrm (N, 3) or None, the
    majorants maj_du, maj_g, maj_n of the same shapes, and r (N,).  d, e (N, 3); n, m (N, 3) or None; f (N, K0); w (N, K1); any of e, w may be None."""
    dt = d.dtype
    U, DU, NU, r = tensors(name, d, n, k, **fault)
    S = scale_of(name, dt)
    out = dict(r=r, du=None, maj_du=None, g_trg=None, maj_g=None, g_nrm=None, maj_n=None)
    ab = np.abs
    for a in (n, e, m, f, w):
        assert a is None or a.dtype == dt
    if e is not None:
        du = np.einsum("pa,pabj,pj->pb", f, DU, e)
        maj = np.einsum("pa,pabj,pj->pb", ab(f), ab(DU), ab(e))
        if NU is not None:
            du = du + np.einsum("pa,pabj,pj->pb", f, NU, m)
            maj = maj + np.einsum("pa,pabj,pj->pb", ab(f), ab(NU), ab(m))
        out["du"], out["maj_du"] = du * S, maj * S
    if w is not None:
        out["g_trg"], out["maj_g"] = np.einsum("pb,pa,pabj->pj", w, f, DU) * S, np.einsum("pb,pa,pabj->pj", ab(w), ab(f), ab(DU)) * S
        if NU is not None:
            out["g_nrm"], out["maj_n"] = np.einsum("pb,pa,pabj->pj", w, f, NU) * S, np.einsum("pb,pa,pabj->pj", ab(w), ab(f), ab(NU)) * S
    for v in out.values():
        assert v is None or v.dtype == dt
    return out


def to_ld(*arrays):
    return tuple(None if a is None else np.asarray(a).astype(LD) for a in arrays)


# ---- measure -----------------------------------------------------------------------------------------------------------------------------
def tangent_groups(name):
    return TANGENT_GROUPS.get(name, (list(range(KERNELS[name][1])),))


def q_of(got, true, maj, eps, groups=None, amp=None):
    """q per pair (N,), float64: the largest over the groups of max_j |got_j - true_j| / (eps a), a the group's largest majorant component (and, for
    Helmholtz, amp = 1 + (|Re k| + |Im k|) r).  true and maj are long double.  A pair whose majorant is 0 (the coincident one) has q = 0 when got is
    exactly 0 and inf otherwise; a non-finite got gives inf."""
    assert true.dtype == LD and maj.dtype == LD
    N = true.shape[0]
    groups = groups or (list(range(true.shape[1])),)
    q = np.zeros(N)
    g = np.asarray(got).astype(LD)
    for cols in groups:
        err = np.abs(g[:, cols] - true[:, cols]).max(axis=1)
        a = maj[:, cols].max(axis=1) * LD(eps)
        if amp is not None:
            a = a * amp
        with np.errstate(divide="ignore", invalid="ignore"):
            qq = np.where(a > 0, err / np.where(a > 0, a, 1), np.where(err == 0, 0, np.inf)).astype(np.float64)
        qq[~np.isfinite(np.asarray(got, dtype=np.float64)[:, cols]).all(axis=1)] = np.inf
        q = np.maximum(q, qq)
    return q


def helmholtz_amp(k, r):
    return 1 + LD(abs(k[0]) + abs(k[1])) * r.astype(LD)


def zones_of(r):
    """zone index per pair from the nominal distance: 0, 1, 2 as ZONE_NAMES; -1 for the coincident pair"""
    z = np.digitize(r, ZONE_EDGES)
    return np.where(r == 0, -1, z)


# ---- probe geometry ----------------------------------------------------------------------------------------------------------------------
# the live point: on the 2^-10 lattice, so that a coordinate up to 2^10 away still differs from it by an fp32 number
P = np.array([326.0, 278.0, 145.0]) / 1024.0
LIVE_SLOTS = lambda n: (0, 255, 256, n - 1)        # first and last lane of a tile, the first of the next tile, the ragged last tile
N_OWNERS, N_STREAMED = 300, 600                    # a full workgroup and a ragged one; tiles of 256, 256 and 88


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def lattice(rng, shape, lo=-0.5, hi=0.5):
    """nonzero multiples of 2^-10 in [lo, hi]: exact in fp32 and fp64, and so are their differences"""
    v = rng.integers(int(lo * 1024), int(hi * 1024) + 1, size=shape)
    v = np.where(v == 0, 1, v)
    return v / 1024.0


def snap_exact(x, dt):
    """x (N, 3), float64, moved to the nearest points for which x - P is exact in dt, per coordinate: with M = 2^(floor(log2 max(|x|, |P|)) + 2) both
    numbers and their difference lie below M, so all three are numbers of dt once x and P are multiples of M 2^-t (t = 24 or 53 bits); P's lattice
    (2^-10) is finer than that grid up to |x| < 2^11 in fp32"""
    t = 24 if np.dtype(dt) == np.float32 else 53
    big = np.maximum(np.abs(x), np.abs(P)[None, :])
    g = 2.0 ** (np.floor(np.log2(big)) + 2 - t)
    return (np.round(x / g) * g).astype(dt)


def owner_distances(dt, n, rng, helmholtz=False):
    """n - 1 nominal distances, log-spaced, a third per zone, in random order, and one 0 (the coincident owner) at a random place"""
    lo = -14.0 if np.dtype(dt) == np.float32 else -40.0
    hi = 3.0 if helmholtz else 10.0
    m = n - 1
    cnt = (m // 3, m // 3, m - 2 * (m // 3))
    ex = np.concatenate([np.linspace(lo, -8.0, cnt[0], endpoint=False), np.linspace(-8.0, 1.0, cnt[1], endpoint=False), np.linspace(1.0, hi, cnt[2])])
    r = np.concatenate([2.0 ** ex, [0.0]])
    return r[rng.permutation(n)]


def owners(dt, n, seed, helmholtz=False):
    """(x (n, 3) in dt, r (n,) the distance |x - P| as a double, exact to its rounding): owners at P + r u, coordinates snapped so that x - P is exact in dt"""
    rng = np.random.default_rng(seed)
    r = owner_distances(dt, n, rng, helmholtz)
    x = snap_exact(P[None, :] + r[:, None] * _unit(rng, n), dt)
    x[r == 0] = P.astype(dt)
    d = x.astype(LD) - P.astype(LD)[None, :]
    rr = np.sqrt((d * d).sum(axis=1)).astype(np.float64)
    assert np.all((rr == 0) == (r == 0))
    return x, rr


def differences_exact(a, b):
    """a - b formed in the arrays' own type equals the long-double difference, everywhere"""
    assert a.dtype == b.dtype
    return bool(np.all((a - b).astype(LD) == a.astype(LD) - b.astype(LD)))


def launch(name, dt, side, slot, seed, n_owners=N_OWNERS, n_streamed=N_STREAMED, k=None):
    """One probe launch.  side "trg": the targets own the sums (n_owners targets around P, n_streamed sources of which the one at `slot` is live and
    sits at P: its density is the only nonzero one); side "src": the sources own them (n_owners sources around P, all densities live; of the
    n_streamed targets the one at `slot` sits at P and carries the only nonzero weight).  Dead points fill the unit box with nonzero tangents and
    normals.  Returns a dict of flat arrays in dt as the library takes them (xt, xs, xn, f, w, dxt, dxs, dxn), the per-pair inputs of the probed pairs
    (d, e, n, m, f_pair, w_pair, each (n_owners, .)), r, and `live`."""
    K0, K1, has_n, _ = KERNELS[name]
    rng = np.random.default_rng(seed)
    xo, r = owners(dt, n_owners, seed + 1, helmholtz=name.startswith("Helmholtz"))
    xst = (rng.integers(0, 2 ** 20, size=(n_streamed, 3)) / 2.0 ** 20).astype(dt)
    xst[slot] = P.astype(dt)
    L = lambda *shape: lattice(rng, shape).astype(dt)
    live = np.zeros(n_streamed, dtype=bool)
    live[slot] = True
    if side == "trg":
        xt, xs, Nt, Ns = xo, xst, n_owners, n_streamed
        f = np.where(live[:, None], L(Ns, K0), dt(0.0))                  # +0.0 everywhere but the live source
        w = L(Nt, K1)
    else:
        xt, xs, Nt, Ns = xst, xo, n_streamed, n_owners
        f = L(Ns, K0)
        w = np.where(live[:, None], L(Nt, K1), dt(0.0))
    xn = L(Ns, 3) if has_n else None
    dxt, dxs, dxn = L(Nt, 3), L(Ns, 3), (L(Ns, 3) if has_n else None)
    B = lambda a, n: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (n,) + a.shape[1:]))
    if side == "trg":                # pair t: (target t, the live source)
        pair = dict(d=xt - xs[slot][None, :], e=dxt - dxs[slot][None, :], n=B(None if xn is None else xn[slot][None, :], Nt),
                    m=B(None if dxn is None else dxn[slot][None, :], Nt), f_pair=B(f[slot][None, :], Nt), w_pair=w)
        exact = differences_exact(xt, B(xs[slot][None, :], Nt)) and differences_exact(dxt, B(dxs[slot][None, :], Nt))
    else:                            # pair s: (the live target, source s)
        pair = dict(d=xt[slot][None, :] - xs, e=dxt[slot][None, :] - dxs, n=xn, m=dxn, f_pair=f, w_pair=B(w[slot][None, :], Ns))
        exact = differences_exact(B(xt[slot][None, :], Ns), xs) and differences_exact(B(dxt[slot][None, :], Ns), dxs)
    flat = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dt).ravel()
    out = dict(xt=flat(xt), xs=flat(xs), xn=flat(xn), f=flat(f), w=flat(w), dxt=flat(dxt), dxs=flat(dxs), dxn=flat(dxn),
               r=r, live=slot, side=side, exact=exact, Nt=Nt, Ns=Ns, k=k)
    out.update(pair)
    assert all(v.dtype == dt for v in pair.values() if v is not None)
    return out


def truth_and_yardstick(name, c):
    """(truth, yard): pair_values in long double on the launch's exactly formed per-pair inputs, and the same formula in the launch's own type"""
    args = (c["d"], c["n"], c["e"], c["m"], c["f_pair"], c["w_pair"])
    return pair_values(name, *to_ld(*args), k=c["k"]), pair_values(name, *args, k=c["k"])


def mp_pair_values(name, d, n, e, m, f, w, k=None, dps=40):
    """pair_values for ONE pair, the same sympy expressions evaluated in mpmath at `dps` digits: (du, g_trg, g_nrm) as lists of mpf, scale included.  The
    inputs are long doubles and enter exactly."""
    import mpmath
    import sympy as sp
    K0, K1, has_n, (num, den) = KERNELS[name]
    U, DU, NU, s = symbolic(name)
    with mpmath.workdps(dps):
        mp = lambda x: mpmath.mpf(float(x)) + mpmath.mpf(float(LD(x) - LD(float(x))))           # a long double is the exact sum of two doubles
        dv, nv = [mp(x) for x in d], ([mp(x) for x in n] if has_n else [mpmath.mpf(0)] * 3)
        R = mpmath.sqrt(sum(x * x for x in dv))
        vals = dv + nv + [R, 1 / R, mp(k[0]) if k else mpmath.mpf(0), mp(k[1]) if k else mpmath.mpf(0), mpmath.mpf(1)]
        ev = lambda expr: sp.lambdify(_args(s), expr, modules="mpmath")(*vals)
        S = mpmath.mpf(num) / (den * mpmath.pi)
        ev3 = lambda T: [[[ev(T[a][b][j]) for j in range(3)] for b in range(K1)] for a in range(K0)]
        D, Nn = ev3(DU), (ev3(NU) if has_n else None)
        fv, wv, evv = [mp(x) for x in f], [mp(x) for x in w], [mp(x) for x in e]
        mv = [mp(x) for x in m] if has_n else None
        du = [S * sum(fv[a] * sum(D[a][b][j] * evv[j] + (Nn[a][b][j] * mv[j] if has_n else 0) for j in range(3)) for a in range(K0)) for b in range(K1)]
        g = [S * sum(wv[b] * fv[a] * D[a][b][j] for a in range(K0) for b in range(K1)) for j in range(3)]
        gn = [S * sum(wv[b] * fv[a] * Nn[a][b][j] for a in range(K0) for b in range(K1)) for j in range(3)] if has_n else None
        return du, g, gn
