"""The two functors the reference does not have are this repository's on every side: HIP, oracle and the functor
text instantiated on the reference's GenericKernel.  These tests pin them to INDEPENDENT mathematics instead:
  Helmholtz3D-FxU   against numpy complex128  sum_s exp(i k r) / (4 pi r) f_s  with a complex wavenumber;
  Laplace3D-FDxUdU  potential against numpy  sum_s q/(4 pi r) + mu (r.n)/(4 pi r^3), gradient against central finite differences
                    of that numpy potential (truncation error O(h^2), so the tolerance is 1e-6, not rounding).
CPU: the oracle.  GPU: the HIP path through the C ABI."""
import numpy as np
import pytest

from conftest import rel_l2


def _helmholtz_numpy(xt, xs, f, k):
    d = xt.reshape(-1, 1, 3) - xs.reshape(1, -1, 3)
    r = np.sqrt((d * d).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(r > 0, np.exp(1j * k * r) / (4 * np.pi * r), 0)
    fc = f[0::2] + 1j * f[1::2]
    u = G @ fc
    return np.stack([u.real, u.imag], 1).ravel()


def _laplace_pot_numpy(x, xs, xn, q, mu):
    d = x.reshape(-1, 1, 3) - xs.reshape(1, -1, 3)
    r2 = (d * d).sum(-1)
    rinv = 1 / np.sqrt(r2)
    rn = (d * xn.reshape(1, -1, 3)).sum(-1)
    return ((q * rinv) + mu * rn * rinv ** 3).sum(1) / (4 * np.pi)


def _helmholtz_case(seed, k):
    rng = np.random.default_rng(seed)
    Nt, Ns = 257, 1000
    xt, xs, f = rng.random(Nt * 3), rng.random(Ns * 3), rng.random(Ns * 2) - 0.5
    xt[:30] = xs[:30]                                     # ten coincident points: G = 0 there
    return xt, xs, f, _helmholtz_numpy(xt, xs, f, k)


def _fused_case(seed):
    rng = np.random.default_rng(seed)
    Nt, Ns = 100, 700
    xt = rng.random(Nt * 3) + 1.5                         # targets away from the sources: smooth field, FD is accurate
    xs, xn = rng.random(Ns * 3), rng.random(Ns * 3) - 0.5
    q, mu = rng.random(Ns) - 0.5, rng.random(Ns) - 0.5
    pot = _laplace_pot_numpy(xt, xs, xn, q, mu)
    h = 1e-4
    grad = np.empty((Nt, 3))
    for j in range(3):
        e = np.zeros(3); e[j] = h
        xp, xm = (xt.reshape(-1, 3) + e).ravel(), (xt.reshape(-1, 3) - e).ravel()
        grad[:, j] = (_laplace_pot_numpy(xp, xs, xn, q, mu) - _laplace_pot_numpy(xm, xs, xn, q, mu)) / (2 * h)
    return xt, xs, xn, np.stack([q, mu], 1).ravel().copy(), pot, grad


K_CASES = [(7.5, 0.3), (20.0, 0.0), (0.5, 2.0), (-3.0, 0.1)]


@pytest.mark.parametrize("k", K_CASES)
def test_oracle_helmholtz_against_numpy_complex(O, k):
    xt, xs, f, ref = _helmholtz_case(3, complex(*k))
    assert rel_l2(O.eval("Helmholtz3D-FxU", xt, xs, None, f, ctx=np.array(k)), ref) < 5e-15


def test_oracle_fused_laplace_against_numpy_and_finite_differences(O):
    xt, xs, xn, f, pot, grad = _fused_case(4)
    u = O.eval("Laplace3D-FDxUdU", xt, xs, xn, f).reshape(-1, 4)
    assert rel_l2(u[:, 0], pot) < 5e-15
    assert rel_l2(u[:, 1:], grad) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("k", K_CASES)
def test_hip_helmholtz_against_numpy_complex(k):
    import sctl_amd
    xt, xs, f, ref = _helmholtz_case(3, complex(*k))
    assert rel_l2(sctl_amd.eval_host("Helmholtz3D-FxU", xt, xs, None, f, ctx=np.array(k)), ref) < 1e-13
    u32 = sctl_amd.eval_host("Helmholtz3D-FxU", xt.astype(np.float32), xs.astype(np.float32), None, f.astype(np.float32), ctx=np.array(k))
    assert rel_l2(u32, ref) < 3e-5


@pytest.mark.gpu
def test_hip_fused_laplace_against_numpy_and_finite_differences():
    import sctl_amd
    xt, xs, xn, f, pot, grad = _fused_case(4)
    u = sctl_amd.eval_host("Laplace3D-FDxUdU", xt, xs, xn, f).reshape(-1, 4)
    assert rel_l2(u[:, 0], pot) < 1e-13
    assert rel_l2(u[:, 1:], grad) < 1e-6
    # the double-layer part alone: gradient of mu (r.n)/r^3
    f_mu = f.copy(); f_mu[0::2] = 0
    u_mu = sctl_amd.eval_host("Laplace3D-FDxUdU", xt, xs, xn, f_mu).reshape(-1, 4)
    f_q = f.copy(); f_q[1::2] = 0
    u_q = sctl_amd.eval_host("Laplace3D-FDxUdU", xt, xs, xn, f_q).reshape(-1, 4)
    assert rel_l2(u_mu + u_q, u) < 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize("k", [(7.5, 0.3), (40.0, 10.0), (40.0, -10.0), (40.0, 0.0), (900.0, 5.0), (3.0, 60.0), (-12.0, 0.5)], ids=lambda k: "k=%g%+gi" % k)
@pytest.mark.parametrize("ns", [1, 2048], ids=["careful_pass", "speculative_pass"])
def test_hip_helmholtz_single_pair_values_against_long_double(k, ns):
    """Every output is ONE kernel value (one active source; the others carry zero density), compared with numpy long double: the error of
    e^{ikr}/(4 pi r) must stay at what the rounding of the distance itself allows, 1e-15 + 4e-16 |k| r relative to |G| (measured: <= 0.7 of
    that).  Guards the table-driven forms at the level a sum over 10^6 sources cannot: a table whose entries were off by j x 2.7e-17 (the
    double-double fill contracted into FMAs by the device compiler, round 3) still passed every 1e-12 rel-L2 check but one."""
    import sctl_amd
    L = np.longdouble
    pi = L("3.14159265358979323846264338327950288")
    rng = np.random.default_rng(1)
    nt = 60000
    r_t = np.sort(rng.random(nt)) * 1.7 + 1e-3
    dirs = rng.standard_normal((nt, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    xt = (dirs * r_t[:, None]).ravel().copy()
    xs = np.zeros(ns * 3)
    xs[3:] = rng.random((ns - 1) * 3) + 5.0
    f = np.zeros(ns * 2)
    f[0] = 1.0
    u = sctl_amd.eval_host("Helmholtz3D-FxU", xt, xs, None, f, ctx=np.array(k)).reshape(nt, 2)
    d = xt.reshape(nt, 3).astype(L)
    r = np.sqrt((d * d).sum(-1))
    amp = np.exp(-L(k[1]) * r) / (4 * pi * r)
    err = np.hypot((u[:, 0] - amp * np.cos(L(k[0]) * r)).astype(np.float64), (u[:, 1] - amp * np.sin(L(k[0]) * r)).astype(np.float64)) / amp.astype(np.float64)
    bound = 1e-15 + 4e-16 * (abs(k[0]) + abs(k[1])) * r_t
    assert (err / bound).max() <= 1.0, (err / bound).max()


# ---- per-pair values of the reference's eight kernels (kernel_functions.hpp:15-198) and the fused Laplace kernel through KernelMatrix -------
def _kernel_values(name, d, n, L=np.longdouble):
    """U(d, n)[k0][k1] with the scale factor, from the formulas of include/sctl/kernel_functions.hpp (cited per kernel), every step in the number
    type L: numpy long double (the truth), or np.float32 (what plain fp32 arithmetic makes of the same formula)."""
    pi = L("3.14159265358979323846264338327950288")
    pi4, pi8 = L(4) * pi, L(8) * pi
    d = d.astype(L)
    n = None if n is None else n.astype(L)
    r2 = (d * d).sum(-1)
    ri = L(1) / np.sqrt(r2)
    ri3 = ri * ri * ri
    ri5 = ri3 * ri * ri
    P = d.shape[0]
    eye = np.eye(3, dtype=L)
    if name == "Laplace3D-FxU":      # :26-30
        return (ri / pi4).reshape(P, 1, 1)
    if name == "Laplace3D-DxU":      # :44-50
        return ((d * n).sum(-1) * ri3 / pi4).reshape(P, 1, 1)
    if name == "Laplace3D-FxdU":     # :64-71, scale -1/(4 pi)
        return (-(d * ri3[:, None]) / pi4).reshape(P, 1, 3)
    stokeslet = (eye[None] * ri[:, None, None] + d[:, :, None] * d[:, None, :] * ri3[:, None, None]) / pi8
    if name == "Stokes3D-FxU":       # :85-94
        return stokeslet
    if name == "Stokes3D-DxU":       # :108-119, scale 3/(4 pi)
        return d[:, :, None] * d[:, None, :] * ((d * n).sum(-1) * ri5)[:, None, None] * (L(3) / pi4)
    if name == "Stokes3D-FxT":       # :133-145, scale -3/(4 pi): u[i][j*3+k] = r_i r_j r_k / r^5
        t = d[:, :, None, None] * d[:, None, :, None] * d[:, None, None, :] * ri5[:, None, None, None]
        return (-(L(3) / pi4) * t).reshape(P, 3, 9)
    if name == "Stokes3D-FSxU":      # :159-171: rows 0-2 the Stokeslet, row 3 the source/sink r_j / r^3
        return np.concatenate([stokeslet, (d * ri3[:, None] / pi8)[:, None, :]], axis=1)
    if name == "Stokes3D-FxUP":      # :185-197: columns 0-2 the Stokeslet, column 3 the pressure r_i / r^3
        return np.concatenate([stokeslet, (d * ri3[:, None] / pi8)[:, :, None]], axis=2)
    if name == "Laplace3D-FDxUdU":   # rows (q, mu) -> columns (u, grad u): q/r + mu (r.n)/r^3 and its gradient in the target
        rn = (d * n).sum(-1)
        U = np.zeros((P, 2, 4), dtype=L)
        U[:, 0, 0] = ri
        U[:, 0, 1:] = -d * ri3[:, None]
        U[:, 1, 0] = rn * ri3
        U[:, 1, 1:] = n * ri3[:, None] - L(3) * d * (rn * ri5)[:, None]
        return U / pi4
    raise ValueError(name)


def _per_pair_error(name, got, ref, d, nn):
    """Relative error of each pair's K0 x K1 block (Frobenius norm) against the long-double block `ref`."""
    den = (ref ** 2).sum((1, 2))
    if name in ("Laplace3D-DxU", "Stokes3D-DxU"):         # values proportional to r.n vanish for r perpendicular to n: measure against |r| |n| instead
        L = np.longdouble
        dl, nl = d.astype(L), nn.astype(L)
        den = den * ((dl * dl).sum(-1) * (nl * nl).sum(-1)) / ((dl * nl).sum(-1) ** 2)
    return np.sqrt((((got - ref) ** 2).sum((1, 2)) / den).astype(np.float64))


def _pair_cloud(info, dt):
    """700 targets x 300 sources in [0,1)^3, 50 of the sources within 1e-3 of the origin (pairs at 1e3 : 1 distance ratios), rounded to dt."""
    rng = np.random.default_rng(11)
    Nt, Ns = 700, 300
    xt = rng.random((Nt, 3)) * np.array([1.0, 1.0, 1.0])
    xs = rng.random((Ns, 3))
    xs[:50] *= 1e-3
    xn = rng.random((Ns, 3)) - 0.5 if info["nd"] else None
    return xt.astype(dt), xs.astype(dt), None if xn is None else xn.astype(dt)


_POWERS = {"Laplace3D-FxU": 1, "Laplace3D-DxU": 3, "Laplace3D-FxdU": 3, "Stokes3D-FxU": 3, "Stokes3D-DxU": 5, "Stokes3D-FxT": 5, "Stokes3D-FSxU": 3,
           "Stokes3D-FxUP": 3, "Laplace3D-FDxUdU": 5}


@pytest.mark.gpu
@pytest.mark.parametrize("digits", [-1, 10])
@pytest.mark.parametrize("name", sorted(_POWERS))
def test_hip_kernel_values_one_pair_at_a_time_against_long_double(name, digits):
    """KernelMatrix entries are single kernel values: each (source, target) block against long double.  Pins the reciprocal-square-root forms
    (ukernels.hpp: rsqrt_cubic83, rsqrt3_cubic, rsqrt5_cubic, the scaled records of the Stokeslet family) pair by pair, where a sum over many
    sources would average their errors away: full precision within a few ulp per power of 1/r, 10 digits within its stated 4.3e-15 per power."""
    import sctl_amd
    info = sctl_amd.kernel_info(name)
    xt, xs, xn = _pair_cloud(info, np.float64)
    Nt, Ns = xt.shape[0], xs.shape[0]
    M = sctl_amd.kernel_matrix_host(name, xt.ravel().copy(), xs.ravel().copy(), None if xn is None else xn.ravel().copy(), digits=digits)
    k0, k1 = info["k0"], info["k1"]
    got = M.reshape(Ns, k0, Nt, k1).transpose(0, 2, 1, 3).reshape(Ns * Nt, k0, k1)
    d = (xt[None, :, :] - xs[:, None, :]).reshape(-1, 3)  # exactly the double subtraction the kernel does
    nn = None if xn is None else np.repeat(xn, Nt, axis=0)
    err = _per_pair_error(name, got, _kernel_values(name, d, nn), d, nn)
    p = _POWERS[name]
    bound = (0.5e-15 + 0.5e-15 * p) if digits < 0 else 5e-15 * p
    # measured on MI355X (round 3), max over the 210 000 pairs: full precision 4.8e-16 (Laplace SL) ... 1.8e-15 (fused Laplace); 10 digits 3.8e-15 ... 2.1e-14
    assert err.max() <= bound, (name, digits, err.max(), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("digits", [-1, 9])
@pytest.mark.parametrize("name", sorted(_POWERS))
def test_hip_fp32_kernel_values_one_pair_at_a_time_against_long_double(name, digits):
    """The same pair-by-pair check for fp32 KernelMatrix at both fp32 accuracies (digits -1: the hardware reciprocal square root as it comes;
    9: one Newton step), on the same cloud rounded to fp32.  The bound is not fitted to the kernel: the formula is evaluated step by step in
    np.float32 (correctly rounded sqrt and divide) on the same pairs, its largest per-pair error against long double is taken, and the kernel is
    allowed 4 times that: its reciprocal square root is the hardware's approximate one, and it builds the powers of 1/r with up to p more
    multiplications than the formula written out."""
    import sctl_amd
    info = sctl_amd.kernel_info(name)
    xt, xs, xn = _pair_cloud(info, np.float32)
    Nt, Ns = xt.shape[0], xs.shape[0]
    M = sctl_amd.kernel_matrix_host(name, xt.ravel().copy(), xs.ravel().copy(), None if xn is None else xn.ravel().copy(), digits=digits)
    assert M.dtype == np.float32
    k0, k1 = info["k0"], info["k1"]
    got = M.reshape(Ns, k0, Nt, k1).transpose(0, 2, 1, 3).reshape(Ns * Nt, k0, k1)
    d = (xt[None, :, :] - xs[:, None, :]).reshape(-1, 3)  # exactly the float subtraction the kernel does
    assert d.dtype == np.float32
    nn = None if xn is None else np.repeat(xn, Nt, axis=0)
    ref = _kernel_values(name, d, nn)
    plain = _kernel_values(name, d, nn, np.float32)
    assert plain.dtype == np.float32
    err, err_plain = _per_pair_error(name, got, ref, d, nn), _per_pair_error(name, plain, ref, d, nn)
    print("%s digits %d: kernel %.3e, plain fp32 formula %.3e" % (name, digits, err.max(), err_plain.max()))
    # measured, max over the 210 000 pairs: plain np.float32 formula | kernel on MI355X at digits -1 | at digits 9
    #   Laplace3D-FxU 2.09e-7 | 1.96e-7 | 2.07e-7     Laplace3D-DxU 5.02e-7 | 4.57e-7 | 5.10e-7     Laplace3D-FxdU 5.21e-7 | 4.67e-7 | 5.21e-7
    #   Laplace3D-FDxUdU 8.65e-7 | 7.91e-7 | 8.52e-7  Stokes3D-FxU 3.07e-7 | 2.87e-7 | 3.14e-7      Stokes3D-DxU 6.86e-7 | 6.41e-7 | 6.90e-7
    #   Stokes3D-FxT 7.61e-7 | 7.13e-7 | 8.95e-7      Stokes3D-FSxU 4.29e-7 | 4.06e-7 | 4.36e-7     Stokes3D-FxUP 4.29e-7 | 4.06e-7 | 4.36e-7
    assert err.max() <= 4 * err_plain.max(), (name, digits, err.max(), err_plain.max())
