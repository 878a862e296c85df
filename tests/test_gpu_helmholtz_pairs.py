"""The fp64 Helmholtz kernel one pair at a time, on the device, against long double.

The kernel evaluates e^{ikr} from LDS tables that every workgroup fills itself (include/sctl_amd/device/fastmath.hpp; HelmholtzConsts<double> in
device/ukernels.hpp), by one of several routes per launch, tile and pair, and with the constants of three accuracy modes.  The sums the other GPU
tests compare (rel-L2 over hundreds of sources, bar 1e-12) cannot see one wrong table node or one pair on the wrong route.  Here exactly ONE
source carries the density 1 + 0i and every other source the density 0: a target's output is then the device's value of one pair,
G = e^{ikr} / (4 pi r), re and im.  The other sources add exact zeros but still fill tiles and set a tile's largest distance, so they decide which
pass and which fallback the probed pair goes through.

Truth: the same fp64 coordinates in np.longdouble (64-bit significand, asserted below), r from the exact coordinate differences.

Measure, full precision (digits = -1, mode 2):
    q = |G_dev - G_true| / (max(|G_true|, 2^-1022) 2^-53 (1 + (|Re k| + |Im k|) r))
i.e. the error in units of half an ulp of the value, with the amplification of the kernel's own few-ulp error in r by dG/dr = (ik - 1/r) G taken
out.  (Below the smallest normal number the spacing of doubles no longer shrinks with the value, hence the max.)

The bar is NOT a number chosen for the device: every case runs the same pairs through the CPU oracle (fp64 libm, the project's reference), takes
ITS largest q, and allows the device FACTOR times that.  FACTOR = 6, from the worst case of what the device does per pair, in half-ulps (2^-53):
  * r, whose relative error enters q with the weight |ik - 1/r| r / (1 + |k| r) <= 1: r^2 from two FMAs and a product (about 1 ulp), the refined
    reciprocal square root with three roundings on its main path (2.5 ulp worst case, profiles/r03_rsq_refine_accuracy.txt), the product
    r^2 (C / r) (0.5 ulp): 4 ulp = 8 half-ulps, against the oracle's r^2 and a correctly rounded sqrt;
  * e^{ikr}: the table forms are within 4.5e-16 of the modulus (tests/test_fastmath.py): 4, against libm's 1 - 2;
  * the amplitude (1 / r times the period factor or the exponential), the product with the node value, the product with the density, the scale:
    4 roundings of half an ulp each: 4 (the oracle has the same).
Worst case 8 + 4 + 4 = 16 half-ulps; the oracle's largest q over a probe set is 2.3 - 3.8 wherever it has been measured, and 16 / 2.7 = 6.  The
issue that asked for this test expected 4 - 6 and treats more than 8 as a finding.  Measured on an MI355X: 0.8 - 1.44 times the oracle's, device
q at most 5.2 (profiles/r20_helmholtz_pairs.txt holds both columns per route and mode).

Lower accuracy modes (digits = 10 -> mode 1, C = 2; digits = 5 -> mode 0, C = 1; capi.hip: mode_for): r is only good to the mode's digits, so the
bar is the project's own 10 * 10^-digits (tests/conftest.py: tol_for) on |G_dev - G_true| / (|G_true| (1 + (|Re k| + |Im k|) r)), per pair.

Every probed pair enters the maximum; a non-finite device value where the truth is finite fails; a truth that is 0 as a double must
come out 0, and one that is inf must not come out finite (the output is the complex product G (1 + 0i), and inf * 0 makes that NaN in IEEE
arithmetic, in the oracle as in the kernel).  One exception is stated, not hidden: for a GROWING wave (Im k < 0) the kernel, like the oracle and like the reference,
forms e^{-Im k r} before it multiplies by 1 / r, so in the narrow window where e^{-Im k r} has left the double range but G has not
(709.8 < -Im k r < 709.8 + ln(4 pi r)) both return inf; the growth probes stay out of that window (it is 8 wide in -Im k r at r = 355).
"""
import numpy as np
import pytest

import sctl_amd

pytestmark = pytest.mark.gpu

NAME = "Helmholtz3D-FxU"
LD = np.longdouble
FACTOR = 6.0
NPROBE = 4096            # 16 workgroups of four waves; the last wave holds the r = 0 and r = 1e-8 probes
NSPECIAL = 64
TILE, WAVE = 256, 64     # eval_kernel.hpp: kTile; lanes of a wave
PHASE_ONE = 1600.0       # fastmath.hpp: kCexpMaxPhase
PHASE_TWO = 1.2e4        # kSincosTabMaxArg
EXP_MAX = 1.0e6          # kExpTabMaxArg
DIGITS_OF_MODE = {2: -1, 1: 10, 0: 5}     # capi.hip mode_for: digits < 0 or > 14 -> 2, <= 7 -> 0, else 1

USABLE = [(7.5, 0.3), (7.5, 0.0), (40.0, 10.0), (40.0, -10.0), (900.0, 5.0), (1e-3, 2e-4)]
REFUSED = [(40.0, float(np.nextafter(10.0, 11.0))), (-3.0, 2.5), (0.0, 0.7), (3.0, 60.0), (5.0, -2.0)]
ONE_WAVE_K = [(7.5, 0.3), (7.5, 0.0), (900.0, 5.0), (-3.0, 2.5), (0.0, 0.7)]
MODE_K = [(7.5, 0.3), (900.0, 5.0), (-3.0, 2.5)]


def kid(k):
    return "k=%g%+gi" % k


def test_long_double_is_wider_than_the_device():
    assert np.finfo(LD).eps < 2e-19


def usable(k):
    """CexpCoeffsK::usable(Re k, -Im k)"""
    return k[0] > 0 and abs(k[1]) <= 0.25 * k[0] and 1e-150 < k[0] < 1e150


# ---- truth and measure -----------------------------------------------------------------------------------------------------------------
_PI = 4 * np.arctan(LD(1))


def truth(x, p, k):
    """(r, G) in long double for the points x (n, 3) against the point p: r from the exact differences of the fp64 coordinates"""
    d = x.astype(LD) - p.astype(LD)[None, :]
    r = np.sqrt((d * d).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        amp = np.exp(-LD(k[1]) * r) / (4 * _PI * r)
        g = np.stack([amp * np.cos(LD(k[0]) * r), amp * np.sin(LD(k[0]) * r)], axis=1)
    g[r == 0] = 0
    return r, g


def measure(dev, x, p, k):
    """(q per pair, e per pair): the error of the device (or oracle) values dev (n, 2) in the two measures of the module docstring.  Pairs whose truth
    is 0 or inf as a double are checked here for being 0 or inf and get q = e = 0."""
    r, g = truth(x, p, k)
    mod = np.sqrt((g * g).sum(axis=1))
    kk = LD(abs(k[0]) + abs(k[1]))
    tiny, huge = LD(2.0) ** -1022, LD(np.finfo(np.float64).max)
    zero = mod < LD(2.0) ** -1080                       # every rounding of the kernel's products gives 0 here
    over = (np.abs(g) > huge).any(axis=1)
    assert not (over & ~(np.abs(g) > huge).all(axis=1)).any(), "a growth probe with one finite component: move it"
    assert np.all(dev[zero] == 0.0), "a pair whose truth is 0: %r" % (dev[zero][np.any(dev[zero] != 0, axis=1)][:4],)
    # an infinite G: the output is the complex product G (1 + 0i), whose terms inf * 0 make it NaN in IEEE arithmetic, in the kernel as in
    # the oracle; what can be asked is that nothing finite comes out
    assert not np.isfinite(dev[over]).any(), "a pair whose truth is inf"
    rest = ~(zero | over)
    assert np.all(np.isfinite(dev[rest])), "non-finite values at r = %r" % (r[rest][~np.isfinite(dev[rest]).all(axis=1)][:4].astype(np.float64),)
    dl = dev.astype(LD) - g
    err = np.sqrt((dl[rest] ** 2).sum(axis=1))
    amp = 1 + kk * r[rest]
    q, e = np.zeros(r.size), np.zeros(r.size)
    q[rest] = (err / (np.maximum(mod[rest], tiny) * LD(2.0) ** -53 * amp)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e[rest] = np.where(mod[rest] > 0, err / (mod[rest] * amp), err).astype(np.float64)
    return q, e, r.astype(np.float64)


# ---- geometry --------------------------------------------------------------------------------------------------------------------------
P0 = np.array([0.3183098861837907, 0.2718281828459045, 0.1414213562373095])      # the probed point: no round numbers


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def ball(rng, n, centre, radius):
    return centre[None, :] + radius * (rng.random(n) ** (1 / 3))[:, None] * unit(rng, n)


def scales(k):
    """(P, L, periods): the period of the phase (of the exponential's table when Re k = 0) and the largest probed distance: 256 periods, or where
    |Im k| r = 650 (e^{+-650} is a normal double), whichever comes first"""
    kr, ki = abs(k[0]), abs(k[1])
    P = 2 * np.pi / kr if kr else np.log(2) / ki
    L = min(256 * P if kr else np.inf, 650 / ki if ki else np.inf)
    return P, L, int(min(256, L // P))


def special_distances(rng):
    """the last wave: coincident probes (r = 0: the value must be exactly 0), r = 1e-8, and in between up to 1e-3"""
    return np.concatenate([np.zeros(8), np.full(28, 1e-8), 10.0 ** rng.uniform(-8, -3, NSPECIAL - 36)])


def standard_distances(k, rng):
    """NPROBE distances: uniform over all periods; the first and the last period; within one reduction step h = P / 2048 of the period boundaries
    m P for a sample of m that holds 1, 127, 128, 254, 255 and 256 where the wavenumber reaches them; the special wave"""
    P, L, nper = scales(k)
    h = P / 2048
    n = NPROBE - NSPECIAL
    groups = [rng.random(1344) * L, rng.random(512) * P, L - rng.random(512) * P]
    ms = sorted({m for m in (1, 2, 3, 64, 127, 128, 129, 200, 254, 255, 256, nper // 2, nper - 1, nper) if 1 <= m <= nper})
    per = (n - 2368) // len(ms)
    for m in ms:
        groups.append(m * P + np.concatenate([[0, h, -h, h / 2, -h / 2], (rng.random(per - 5) * 2 - 1) * h]))
    r = np.concatenate(groups)
    r = np.concatenate([r, rng.random(n - r.size) * L, special_distances(rng)])
    assert r.size == NPROBE and np.all(r >= 0)
    return r, ms


def points_at(r, rng, directions=None):
    u = unit(rng, r.size) if directions is None else directions
    return P0[None, :] + r[:, None] * u


def standard_case(k, seed, n_other, probe_index):
    """probes at standard_distances around P0 in random directions; the other points in a ball of 1 % of the largest distance around P0"""
    rng = np.random.default_rng(seed)
    r, ms = standard_distances(k, rng)
    x = points_at(r, rng)
    _, L, _ = scales(k)
    other = ball(rng, n_other, P0, 0.01 * L)
    other[probe_index] = P0
    return x, other


# ---- routes: each returns the device's (n, 2) values of the pairs (probe point, others[probe_index]) ------------------------------------
def ctx_of(k):
    return np.array(k, dtype=np.float64)


def flat(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def fwd_host(x, others, idx, k, digits):
    f = np.zeros(others.shape[0] * 2)
    f[2 * idx] = 1.0
    return sctl_amd.eval_host(NAME, flat(x), flat(others), None, f, ctx=ctx_of(k), digits=digits).reshape(-1, 2)


def fwd_device(x, others, idx, k, digits):
    import torch
    f = np.zeros(others.shape[0] * 2)
    f[2 * idx] = 1.0
    d = [torch.from_numpy(a).to("cuda:0") for a in (flat(x), flat(others), f)]
    return sctl_amd.eval_device(NAME, d[0], d[1], None, d[2], ctx=ctx_of(k), digits=digits).cpu().numpy().reshape(-1, 2)


def matrix_host(x, others, idx, k, digits):
    M = sctl_amd.kernel_matrix_host(NAME, flat(x), flat(others), None, ctx=ctx_of(k), digits=digits)
    return M[2 * idx].reshape(-1, 2).copy()


def list_host(x, others, idx, k, digits):
    f = np.zeros(others.shape[0] * 2)
    f[2 * idx] = 1.0
    one = lambda v: np.array([v], dtype=np.int64)
    return sctl_amd.eval_lists_host(NAME, one(0), one(x.shape[0]), one(0), one(others.shape[0]), flat(x), flat(others), None, f, ctx=ctx_of(k),
                                    digits=digits).reshape(-1, 2)


def transpose_host(x, others, idx, k, digits):
    """the probes are the SOURCES here and own the output; one TARGET (others[idx]) carries the weight 1 + 0i: g = (Re G, -Im G)"""
    w = np.zeros(others.shape[0] * 2)
    w[2 * idx] = 1.0
    g = sctl_amd.eval_transpose_host(NAME, flat(others), flat(x), None, w, ctx=ctx_of(k), digits=digits).reshape(-1, 2)
    return g * np.array([1.0, -1.0])


def tiles_per_split(n_streamed, splits):
    return -(-(-(-n_streamed // TILE)) // splits)


def speculative_count(transposed=False):
    """The smallest number of streamed points (sources forward, targets transposed; ragged last tile) at which a workgroup of the all-pairs evaluator
    runs its unmasked pass: `always_masked = ntile < 4` (eval_kernel.hpp, eval_transpose_kernel.hpp) with ntile the tiles of ONE split of the plan."""
    def splits(n):
        if transposed:
            return sctl_amd.plan_transpose(NAME, 0, n, NPROBE)["splits"]
        return sctl_amd.plan(NAME, 0, NPROBE, n)["src_splits"]
    for ntile in range(4, 4096):
        n = ntile * TILE - 100
        if tiles_per_split(n, splits(n)) >= 4:
            assert tiles_per_split(n - TILE, splits(n - TILE)) < 4
            return n, tiles_per_split(n, splits(n))
    raise AssertionError("no speculative size")


def streamed_count(which, transposed=False):
    """(points streamed past the probes, index of the probed one among them): 900 for the careful pass (one tile per split: the masked loop only),
    the planner's threshold for the speculative one, where the probed point sits in the second tile of the fourth split"""
    if which == "careful":
        n = 900
        s = sctl_amd.plan_transpose(NAME, 0, n, NPROBE)["splits"] if transposed else sctl_amd.plan(NAME, 0, NPROBE, n)["src_splits"]
        assert tiles_per_split(n, s) < 4
        return n, 300
    n, per = speculative_count(transposed)
    return n, (3 * per + 1) * TILE + 77


# ---- the bar ---------------------------------------------------------------------------------------------------------------------------
def check(O, label, dev, x, p, k, mode=2, coincident=True):
    """dev against the truth, and against the oracle's error on the same pairs (mode 2) or the mode's digits (modes 1, 0)"""
    qd, ed, r = measure(dev, x, p, k)
    ref = O.eval(NAME, flat(x), flat(p), None, np.array([1.0, 0.0]), ctx=ctx_of(k)).reshape(-1, 2)
    qo, eo, _ = measure(ref, x, p, k)
    i = int(np.argmax(qd))
    print("PAIRS %-44s mode %d  oracle q %6.2f  device q %6.2f  ratio %5.2f  device e %.2e  (worst at r = %.17g, |k| r = %.4g)"
          % (label, mode, qo.max(), qd.max(), qd.max() / qo.max(), ed.max(), r[i], (abs(k[0]) + abs(k[1])) * r[i]))
    assert not coincident or (np.all(dev[r == 0] == 0.0) and (r == 0).sum() == 8)
    if mode == 2:
        assert qd.max() <= FACTOR * qo.max(), (label, qd.max(), qo.max(), r[i])
    else:
        digits = DIGITS_OF_MODE[mode]
        assert ed.max() <= 10.0 * 10.0 ** -digits, (label, ed.max(), r[i])
    return qd, r


# ---- all-pairs forward, the one-reduction form and its refusals ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["careful", "speculative"])
@pytest.mark.parametrize("k", USABLE + REFUSED, ids=kid)
def test_all_pairs_forward(O, k, which):
    """eval_host over the standard distances: the six wavenumbers the one-reduction form accepts (the decay ratio of exactly 1/4 with both signs
    among them) and its five refusals, which run the two-reduction form: the next double after the ratio 1/4, Re k < 0, Re k = 0, strong decay,
    growth.  Distances beyond a phase of 1600 (the last 1.4 of the 256 periods) take libm per pair in the careful pass and re-run their tile
    in the speculative one."""
    ns, idx = streamed_count(which)
    x, others = standard_case(k, [11, USABLE.index(k) if k in USABLE else 10 + REFUSED.index(k)], ns, idx)
    check(O, "all-pairs %s %s" % (which, kid(k)), fwd_host(x, others, idx, k, -1), x, others[idx], k)


def test_all_pairs_device_entry(O):
    """the device-resident entry runs the same kernel: one wavenumber, speculative size"""
    k = (7.5, 0.3)
    ns, idx = streamed_count("speculative")
    x, others = standard_case(k, [12], ns, idx)
    check(O, "all-pairs device entry %s" % kid(k), fwd_device(x, others, idx, k, -1), x, others[idx], k)


# ---- range edges -----------------------------------------------------------------------------------------------------------------------
def edge_case(k, limit_phase, seed, n_other, tiles):
    """Probes on both sides of the distance r_lim = limit_phase / |Re k|.  Workgroups 0 - 7 hold probes at 0.1 - 0.95 r_lim, workgroups 8 - 15 a mix of
    0.85 - 1.08 r_lim in every wave.  The other points lie within 0.5 % of r_lim of P0, except those of the tiles named in `tiles[1:]`, which fill a
    ball of radius r_lim: tile tiles[0] (compact) is within range for every wave of the first half and beyond it for every wave of the second, the
    spread tiles are beyond range for every wave.  Returns the probes, the other points and one probed index per tile of `tiles`."""
    rng = np.random.default_rng(seed)
    rl = limit_phase / abs(k[0])
    n = NPROBE - NSPECIAL
    r = np.concatenate([rng.uniform(0.1, 0.95, n // 2) * rl, rng.uniform(0.85, 1.08, n - n // 2) * rl, special_distances(rng)])
    x = points_at(r, rng)
    other = ball(rng, n_other, P0, 0.005 * rl)
    idx = []
    for j, t in enumerate(tiles):
        if j > 0:
            other[t * TILE:(t + 1) * TILE] = ball(rng, min(TILE, n_other - t * TILE), P0, rl)
        idx.append(min(t * TILE + 77 + j, n_other - 1))
        other[idx[-1]] = P0 + (np.array([1e-3, -2e-3, 1.5e-3]) * rl * j)
    return x, other, idx, rl


def waves_beyond(x, tile_points, k, limit_phase):
    """per wave of the probes: does any (probe, point of the tile) distance exceed the limit (what tile_bad reports, up to its 2^-20 rounding up)"""
    d = np.sqrt(((x[:, None, :] - tile_points[None, :, :]) ** 2).sum(axis=2)).max(axis=1)
    return (abs(k[0]) * d).reshape(-1, WAVE).max(axis=1) > limit_phase


@pytest.mark.parametrize("which", ["careful", "speculative"])
@pytest.mark.parametrize("k,limit", [((1000.0, 0.5), PHASE_ONE), ((1000.0, 0.0), PHASE_ONE), ((2.0e4, 1.0), PHASE_ONE), ((3.0e4, 0.0), PHASE_ONE),
                                     ((2.0e4, 1.0), PHASE_TWO), ((3.0e4, 0.0), PHASE_TWO), ((-2.0e4, 1.0), PHASE_TWO), ((-3.0e4, 0.0), PHASE_TWO)],
                         ids=lambda v: kid(v) if isinstance(v, tuple) else "phase%g" % v)
def test_all_pairs_phase_limit(O, k, limit, which):
    """One launch with tiles on both sides of the table's range and probed pairs on both sides of it.  Re k > 0 runs the one-reduction form, whose
    limit is a phase of 1600 (beyond: libm, also around 1.2e4); Re k < 0 the two-reduction form, whose limit is 1.2e4.  The probed source sits
    once in a compact tile (in range for half the waves) and once in a spread one (every wave re-runs it)."""
    ns, idx0 = streamed_count(which)
    t0 = idx0 // TILE
    x, others, idx, rl = edge_case(k, limit, [13, int(abs(k[0])), int(limit), k[0] < 0], ns, [t0, t0 + 1])
    own = PHASE_ONE if usable(k) else PHASE_TWO
    for j, i in enumerate(idx):
        t = i // TILE
        beyond = waves_beyond(x, others[t * TILE:(t + 1) * TILE], k, own)
        if limit == own:
            assert (not beyond[:28].any() and beyond[32:63].all()) if j == 0 else beyond[:63].all()
        _, r = check(O, "all-pairs %s %s around %g, %s tile" % (which, kid(k), limit, "spread" if j else "compact"),
                     fwd_host(x, others, i, k, -1), x, others[i], k, coincident=(j == 0))   # (the second probed source lies a little off P0)
        ph = abs(k[0]) * r
        assert (ph < 0.9 * limit).sum() > 500 and (ph > limit).sum() > 500 and ((ph > 0.999 * limit) & (ph < 1.001 * limit)).sum() >= 10


@pytest.mark.parametrize("which", ["careful", "speculative"])
def test_all_pairs_decay_leaves_the_double_range(O, which):
    """k = 3 + 60i: |Im k| r from 650 through the last normal and subnormal values (745) to 0, then far beyond — past kExpTabMaxArg = 1e6, where the
    speculative pass must notice (tile_bad) and the careful pass clamps.  Every value is 0 in truth from 760 on and must be exactly 0."""
    k = (3.0, 60.0)
    rng = np.random.default_rng(14)
    n = NPROBE - NSPECIAL
    a = np.concatenate([rng.uniform(650, 800, n - 512), 10.0 ** rng.uniform(3, 6.5, 256), EXP_MAX * rng.uniform(0.999, 1.001, 256)])
    x = points_at(np.concatenate([a / k[1], special_distances(rng)]), rng)
    ns, idx = streamed_count(which)
    others = ball(rng, ns, P0, 0.05)
    others[idx] = P0
    dev = fwd_host(x, others, idx, k, -1)
    check(O, "all-pairs %s %s decay to 0" % (which, kid(k)), dev, x, others[idx], k)
    assert np.all(dev[n - 512:n] == 0.0)


@pytest.mark.parametrize("which", ["careful", "speculative"])
def test_all_pairs_growth_leaves_the_double_range(O, which):
    """k = 5 - 2i: -Im k r from 650 to 709.7 (finite) and from 740 to 800 (inf in truth, both components: nothing finite may come out).  A zero
    density times an infinite G would be NaN, so probes and zero-density sources share one thin segment 325 - 400 away from the probed source,
    where every distance between them keeps G finite (and there is no wave of coincident probes here); the window where the exponential has
    overflowed and G has not is left out (module docstring)."""
    k = (5.0, -2.0)
    rng = np.random.default_rng(15)
    half = NPROBE // 2
    a = np.concatenate([rng.uniform(650, 709.7, half), rng.uniform(740, 800, NPROBE - half)])
    u0 = np.array([0.6, 0.48, 0.64])

    def across(n):                                    # a little off the segment, at right angles to it: r grows by less than 1e-3
        j = rng.normal(size=(n, 3)) * 0.3
        return j - (j @ u0)[:, None] * u0[None, :]
    x = points_at(a / 2.0, rng, directions=np.tile(u0, (NPROBE, 1))) + across(NPROBE)
    ns, idx = streamed_count(which)
    others = P0[None, :] + rng.uniform(325, 400, ns)[:, None] * u0[None, :] + across(ns)
    others[idx] = P0
    dev = fwd_host(x, others, idx, k, -1)
    check(O, "all-pairs %s %s growth to inf" % (which, kid(k)), dev, x, others[idx], k, coincident=False)
    assert np.all(np.isfinite(dev[:half])) and not np.isfinite(dev[half:]).any()


# ---- one-wave evaluators: always the small tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [matrix_host, list_host], ids=["matrix", "list"])
@pytest.mark.parametrize("k", ONE_WAVE_K, ids=kid)
def test_one_wave_evaluators(O, k, route):
    """kernel_matrix_host (per pair by construction; 5 sources) and a single list through eval_lists_host (900 sources): the two-reduction form
    whatever the wavenumber, so 900 + 5i runs sincos_tab_k / exp_tab_k here and cexp_tab_k in the all-pairs cases"""
    ns, idx = (5, 2) if route is matrix_host else (900, 300)
    x, others = standard_case(k, [16, ONE_WAVE_K.index(k)], ns, idx)
    check(O, "%s %s" % (route.__name__, kid(k)), route(x, others, idx, k, -1), x, others[idx], k)


@pytest.mark.parametrize("route", [matrix_host, list_host], ids=["matrix", "list"])
@pytest.mark.parametrize("k", [(2.0e4, 1.0), (3.0e4, 0.0)], ids=kid)
def test_one_wave_phase_limit(O, k, route):
    """the two-reduction form's own limit, |Re k| r = 1.2e4, with pairs on both sides (libm beyond); the list has a compact and a spread tile"""
    ns = 5 if route is matrix_host else 900
    x, others, idx, rl = edge_case(k, PHASE_TWO, [17, int(k[0])], ns, [0] if route is matrix_host else [1, 2])
    for j, i in enumerate(idx):
        check(O, "%s %s around 1.2e4" % (route.__name__, kid(k)), route(x, others, i, k, -1), x, others[i], k, coincident=(j == 0))


# ---- transposed all-pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["careful", "speculative"])
@pytest.mark.parametrize("k", [(7.5, 0.3), (-3.0, 2.5)], ids=kid)
def test_all_pairs_transposed(O, k, which):
    """eval_transpose_host: the probes are sources, one target carries the weight 1 + 0i, every other target the weight 0"""
    nt, idx = streamed_count(which, transposed=True)
    x, others = standard_case(k, [18, int(k[0] > 0)], nt, idx)
    check(O, "transposed %s %s" % (which, kid(k)), transpose_host(x, others, idx, k, -1), x, others[idx], k)


# ---- accuracy modes: the constants of C = 2 and C = 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("route", ["careful", "speculative", "matrix"])
@pytest.mark.parametrize("k", MODE_K, ids=kid)
def test_accuracy_modes(O, k, route, mode):
    """digits = 10 (mode 1: the distance arrives as 2 r) and digits = 5 (mode 0: as r), the default's 0x1.555555p+1 r being every case above"""
    digits = DIGITS_OF_MODE[mode]
    if route == "matrix":
        ns, idx, run = 5, 2, matrix_host
    else:
        (ns, idx), run = streamed_count(route), fwd_host
    x, others = standard_case(k, [19, MODE_K.index(k)], ns, idx)
    check(O, "%s %s digits %d" % (route, kid(k), digits), run(x, others, idx, k, digits), x, others[idx], k, mode=mode)


# ---- independence from company -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [(7.5, 0.3), (-3.0, 2.5)], ids=kid)
def test_a_pair_does_not_depend_on_its_neighbours(k):
    """The probed pairs' values, bit for bit, with two different sets of zero-density sources at similar distances (every tile within range both
    times: the same route, other neighbours).  A lane that read another lane's table node would show here."""
    ns, idx = streamed_count("speculative")
    rng = np.random.default_rng(20)
    P, L, _ = scales(k)
    x = points_at(np.concatenate([rng.random(NPROBE - NSPECIAL) * 0.9 * min(L, PHASE_ONE / abs(k[0])), special_distances(rng)]), rng)
    out = []
    for draw in range(2):
        others = ball(rng, ns, P0, 0.01 * L)
        others[idx] = P0
        out.append(fwd_host(x, others, idx, k, -1))
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))
    assert np.count_nonzero(out[0]) >= 2 * (NPROBE - 8)
