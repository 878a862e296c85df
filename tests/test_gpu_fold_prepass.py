"""The fp64 tile-centred single layer with its source pre-pass (sctl_amd/csrc/centered_kernel.hpp: fold_prepass_kernel sorts the sources of every split
by the sign of their density into 64-record tiles once per launch; the kernel's FOLD branch reads them).  Density patterns that reach every branch of
the pre-pass and of the tile's fast (all far) and slow paths, each against the exact all-pairs kernel (SCTL_AMD_CENTERED=0) on ALL targets and against the
CPU oracle on a target subset, at the project's bar for fp64 (rel-L2 <= 1e-12); the 10-digit mode at its own (1e-9, tests/test_gpu_centered.py).

Sizes: the smallest the dispatch sends down this path, 2^18 targets x (2^14 + 37) sources — four splits of 65 tiles, the last one ragged (3941 = 61 x 64 + 37)."""
import os

import numpy as np
import pytest

import sctl_amd
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAME = "Laplace3D-FxU"
NT, NS = 1 << 18, (1 << 14) + 37
CHUNK = 65 * 64                       # sources per split that the planner gives these sizes (four splits: asserted in `clouds`)


@pytest.fixture(scope="module")
def clouds():
    import torch
    rng = np.random.default_rng(2024)
    xt, xs = rng.random(NT * 3), rng.random(NS * 3)
    pl = sctl_amd.plan(NAME, 0, NT, NS)
    assert pl["path"] == "tile-centred" and pl["src_splits"] == -(-NS // CHUNK) == 4, pl
    return {"xt": xt, "xs": xs, "d_xt": torch.from_numpy(xt).cuda(), "d_xs": torch.from_numpy(xs).cuda(), "sel": rng.choice(NT, 200, replace=False)}


def _centred(d_xt, d_xs, f, **kw):
    import torch
    return sctl_amd.eval_device(NAME, d_xt, d_xs, None, torch.from_numpy(f).cuda(), **kw).cpu().numpy()


def _exact(d_xt, d_xs, f):
    import torch
    os.environ["SCTL_AMD_CENTERED"] = "0"
    try:
        assert sctl_amd.plan(NAME, 0, NT, f.size)["path"] == "exact"
        return sctl_amd.eval_device(NAME, d_xt, d_xs, None, torch.from_numpy(f).cuda()).cpu().numpy()
    finally:
        del os.environ["SCTL_AMD_CENTERED"]


def _density(kind, rng):
    mag = rng.random(NS) + 0.1
    sign = rng.choice([-1.0, 1.0], NS)
    if kind == "all_positive":
        return mag
    if kind == "all_negative":
        return -mag
    if kind == "random_signs":
        return mag * sign
    if kind == "one_sign_runs_out":            # 99 % positive: the negative tiles of a split end long before the positive ones
        return mag * np.where(rng.random(NS) < 0.01, -1.0, 1.0)
    if kind == "one_source_of_a_sign":         # exactly one negative source in every split: a tile of one record and 63 of padding
        f = mag.copy()
        f[np.arange(0, NS, CHUNK) + 1234] *= -1
        return f
    if kind == "zeros_mixed_in":
        f = mag * sign
        f[rng.random(NS) < 0.3] = 0.0
        f[7] = -0.0
        return f
    raise ValueError(kind)


def _check(clouds, f, xs=None, d_xs=None, tol=1e-12):
    O = clouds["O"]
    xs = clouds["xs"] if xs is None else xs
    d_xs = clouds["d_xs"] if d_xs is None else d_xs
    u = _centred(clouds["d_xt"], d_xs, f)
    u_exact = _exact(clouds["d_xt"], d_xs, f)
    sel = clouds["sel"]
    ref = O.eval(NAME, clouds["xt"].reshape(NT, 3)[sel].ravel().copy(), xs, None, f)
    e_x, e_o = rel_l2(u, u_exact), rel_l2(u[sel], ref)
    print("rel-L2 vs exact kernel %.2e, vs oracle %.2e" % (e_x, e_o))
    assert np.all(np.isfinite(u))
    assert e_x <= tol and e_o <= tol, (e_x, e_o)
    return u


@pytest.fixture(autouse=True)
def _with_oracle(clouds, O):
    clouds["O"] = O


@pytest.mark.parametrize("kind", ["all_positive", "all_negative", "random_signs", "one_sign_runs_out", "one_source_of_a_sign", "zeros_mixed_in"])
def test_density_patterns_match_exact_kernel_and_oracle(clouds, kind):
    f = _density(kind, np.random.default_rng(7))
    u = _check(clouds, f)
    u10 = _centred(clouds["d_xt"], clouds["d_xs"], f, digits=10)
    assert sctl_amd.plan(NAME, 0, NT, NS, digits=10)["path"] == "tile-centred" and rel_l2(u10, u) <= 1e-9, rel_l2(u10, u)


def test_all_zero_densities_give_exact_zeros(clouds):
    """every source dropped by the pre-pass: no tile, no exception, and the partial sums of every split still written"""
    u = _centred(clouds["d_xt"], clouds["d_xs"], np.zeros(NS))
    assert np.all(u == 0.0)
    f = np.zeros(NS)
    f[NS - 1] = 0.25                             # one source in the last split only
    _check(clouds, f)


@pytest.mark.parametrize("bad", [(np.nan,), (np.inf,), (-np.inf,), (np.nan, np.inf, -np.inf)])
def test_non_finite_densities_propagate_as_in_the_exact_kernel(clouds, bad):
    """not finite: the pre-pass's exception list, the exact pair in every wave — the same NaN / inf pattern target for target.  (1/r > 0 for every pair, so
    a non-finite density reaches every target; what can differ between targets is inf - inf, which both kernels must meet alike.)"""
    rng = np.random.default_rng(8)
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS)
    f[rng.choice(NS, 12 * len(bad), replace=False)] = np.tile(bad, 12)
    u, u_exact = _centred(clouds["d_xt"], clouds["d_xs"], f), _exact(clouds["d_xt"], clouds["d_xs"], f)
    assert np.array_equal(np.isnan(u), np.isnan(u_exact))
    assert np.array_equal(np.isposinf(u), np.isposinf(u_exact)) and np.array_equal(np.isneginf(u), np.isneginf(u_exact))
    assert not np.any(np.isfinite(u))            # (every target sees every source)
    # ... and with the bad sources confined to a zero-weight role the finite ones are still summed right: same densities, bad ones set to 0
    g = np.where(np.isfinite(f), f, 0.0)
    _check(clouds, g)


@pytest.mark.parametrize("scale", [1e160, 1e-160, 1e100, 1e-100, 1e80, 1e-80])
def test_huge_and_tiny_densities(clouds, scale):
    """|f| ~ 1e+-160: f^2 over- or underflows, the exception list; 1e+-100: folded by the pre-pass (k ~ 1e-+200) and thrown back to the exact pair by the kernel's
    band test on k |x_s'|^2; 1e+-80: folded and inside the band, far records with k ~ 1e-+160"""
    rng = np.random.default_rng(9)
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS) * scale
    _check(clouds, f)


def test_magnitudes_mixed_in_one_launch(clouds):
    rng = np.random.default_rng(10)
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS) * rng.choice([1e100, 1e80, 1.0, 1e-80, 1e-100, 1e-160], NS)
    f[:50] = 1e160 * np.sign(f[:50])   # above every band, and not so many that they hide the rest: compared per term below
    u = _check(clouds, f)
    # the small terms for themselves (the large ones dominate the norm above)
    g = np.where(np.abs(f) <= 1.0, f, 0.0)
    _check(clouds, g)
    assert np.all(np.isfinite(u))


def test_sources_equal_to_targets(clouds):
    """coincident pairs contribute exactly 0: they can only be near, and the exact pair masks r = 0"""
    import torch
    rng = np.random.default_rng(11)
    pick = rng.choice(NT, NS, replace=False)
    xs = clouds["xt"].reshape(NT, 3)[pick].ravel().copy()
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS)
    _check(clouds, f, xs=xs, d_xs=torch.from_numpy(xs).cuda())


def test_source_cloud_inside_one_target_cluster(clouds):
    """most tiles mostly near for the waves around the cloud: the slow path of every tile, near lists that fill up between far loops"""
    import torch
    rng = np.random.default_rng(12)
    centre = clouds["xt"].reshape(NT, 3)[12345]
    xs = (centre + 2e-3 * rng.standard_normal((NS, 3))).ravel()
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS)
    _check(clouds, f, xs=xs, d_xs=torch.from_numpy(xs).cuda())


def test_two_runs_are_bit_identical(clouds):
    rng = np.random.default_rng(13)
    f = (rng.random(NS) + 0.1) * rng.choice([-1.0, 1.0], NS)
    f[rng.random(NS) < 0.1] = 0.0
    f[100], f[5000] = 1e170, np.float64(1e-170)
    a, b = _centred(clouds["d_xt"], clouds["d_xs"], f), _centred(clouds["d_xt"], clouds["d_xs"], f)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_operator_handle_and_presorted_slabs_match_the_device_entry(clouds):
    """sctl_amd_op_* keeps the targets sorted (the `presorted` launch), with two devices listed it cuts slabs of 2^17 targets (the slab form of the
    plan: other splits, another summation order — the bar between two orders of the same terms, 2e-14, as tests/test_gpu_centered.py)"""
    rng = np.random.default_rng(14)
    f = (rng.random(NS) + 0.1) * np.where(rng.random(NS) < 0.2, -1.0, 1.0)
    f[::97] = 0.0
    one = _centred(clouds["d_xt"], clouds["d_xs"], f)
    for devs in ((0,), (0, 0)):
        op = sctl_amd.DirectOp(NAME, np.float64, devices=devs)
        op.set_targets(clouds["xt"])
        op.set_sources(clouds["xs"])
        u = np.zeros(NT)
        op.eval(f, u, accumulate=False)
        assert rel_l2(u, one) <= 2e-14, (devs, rel_l2(u, one))
        op.eval(-f, u, accumulate=True)          # the density changes from call to call: the pre-pass runs again
        assert np.max(np.abs(u)) <= 1e-13 * np.max(np.abs(one)), devs
        op.close()
    two = sctl_amd.eval_host(NAME, clouds["xt"], clouds["xs"], None, f, devices=[0, 0])
    assert rel_l2(two, one) <= 2e-14, rel_l2(two, one)
