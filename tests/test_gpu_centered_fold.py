"""The fp64 tile-centred single layer with the density folded into the far records (sctl_amd/csrc/centered_kernel.hpp, CenteredFxU<double>::FOLD):
far sources in two lists by the sign of the density, f == 0 dropped, non-finite or extreme densities sent to the exact pair.  Each case against the
exact all-pairs kernel (SCTL_AMD_CENTERED=0) on all targets and, where the values are finite, against the CPU oracle."""
import os

import numpy as np
import pytest

import sctl_amd
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAME = "Laplace3D-FxU"
NT, NS = 20000 + 37, 30011      # ragged: not multiples of the 256-target wave or the 64-source tile


def _eval(xt, xs, f, centred, digits=-1):
    import torch
    os.environ["SCTL_AMD_CENTERED"] = "1" if centred else "0"
    try:
        assert sctl_amd.plan(NAME, 0, xt.size // 3, xs.size // 3, digits=digits)["path"] == ("tile-centred" if centred else "exact")
        d = [torch.from_numpy(a).cuda() for a in (xt, xs, f)]
        return sctl_amd.eval_device(NAME, d[0], d[1], None, d[2], digits=digits).cpu().numpy()
    finally:
        del os.environ["SCTL_AMD_CENTERED"]


def _rel(u, ref):
    """rel-L2 after scaling both by the largest |ref| (densities of 1e200 would overflow the squares)"""
    s = np.abs(ref).max()
    return rel_l2(u / s, ref / s) if s > 0 else float(np.abs(u).max())


def _densities(kind, rng):
    f = rng.random(NS) - 0.5
    if kind == "positive":
        return 0.1 + rng.random(NS)
    if kind == "negative":
        return -0.1 - rng.random(NS)
    if kind == "zeros":                  # exact zeros contribute exactly 0 and are dropped from the far lists
        f[rng.random(NS) < 0.3] = 0.0
        return f
    if kind == "tiny":                   # |f| = 1e-200 (f^2 underflows: the exact pair) next to O(1) values
        sel = rng.random(NS) < 0.1
        f[sel] = np.where(rng.random(sel.sum()) < 0.5, 1e-200, -1e-200)
        return f
    if kind == "huge":                   # |f| = 1e200 (f^2 overflows: the exact pair) next to O(1) values
        sel = rng.random(NS) < 0.01
        f[sel] = np.where(rng.random(sel.sum()) < 0.5, 1e200, -1e200)
        return f
    if kind == "all_tiny":
        return 1e-200 * f
    if kind == "all_huge":
        return 1e200 * f
    return f                             # "mixed"


@pytest.mark.parametrize("kind", ["positive", "negative", "mixed", "zeros", "tiny", "huge", "all_tiny", "all_huge"])
def test_folded_densities_match_exact_kernel_and_oracle(O, kind):
    rng = np.random.default_rng(2024)
    xt, xs = rng.random(NT * 3), rng.random(NS * 3)
    f = _densities(kind, rng)
    u = _eval(xt, xs, f, True)
    ue = _eval(xt, xs, f, False)
    assert np.all(np.isfinite(u))
    assert _rel(u, ue) <= 2e-14, (kind, _rel(u, ue))
    sel = rng.choice(NT, 200, replace=False)
    ref = O.eval(NAME, xt.reshape(NT, 3)[sel].ravel().copy(), xs, None, f)
    assert _rel(u[sel], ref) <= 1e-12, (kind, _rel(u[sel], ref))
    assert np.array_equal(u, _eval(xt, xs, f, True))             # run to run: bit for bit
    for digits, tol in ((10, 1e-13), (3, 1e-6)):                  # the 10-digit Newton step (MODE 1) and the bare seed (MODE 0) fold the same way
        u_d, ue_d = _eval(xt, xs, f, True, digits), _eval(xt, xs, f, False, digits)
        assert _rel(u_d, ue_d) <= tol, (kind, digits, _rel(u_d, ue_d))


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "inf_and_-inf"])
def test_non_finite_densities_propagate_as_in_the_exact_kernel(bad):
    rng = np.random.default_rng(7)
    xt, xs = rng.random(NT * 3), rng.random(NS * 3)
    f = rng.random(NS) - 0.5
    idx = rng.choice(NS, 2, replace=False)
    f[idx] = {"nan": (np.nan, 0.25), "inf": (np.inf, 0.25), "-inf": (-np.inf, 0.25), "inf_and_-inf": (np.inf, -np.inf)}[bad]
    u, ue = _eval(xt, xs, f, True), _eval(xt, xs, f, False)
    assert not np.any(np.isfinite(ue))
    assert np.array_equal(np.isnan(u), np.isnan(ue)) and np.array_equal(np.isinf(u), np.isinf(ue))
    assert np.array_equal(np.sign(u[np.isinf(u)]), np.sign(ue[np.isinf(ue)]))


@pytest.mark.parametrize("npos,nneg", [(1, 2), (2, 1), (3, 3), (5, 0), (0, 7), (61, 66), (130, 3), (4, 8)])
def test_ragged_leftovers_of_either_list(O, npos, nneg):
    """Targets in a small cube far from every source: all sources are far, so each wave's positive and negative lists hold exactly npos and nneg
    records and leave npos % 4 and nneg % 4 of them to the tail; exact zeros fill the source set up to the 64 the centred path needs."""
    rng = np.random.default_rng(npos * 1000 + nneg)
    nt, ns = 1000, max(100, npos + nneg + 11)
    xt = 0.01 * rng.random(nt * 3)
    xs = 0.5 + 0.5 * rng.random(ns * 3)
    f = np.zeros(ns)
    f[:npos] = 0.1 + rng.random(npos)
    f[npos:npos + nneg] = -0.1 - rng.random(nneg)
    f = f[rng.permutation(ns)]
    u, ue = _eval(xt, xs, f, True), _eval(xt, xs, f, False)
    ref = O.eval(NAME, xt, xs, None, f)
    assert _rel(u, ue) <= 2e-14, _rel(u, ue)
    assert _rel(u, ref) <= 1e-12, _rel(u, ref)
