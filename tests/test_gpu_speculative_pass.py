"""Every all-pairs kernel form through its unmasked pass, a tile repair and the switch to the masked loop, against the CPU oracle.

The shapes come from tests/speculative_shapes.py (tests/test_speculative_shapes_cpu.py holds the planner's proof that they speculate): about
16 000 or 33 000 targets against 66 000 to 90 000 sources, splits of at least 12 tiles, with three kinds of waves in one launch: regime A (one
repaired tile, goes on speculating), regime B (repairs until it runs masked), regime C (no coincident pair: unmasked throughout).

  one density        eval_kernel<Ker, R, MODE, T>: 10 kernels x (fp64 modes 0, 1, 2; fp32 modes 0, 1) x T in (1, 2)
  several densities  eval_multi_kernel<Ker, R, MODE, T, M>: the same modes x nd in (2, 3, 4, 7, 8), i.e. every form M of the launch table, a partly
                     filled form (nact < M: the padded zero densities of a coincident tile are NaN in the unmasked pass) and a second pass

Tolerances are the project's: conftest.tol_for against the oracle (fp32 one density at digits 9: 3e-5 as in test_gpu_fuzz.py); two GPU paths on
all targets 1e-14 (fp64) and 1e-6 (fp32) as in test_gpu_densities.py, and at digits 5 / 10 the mode's oracle tolerance (both sides round their
seeds alike but sum in other groupings).  The same bounds hold on the coincident targets of regimes A and B alone, and one by one: for a single
target the error is measured against the larger of its own value and the RMS value of its regime, because a sum of 10^5 terms of either sign
can cancel to a value far below the terms whose rounding it carries."""
import numpy as np
import pytest

import sctl_amd
import speculative_shapes as S
from conftest import ctx_for, rel_l2, tol_for

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float64, np.float32]
_ORACLE = {}


def _tol_oracle(dt, digits, nd):
    if dt == np.float64:
        return tol_for(dict(digits=digits, dtype="f64"))
    return 3e-5 if (nd == 1 and digits == 9) else tol_for(dict(digits=-1, dtype="f32"))


def _tol_paths(dt, digits):
    if dt == np.float32:
        return 1e-6
    return 1e-14 if digits < 0 else _tol_oracle(dt, digits, 1)


def _oracle_rows(O, c, rows):
    """Oracle values of density rows `rows` on the subset's targets, fp64 copies of the case's inputs; (len(subset), k1) each.  Shared between
    the cases (digits, nd) and the tests that get the same clouds."""
    if any(k[:2] != (c.name, c.real) for k in _ORACLE):
        _ORACLE.clear()
    f8 = lambda a: None if a is None else a.astype(np.float64)
    k1 = sctl_amd.kernel_info(c.name)["k1"]
    out = []
    for m in rows:
        key = (c.name, c.real, c.Nt, c.Ns, c.trg_per_lane, c.tiles_lo, m)
        if key not in _ORACLE:
            xsel = f8(c.xt.reshape(-1, 3)[c.subset]).ravel().copy()
            _ORACLE[key] = O.eval(c.name, xsel, f8(c.xs), f8(c.xn), f8(c.F[m]), ctx=ctx_for(c.name)).reshape(-1, k1)
        out.append(_ORACLE[key])
    return out


def _regimes(c):
    return (("A", c.a_trg), ("B", c.b_trg), ("C", c.c_sel), ("subset", c.subset))


def _check_oracle(c, got, ref, tol, what):
    """got: (Nt, k1) result without its prefill; ref: (len(subset), k1) oracle values.  rel-L2 on the subset and on each regime alone; every
    coincident target finite and within tol of the oracle on its own."""
    pos = {int(t): i for i, t in enumerate(c.subset)}
    for tag, idx in _regimes(c):
        r = ref[[pos[int(t)] for t in idx]]
        g = got[idx]
        assert np.all(np.isfinite(g)), (what, tag)
        err = rel_l2(g, r)
        print("%s: regime %s vs oracle %.3e (tol %.1e)" % (what, tag, err, tol))
        assert err <= tol, (what, tag, err, tol)
        if tag in ("A", "B"):
            rms = np.sqrt((r.astype(np.float64) ** 2).sum(1).mean())
            per = np.linalg.norm(g.astype(np.float64) - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), rms)
            print("%s: regime %s worst single target %.3e" % (what, tag, per.max()))
            assert per.max() <= tol, (what, tag, int(idx[per.argmax()]), per.max(), tol)


def _check_paths(c, a, b, tol, what):
    """Two GPU results (Nt, k1) of the same problem: rel-L2 on all targets and on regimes A and B alone."""
    for tag, idx in (("all", slice(None)), ("A", c.a_trg), ("B", c.b_trg)):
        err = rel_l2(a[idx], b[idx])
        print("%s: %s targets, two GPU paths %.3e (tol %.1e)" % (what, tag, err, tol))
        assert err <= tol, (what, tag, err, tol)


@pytest.mark.parametrize("dt", PRECISIONS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_one_density_matches_the_oracle_and_its_two_target_halves(O, name, dt):
    k1, ctx = sctl_amd.kernel_info(name)["k1"], ctx_for(name)
    for digits, t in S.one_density_cases(name, dt):
        c = S.build_case(name, dt, digits, t)
        what = "%s %s digits %d, %d per lane, %d x %d" % (name, np.dtype(dt).name, digits, t, c.Nt, c.Ns)
        f, v0 = c.F[0].copy(), c.v0[0]
        u = sctl_amd.eval_host(name, c.xt, c.xs, c.xn, f, v_trg=v0.copy(), digits=digits, ctx=ctx)
        assert u.dtype == dt and np.all(np.isfinite(u)), what
        # the same problem as two target halves: one target per lane and other source splits, every target a full lane's own
        h = c.Nt // 2
        halves = np.concatenate([sctl_amd.eval_host(name, c.xt[:h * 3].copy(), c.xs, c.xn, f, v_trg=v0[:h * k1].copy(), digits=digits, ctx=ctx),
                                 sctl_amd.eval_host(name, c.xt[h * 3:].copy(), c.xs, c.xn, f, v_trg=v0[h * k1:].copy(), digits=digits, ctx=ctx)])
        assert np.all(np.isfinite(halves)), what
        _check_paths(c, u.reshape(-1, k1), halves.reshape(-1, k1), _tol_paths(dt, digits), what)
        _check_oracle(c, (u - v0).reshape(-1, k1), _oracle_rows(O, c, [0])[0], _tol_oracle(dt, digits, 1), what)


@pytest.mark.parametrize("dt", PRECISIONS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_several_densities_match_the_oracle_and_the_single_density_entry(O, name, dt):
    k1, ctx = sctl_amd.kernel_info(name)["k1"], ctx_for(name)
    single = {}                                               # eval_host of a row, per (digits, sizes): the nd cases of one size share them
    for digits, nd in S.several_density_cases(name, dt):
        c = S.build_case(name, dt, digits, S.densities_trg_per_lane(name, dt, digits, nd), nd)
        what = "%s %s digits %d, %d densities (%d per pass, %d per lane), %d x %d" % (name, np.dtype(dt).name, digits, nd, c.plan["densities_per_pass"],
                                                                                     c.trg_per_lane, c.Nt, c.Ns)
        F, V0 = c.F[:nd].copy(), c.v0[:nd]
        U = sctl_amd.eval_densities_host(name, c.xt, c.xs, c.xn, F, V_trg=V0.copy(), digits=digits, ctx=ctx)
        assert U.shape == (nd, c.Nt * k1) and U.dtype == dt and np.all(np.isfinite(U)), what
        refs = _oracle_rows(O, c, range(nd))
        for m in range(nd):
            key = (digits, c.Nt, c.Ns, m)
            if key not in single:
                single[key] = sctl_amd.eval_host(name, c.xt, c.xs, c.xn, F[m].copy(), v_trg=V0[m].copy(), digits=digits, ctx=ctx)
            _check_paths(c, U[m].reshape(-1, k1), single[key].reshape(-1, k1), _tol_paths(dt, digits), "%s, row %d" % (what, m))
            _check_oracle(c, (U[m] - V0[m]).reshape(-1, k1), refs[m], _tol_oracle(dt, digits, nd), "%s, row %d" % (what, m))


@pytest.mark.parametrize("dt", PRECISIONS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_two_runs_agree_bit_for_bit(name, dt):
    """one case of each evaluator per (kernel, precision): unmasked tiles, repaired tiles, the masked loop and the fixed-order reduction of the splits"""
    ctx = ctx_for(name)
    bits = np.int64 if dt == np.float64 else np.int32
    c = S.build_case(name, dt, -1, 2)
    a, b = (sctl_amd.eval_host(name, c.xt, c.xs, c.xn, c.F[0].copy(), v_trg=c.v0[0].copy(), ctx=ctx) for _ in range(2))
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(bits), b.view(bits)), name
    c = S.build_case(name, dt, -1, S.densities_trg_per_lane(name, dt, -1, 3), 3)
    a, b = (sctl_amd.eval_densities_host(name, c.xt, c.xs, c.xn, c.F[:3].copy(), ctx=ctx) for _ in range(2))
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(bits), b.view(bits)), name
