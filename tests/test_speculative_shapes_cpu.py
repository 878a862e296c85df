"""The planner's own word that every case of tests/test_gpu_speculative_pass.py speculates, repairs a tile and flips to the masked loop: the
conditions on the launch plan of each (kernel, precision, digits, targets per lane / densities) case built by tests/speculative_shapes.py, and
the make-up of its three target regimes.  No GPU: sctl_amd.plan and sctl_amd.plan_densities only do the planner's arithmetic."""
import numpy as np
import pytest

import sctl_amd
import speculative_shapes as S

PRECISIONS = [np.float64, np.float32]


def _check_case(c):
    info = sctl_amd.kernel_info(c.name)
    what = (c.name, np.dtype(c.dt).name, c.digits, c.trg_per_lane, c.nd, c.Nt, c.Ns, c.plan)
    # the plan: the exact kernel, the intended targets per lane, splits of at least 12 tiles and at least two of them
    assert c.plan["path"] == "exact" and c.plan["trg_per_lane"] == c.trg_per_lane, what
    chunk = S.TILE * -(-(-(-c.Ns // S.TILE)) // c.plan["src_splits"])
    assert chunk // S.TILE == c.tiles_lo >= 12 and c.plan["src_splits"] >= 2, what
    assert c.tiles_lo <= c.tiles_hi and (c.nd > 1 or c.tiles_lo == c.tiles_hi), what
    # ragged at both ends: the last target workgroup and the last source tile are partly filled
    per_wg = S.TILE * c.trg_per_lane
    assert 0 < c.Nt % per_wg < per_wg and c.Nt // per_wg >= 3, what
    assert 0 < c.Ns % S.TILE, what
    assert c.plan["workgroups"] == -(-c.Nt // per_wg) * c.plan["src_splits"], what
    # arrays
    assert c.xt.dtype == c.dt and c.xt.size == c.Nt * 3 and c.xs.size == c.Ns * 3
    assert c.F.shape == (S.MAX_ND, c.Ns * info["k0"]) and c.v0.shape == (S.MAX_ND, c.Nt * info["k1"]) and c.nd <= S.MAX_ND
    assert (c.xn is None) == (info["nd"] == 0)
    Xt, Xs = c.xt.reshape(-1, 3), c.xs.reshape(-1, 3)
    # regime A: 40 targets on all four waves of workgroup 0, copies of sources of ONE tile that lies in split 0 whatever the split count was
    assert c.a_trg.size == 40 == np.unique(c.a_trg).size
    assert {S.wave_of(int(t), c.trg_per_lane) for t in c.a_trg} == {(0, w) for w in range(4)}
    assert np.array_equal(Xt[c.a_trg], Xs[c.a_src]) and np.unique(c.a_src // S.TILE).size == 1 and c.a_src.max() < c.tiles_lo * S.TILE
    assert 1 * 8 <= c.tiles_lo                                # one repair: the wave goes on speculating
    # regime B: 200 targets on all four waves of workgroup 1; EACH wave meets sources in at least half of the split's tiles, and in more
    # than an eighth of them even at the upper bound of the split's length: it crosses repairs * 8 > tiles
    assert c.b_trg.size == 200 == np.unique(c.b_trg).size and c.b_src.max() < c.tiles_lo * S.TILE
    assert np.array_equal(Xt[c.b_trg], Xs[c.b_src])
    waves = np.array([S.wave_of(int(t), c.trg_per_lane) for t in c.b_trg])
    assert np.all(waves[:, 0] == 1)
    for w in range(4):
        tiles = np.unique(c.b_src[waves[:, 1] == w] // S.TILE)
        assert tiles.size * 2 >= c.tiles_hi and tiles.size * 8 > c.tiles_hi and tiles.size >= 2, (what, w, tiles)
    # regime C: no other target coincides with a source (exact equality of all three coordinates)
    planted = np.zeros(c.Nt, dtype=bool)
    planted[c.a_trg] = planted[c.b_trg] = True
    src_rows = {r.tobytes() for r in Xs}
    assert not any(Xt[t].tobytes() in src_rows for t in np.flatnonzero(~planted)), what
    # the oracle subset: at most 600, all of A and B, both ends, and targets of regime C away from them
    sub = set(c.subset.tolist())
    assert len(sub) == c.subset.size <= 600 and c.subset.min() == 0 and c.subset.max() == c.Nt - 1
    assert set(c.a_trg.tolist()) <= sub and set(c.b_trg.tolist()) <= sub
    assert set(range(64)) <= sub and set(range(c.Nt - 64, c.Nt)) <= sub
    wg = np.array([S.wave_of(int(t), c.trg_per_lane)[0] for t in c.c_sel])
    assert c.c_sel.size >= 100 and set(c.c_sel.tolist()) <= sub and np.all(wg >= 2) and not planted[c.c_sel].any()
    assert np.unique(wg).size >= 30                           # spread over the launch, the partly filled last workgroup included (the last 64)


@pytest.mark.parametrize("dt", PRECISIONS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_one_density_cases_speculate_repair_and_flip(name, dt):
    cases = S.one_density_cases(name, dt)
    assert sorted({t for _, t in cases}) == [1, 2]
    for digits, t in cases:
        c = S.build_case(name, dt, digits, t)
        assert c.nd == 1
        _check_case(c)
        # the two-halves cross-check of the GPU test runs another plan: one target per lane, fewer than 32768 targets each
        h = c.Nt // 2
        for n in (h, c.Nt - h):
            ph = sctl_amd.plan(name, c.real, n, c.Ns, digits)
            assert n < 32768 and ph["trg_per_lane"] == 1 and ph["path"] == "exact", ph
            assert (ph["trg_per_lane"], ph["src_splits"]) != (c.trg_per_lane, c.src_splits), (ph, c.plan)


@pytest.mark.parametrize("dt", PRECISIONS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", sctl_amd.KERNEL_NAMES)
def test_several_densities_cases_speculate_repair_and_flip(name, dt):
    forms = set()
    for digits, nd in S.several_density_cases(name, dt):
        t = S.densities_trg_per_lane(name, dt, digits, nd)
        c = S.build_case(name, dt, digits, t, nd)
        _check_case(c)
        pl = c.plan
        m_max = sctl_amd.plan_densities(name, c.real, 64, c.Nt, c.Ns, digits)["densities_per_pass"]
        assert pl["densities_per_pass"] == (m_max if nd >= m_max else min(m for m in (2, 4, 8) if m >= nd)), (name, nd, pl)
        assert pl["passes"] == -(-nd // m_max)
        # nd <= 8: every pass of the call runs the first pass's form, so its plan is the plan of all of them
        assert pl["passes"] == 1 or nd - m_max > m_max // 2, (name, nd, pl)
        forms.add((pl["densities_per_pass"], nd % pl["densities_per_pass"] != 0, pl["passes"] > 1))
    widths = {m for m, _, _ in forms}
    assert {2, 4} <= widths                                   # every form of the kernel's launch table ...
    assert 8 in widths or sctl_amd.plan_densities(name, 0, 64, 1 << 14, 1 << 14)["densities_per_pass"] == 4
    assert any(partly for _, partly, _ in forms)              # ... a partly filled form (nact < M) ...
    assert 8 in widths or any(second for _, _, second in forms)   # ... and, where the widest form has 4 densities, a second pass

