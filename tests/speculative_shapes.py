"""Shapes at which the all-pairs evaluators (eval_kernel, eval_multi_kernel) run their unmasked pass, repair a tile and give up speculating.

A workgroup evaluates a source tile without the r = 0 mask only when its source split holds at least 4 tiles of 256 sources; a wave whose tile
sums come out non-finite runs that tile again masked, and after `repairs * 8 > tiles of the split` it runs masked from then on.  For small
problems the planner cuts the sources into one tile per split, so nothing of this runs.  build_case() asks the planner itself (sctl_amd.plan,
sctl_amd.plan_densities: no GPU needed) for the smallest ragged problem whose splits hold at least MIN_TILES tiles, and plants coincident
(target, source) pairs so that one launch has three kinds of waves:

  regime A  the four waves of the first target workgroup: N_A of their targets are copies of sources of ONE tile of split 0 -> one repair per
            wave, which then goes on speculating (1 * 8 <= tiles);
  regime B  the four waves of the second workgroup: N_B targets are copies of sources spread over every tile of split 0 -> each wave repairs
            tile after tile until repairs * 8 > tiles and finishes in the masked loop;
  regime C  every other wave: no coincident pair, unmasked throughout.

Every other (workgroup, split) of the launch is purely unmasked as well.  The clouds of a case depend on (kernel, precision, Nt, Ns) only, so
cases that differ in `digits` or `nd` but get the same sizes share their inputs (and a test can share their oracle values)."""
from collections import namedtuple

import numpy as np

import sctl_amd

TILE = 256           # sources per LDS tile == lanes per workgroup (eval_kernel.hpp: kTile, kBlock)
WAVE = 64
MIN_TILES = 12       # per split: one repair leaves a wave speculating (1 * 8 <= 12), two or more flip it (2 * 8 > 12 .. )
N_A, N_B = 40, 200   # coincident targets of regimes A and B
N_ENDS = 64          # first and last targets in the oracle subset
SUBSET_MAX = 500     # (the issue allows 600; the CPU oracle's time goes with it)
MAX_ND = 8           # density rows generated per case: a case of nd densities uses the first nd
NT_START = 16384     # per target-per-lane: 64 full workgroups, + NT_RAGGED targets in a 65th
NT_RAGGED = 77
NS_START = 65700     # ragged, not a multiple of 256
NS_STEP = 8 * TILE + 3
NS_MAX = 400000

DIGITS = {np.float64: (5, 10, -1), np.float32: (-1, 9)}      # modes 0, 1, 2 and 0, 1 (capi.hip: mode_for)
ND_VALUES = (2, 3, 4, 7, 8)

Case = namedtuple("Case", "name dt real digits nd trg_per_lane Nt Ns plan src_splits tiles_lo tiles_hi xt xs xn F v0 "
                          "a_trg a_src b_trg b_src c_sel subset")


def real_of(dt):
    return 0 if np.dtype(dt) == np.float64 else 1


def _plan(name, real, nd, Nt, Ns, digits):
    if nd == 1:
        return sctl_amd.plan(name, real, Nt, Ns, digits)
    pl = sctl_amd.plan_densities(name, real, nd, Nt, Ns, digits)
    pl["path"] = "exact"                                      # the several-densities entry has no other path
    return pl


def split_tiles(Ns, pl, nd):
    """(lower, upper) bound of the tiles per source split.  One density: both are ceil(ceil(Ns/256) / src_splits), because the planner's
    src_splits is ceil(tiles / tiles per split) of the tiles per split it chose.  Several densities: the planner reports the splits rounded up
    to eights (from 8 on), so the count it cut the sources into lies in [src_splits - 7, src_splits]."""
    ntile = -(-Ns // TILE)
    s = pl["src_splits"]
    lo = -(-ntile // s)
    hi = lo if (nd == 1 or s < 8) else -(-ntile // (s - 7))
    return lo, hi


def sizes(name, dt, digits, trg_per_lane, nd=1):
    """Smallest (Nt, Ns, plan) from the starting points at which the conditions of tests/test_speculative_shapes_cpu.py hold."""
    real = real_of(dt)
    Nt = NT_START * trg_per_lane + NT_RAGGED
    for Ns in range(NS_START, NS_MAX, NS_STEP):
        if Ns % TILE == 0:
            continue
        pl = _plan(name, real, nd, Nt, Ns, digits)
        if pl["trg_per_lane"] != trg_per_lane:
            raise ValueError("%s: the planner gives %d targets per lane at Nt = %d, not %d" % (name, pl["trg_per_lane"], Nt, trg_per_lane))
        if pl["path"] == "exact" and pl["src_splits"] >= 2 and split_tiles(Ns, pl, nd)[0] >= MIN_TILES:
            return Nt, Ns, pl
    raise ValueError("%s: no source count below %d gives %d tiles per split" % (name, NS_MAX, MIN_TILES))


def densities_trg_per_lane(name, dt, digits, nd):
    """Targets per lane of the form that takes nd densities (fixed per form in the launch table, whatever the sizes)."""
    return sctl_amd.plan_densities(name, real_of(dt), nd, NT_START + NT_RAGGED, NS_START, digits)["trg_per_lane"]


def wave_of(t, trg_per_lane):
    """(workgroup, wave) that owns target t: a lane holds the targets tbase + j * 256 + tid, j < trg_per_lane."""
    per_wg = TILE * trg_per_lane
    return t // per_wg, (t % per_wg) % TILE // WAVE


def _spread_over_waves(wg, n, trg_per_lane):
    """n targets of workgroup wg, dealt to its four waves in turn and, within a wave, to its trg_per_lane target slots in turn."""
    out = []
    for i in range(n):
        wave, k = i % 4, i // 4
        j, lane = k % trg_per_lane, k // trg_per_lane
        assert lane < WAVE
        out.append(wg * TILE * trg_per_lane + j * TILE + wave * WAVE + lane)
    return np.array(out, dtype=np.int64)


_CLOUDS = {}


def _cloud(name, dt, Nt, Ns):
    key = (name, np.dtype(dt).name, Nt, Ns)
    if key not in _CLOUDS:
        if any(k[:2] != key[:2] for k in _CLOUDS):            # the sizes of one (kernel, precision) at a time: 8 density rows of a Stokes kernel are 25 MB
            _CLOUDS.clear()
        info = sctl_amd.kernel_info(name)
        rng = np.random.default_rng([sctl_amd.KERNEL_NAMES.index(name), real_of(dt), Nt, Ns])
        xt, xs = rng.random(Nt * 3).astype(dt), rng.random(Ns * 3).astype(dt)
        xn = (rng.random(Ns * info["nd"]) - 0.5).astype(dt) if info["nd"] else None
        F = (rng.random((MAX_ND, Ns * info["k0"])) - 0.5).astype(dt)
        v0 = (rng.random((MAX_ND, Nt * info["k1"])) - 0.5).astype(dt)
        _CLOUDS[key] = (xt, xs, xn, F, v0, rng.integers(1 << 30))
    return _CLOUDS[key]


def build_case(name, dt, digits, trg_per_lane, nd=1):
    """The case of (kernel, precision, digits, targets per lane[, densities]): sizes from the planner, clouds in [0,1)^3 with the coincident
    pairs of regimes A and B planted, and the oracle subset.  xt, xs, xn are flat arrays of dtype dt; F is (MAX_ND, Ns*SrcDim) and v0 (a prefill
    of the result) is (MAX_ND, Nt*TrgDim): one density uses row 0, nd densities the first nd rows.  The arrays are shared between cases of one
    size and must not be written to."""
    Nt, Ns, pl = sizes(name, dt, digits, trg_per_lane, nd)
    lo, hi = split_tiles(Ns, pl, nd)
    xt, xs, xn, F, v0, seed = _cloud(name, dt, Nt, Ns)
    rng = np.random.default_rng(seed)
    # regime A: sources of one tile in the middle of split 0; regime B: target i meets tile (i // 4) % lo, so each wave of the workgroup has
    # a coincident source in every tile of the split (50 targets per wave, tiles visited in turn)
    a_trg = _spread_over_waves(0, N_A, trg_per_lane)
    a_src = (lo // 2) * TILE + rng.choice(TILE, N_A, replace=False)
    b_trg = _spread_over_waves(1, N_B, trg_per_lane)
    b_tile = (np.arange(N_B) // 4) % lo
    b_src = b_tile * TILE + rng.choice(TILE, N_B, replace=False)
    xt = xt.copy()
    X = xt.reshape(Nt, 3)
    X[a_trg] = xs.reshape(Ns, 3)[a_src]
    X[b_trg] = xs.reshape(Ns, 3)[b_src]
    fixed = np.unique(np.concatenate([a_trg, b_trg, np.arange(N_ENDS), np.arange(Nt - N_ENDS, Nt)]))
    c_all = np.arange(2 * TILE * trg_per_lane, Nt - N_ENDS)  # regime C outside the two ends
    c_sel = np.sort(rng.choice(c_all, SUBSET_MAX - fixed.size, replace=False))
    subset = np.unique(np.concatenate([fixed, c_sel]))
    return Case(name, dt, real_of(dt), digits, nd, trg_per_lane, Nt, Ns, pl, pl["src_splits"], lo, hi, xt, xs, xn, F, v0,
                a_trg, a_src, b_trg, b_src, c_sel, subset)


def one_density_cases(name, dt):
    return [(digits, t) for digits in DIGITS[dt] for t in (1, 2)]


def several_density_cases(name, dt):
    return [(digits, nd) for digits in DIGITS[dt] for nd in ND_VALUES]
