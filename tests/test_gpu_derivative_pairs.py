"""The gradient and tangent kernels (eval_grad_*, eval_jvp_*; pair_g and pair_j of include/sctl_amd/device/ukernels.hpp) one pair at a time, on the
device, against long double.

The other GPU tests of these entries compare sums over whole clouds by rel-L2: one close pair owns the norm, so a far pair, a sub-dominant term or
one lane of the unmasked body can be wrong unseen.  Here exactly ONE streamed point is live, every other one carries +0.0 (its density on the
target-owned side, its weight on the source-owned side), so each owner's output is the device's value of one pair; tests/pair_truth.py has the
truth (sympy-differentiated blocks in np.longdouble), the measure q (error over eps_R times the largest component of the majorant, per output
group) and the probe geometry (owners at P + r u, r from 2^-40 (fp64) or 2^-14 (fp32) to 2^10, one owner on P itself, every d = x_trg - x_src and
e = dx_trg - dx_src exact in the working precision, which is how both kernels form them: one subtraction per component).

Bars, none fitted to the device:
  * full precision (digits = -1), both types: per case, output and zone the device's largest q is at most FACTOR = 4 times the largest q that the
    yardstick (the same formula in plain numpy of the working precision, correctly rounded sqrt and divide) has over the same pairs: the project's
    rule for per-pair values (tests/test_independent_math.py: test_hip_fp32_kernel_values_one_pair_at_a_time_against_long_double), which allows
    for an approximate root and more multiplications per power than the formula written out;
  * fp32 at digits = 9 runs the refined root that fp32 at full precision already takes in these forms (rsqrt_grad), and 10 * 10^-9 lies below the
    unit roundoff of fp32 (6e-8), a bar that no fp32 value can meet: it is held to the full-precision bar, and its q eps_R is printed;
  * fp64 at digits = 10 and 5: the project's 10 * 10^-digits on q eps_R, per pair;
  * every probed pair enters the maximum (0 probes are left out); a non-finite value fails; the coincident pair is exactly 0 in every output; owners
    on the dead side of a launch are exactly 0; the live point's own summed gradient is minus the sum of the per-pair ones (1e-12 of the sum of
    magnitudes in fp64).
Every figure is printed before anything is asserted; profiles/r23_derivative_pairs.txt holds the output of a run on an MI355X.  Measured there: the
largest ratio at full precision is 2.98 in fp64 (Helmholtz, k = -3 + 2.5i, g_trg, r >= 2; every other kernel at most 1.8) and 1.80 in fp32 (2.06 at
digits = 9, Helmholtz on its scaled root), 1.63 and 1.51 on the unmasked shape; fp64 at 10 digits is within 2.1e-14 and at 5 digits within 3.8e-7 of
the majorant.  No form needed more than the factor 4."""
import numpy as np
import pytest

import pair_truth as pt
import sctl_amd
from conftest import ctx_for
from grad_truth import HELMHOLTZ_KS
from pair_truth import LD

pytestmark = pytest.mark.gpu

KERNELS = sctl_amd.KERNEL_NAMES
FACTOR = 4.0
MODES = [(np.float64, -1), (np.float64, 10), (np.float64, 5), (np.float32, -1), (np.float32, 9)]
MODE_IDS = ["f64", "f64-d10", "f64-d5", "f32", "f32-d9"]
CASES = [(n, None) for n in KERNELS if not n.startswith("Helmholtz")] + [("Helmholtz3D-FxU", k) for k in HELMHOLTZ_KS]
CASE_IDS = ["%s%s" % (n, "" if k is None else "-k=%g%+gi" % k) for n, k in CASES]
SPEC_OWNERS, SPEC_STREAMED = 20000 + 77, 13 * 4 * 256 + 300        # the unmasked shape of tests/test_gpu_grad.py and tests/test_gpu_jvp.py

_SHARED = {}


def prepared(name, dt, side, slot, k, n_owners=pt.N_OWNERS, n_streamed=pt.N_STREAMED):
    """a launch, its long-double truth and its yardstick, computed once and shared by the accuracy modes; never modified"""
    key = (name, np.dtype(dt).name, side, slot, k, n_owners)
    if key not in _SHARED:
        seed = 1000 * KERNELS.index(name) + 10 * slot + (5 if side == "src" else 0) + (0 if k is None else 1 + HELMHOLTZ_KS.index(k))
        c = pt.launch(name, dt, side, slot, seed, n_owners, n_streamed, k)
        assert c["exact"]
        _SHARED[key] = (c,) + pt.truth_and_yardstick(name, c)
    return _SHARED[key]


def ctx_of(name, k):
    return ctx_for(name) if k is None else np.array(k, dtype=np.float64)


class Table:
    """q of the device and of the yardstick per (output, zone), with where the device's worst pair was"""

    def __init__(self, tag, name, dt, k):
        self.tag, self.name, self.eps, self.k = tag, name, pt.EPS[np.dtype(dt)], k
        self.rows = {}

    def add(self, what, where, c, got, true, maj, yard, groups=None):
        amp = pt.helmholtz_amp(self.k, c["r"]) if self.k is not None else None
        qd = pt.q_of(got, true, maj, self.eps, groups, amp)
        qy = pt.q_of(yard, true, maj, self.eps, groups, amp)
        z = pt.zones_of(c["r"])
        assert qd.shape == qy.shape == z.shape == c["r"].shape          # one q per owner: nothing is left out
        hit = np.flatnonzero(z == -1)
        assert hit.size == 1
        self.rows.setdefault((what, "coincident"), []).append((0.0, float(qd[hit[0]]), where, int(hit[0]), 0.0))
        for j in range(3):
            idx = np.flatnonzero(z == j)
            assert idx.size >= 64
            i = idx[np.argmax(qd[idx])]
            self.rows.setdefault((what, pt.ZONE_NAMES[j]), []).append((float(qy[idx].max()), float(qd[i]), where, int(i), float(c["r"][i])))

    def report(self):
        """print every figure, then return [(what, zone, yardstick q, device q, ratio)]"""
        out = []
        for (what, zone), rows in self.rows.items():
            qy = max(r[0] for r in rows)
            qd, where, i, r = max((r[1], r[2], r[3], r[4]) for r in rows)
            ratio = qd / qy if qy > 0 else (0.0 if qd == 0 else np.inf)
            print("%s | %-5s | %-13s | yardstick q %7.2f | device q %9.3g | ratio %6.2f | q eps %.2e | worst: %s, owner %d, r %.3e"
                  % (self.tag, what, zone, qy, qd, ratio, qd * self.eps, where, i, r))
            out.append((what, zone, qy, qd, ratio))
        return out


def run_launches(name, dt, digits, k, slots, n_owners, n_streamed, table):
    """the target-owned launches (tangent, g_trg) and the source-owned ones (g_src, g_nrm) at every live slot; returns the findings that are not q's"""
    ctx = ctx_of(name, k)
    bad = []
    for side in ("trg", "src"):
        for slot in slots:
            c, tr, ya = prepared(name, dt, side, slot, k, n_owners, n_streamed)
            where = "%s-owned, live slot %d" % ("target" if side == "trg" else "source", slot)
            g_trg, g_src, g_nrm = sctl_amd.eval_grad_host(name, c["xt"], c["xs"], c["xn"], c["f"], c["w"], digits=digits, ctx=ctx)
            assert g_trg.dtype == dt
            g_trg, g_src = g_trg.reshape(-1, 3), g_src.reshape(-1, 3)
            g_nrm = None if g_nrm is None else g_nrm.reshape(-1, 3)
            if side == "trg":
                du = sctl_amd.eval_jvp_host(name, c["xt"], c["xs"], c["xn"], c["f"], d_trg=c["dxt"], d_src=c["dxs"], d_nrm=c["dxn"], digits=digits, ctx=ctx)
                table.add("du", where, c, du.reshape(c["Nt"], -1), tr["du"], tr["maj_du"], ya["du"], pt.tangent_groups(name))
                table.add("g_trg", where, c, g_trg, tr["g_trg"], tr["maj_g"], ya["g_trg"])
                own, dead = (g_src[slot], g_trg), [g_src] + ([g_nrm] if g_nrm is not None else [])
            else:
                table.add("g_src", where, c, g_src, -tr["g_trg"], tr["maj_g"], -ya["g_trg"])
                if g_nrm is not None:
                    table.add("g_nrm", where, c, g_nrm, tr["g_nrm"], tr["maj_n"], ya["g_nrm"])
                own, dead = (g_trg[slot], g_src), [g_trg]
            for a in dead:                                   # the owners whose density or weight is +0.0
                rest = np.delete(a, slot, axis=0)
                if not np.all(rest == 0):
                    bad.append("%s: %d dead owners are not exactly 0" % (where, int((rest != 0).any(axis=1).sum())))
            live_sum, pairs = own
            fin = np.isfinite(pairs).all()
            gap = np.abs(live_sum.astype(LD) + pairs.astype(LD).sum(axis=0)).max() / np.abs(pairs.astype(LD)).sum(axis=0).max() if fin else np.inf
            print("%s | %s: the live point's gradient against minus the sum of the pairs: %.2e of the sum of magnitudes" % (table.tag, where, gap))
            # fp64: 1e-12.  fp32: both sides run the same pair form on the same d, so only the order of the additions differs: n roundings at most
            if not gap <= (1e-12 if dt == np.float64 else pairs.shape[0] * 2.0 ** -24):
                bad.append("%s: live point's gradient off by %.2e" % (where, gap))
    return bad


def judge(rows, bad, dt, digits, eps):
    for what, zone, qy, qd, ratio in rows:
        if zone == "coincident":
            if qd != 0:
                bad.append("%s: the coincident pair is not exactly 0" % what)
        elif not np.isfinite(qd):
            bad.append("%s, %s: a non-finite value" % (what, zone))
        elif dt == np.float64 and digits >= 0:
            if not qd * eps <= 10.0 * 10.0 ** -digits:
                bad.append("%s, %s: %.2e above 10 * 10^-%d" % (what, zone, qd * eps, digits))
        elif not (qy > 0 and qd <= FACTOR * qy):
            bad.append("%s, %s: device q %.3g is %.2f x the yardstick's %.3g (bar %g)" % (what, zone, qd, ratio, qy, FACTOR))
    assert not bad, bad


@pytest.mark.parametrize("dt,digits", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,k", CASES, ids=CASE_IDS)
def test_masked_shape_one_pair_per_owner(name, k, dt, digits):
    """300 owners x 600 streamed points (a full workgroup and a ragged one; tiles of 256, 256 and 88 over several splits, asserted from the plans; always
    masked), the live point in the first and the last lane of a tile, the first lane of the next and the ragged tile: 12 host launches"""
    real = 0 if dt == np.float64 else 1
    assert sctl_amd.plan_jvp(name, real, 300, 600, digits)["splits"] > 1
    assert sctl_amd.plan_grad(name, real, 300, 600, digits)["trg"]["splits"] > 1 and sctl_amd.plan_grad(name, real, 600, 300, digits)["src"]["splits"] > 1
    tag = "%s%s %s digits %d" % (name, "" if k is None else " k=%g%+gi" % k, dt.__name__, digits)
    table = Table(tag, name, dt, k)
    bad = run_launches(name, dt, digits, k, pt.LIVE_SLOTS(pt.N_STREAMED), pt.N_OWNERS, pt.N_STREAMED, table)
    judge(table.report(), bad, dt, digits, table.eps)


def spec_slot(splits):
    """a lane in a middle tile of a middle split, and the tiles per split"""
    tiles = -(-SPEC_STREAMED // 256)
    per = -(-tiles // splits)
    assert per >= 4 and tiles - (splits - 1) * per >= 4, (splits, per)          # tiles run unmasked (test_unmasked_pass_and_repair)
    return ((splits // 2) * per + per // 2) * 256 + 100, per


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", KERNELS)
def test_unmasked_shape_one_pair_per_owner(name, dt):
    """20077 owners x 13612 streamed points at full precision, both orientations of the gradient: every split holds at least four tiles, so they run
    the unmasked body (rsqrt_grad<MODE, false>); the live point sits in a middle tile of a middle split, and the one owner that coincides with it
    sends its workgroup through the compare and the masked re-run of that very tile.  20077 pairs per launch, the rest of the outputs exactly 0."""
    real = 0 if dt == np.float64 else 1
    k = HELMHOLTZ_KS[0] if name.startswith("Helmholtz") else None
    pj = sctl_amd.plan_jvp(name, real, SPEC_OWNERS, SPEC_STREAMED)
    pg = sctl_amd.plan_grad(name, real, SPEC_OWNERS, SPEC_STREAMED)["trg"]
    ps = sctl_amd.plan_grad(name, real, SPEC_STREAMED, SPEC_OWNERS)["src"]
    slot, _ = spec_slot(pg["splits"])
    assert spec_slot(pj["splits"])[0] == slot and spec_slot(ps["splits"])[0] == slot, (pj, pg, ps)
    tag = "%s %s unmasked, splits %d" % (name, dt.__name__, pg["splits"])
    table = Table(tag, name, dt, k)
    bad = run_launches(name, dt, -1, k, (slot,), SPEC_OWNERS, SPEC_STREAMED, table)
    for key in [x for x in _SHARED if x[5] == SPEC_OWNERS]:                       # 20077-pair truths are not worth keeping
        del _SHARED[key]
    judge(table.report(), bad, dt, -1, table.eps)
