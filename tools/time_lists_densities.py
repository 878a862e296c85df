"""Several densities over the P2P lists (sctl_amd_lists_eval_densities_device) against nd calls of the single-density list entry
(sctl_amd_lists_eval_device, unchanged: the path a caller had before) in one process, alternating: 2^21 uniform points in g^3 boxes, every box
against its 27 neighbours, targets == sources, at ~8, ~24, ~64 and ~512 points per leaf; Laplace3D-FxU and Stokes3D-FxU in fp64, Laplace3D-FxU
in fp32; nd = 2, 4, 8, 16.  Device arrays, times by device events around work on torch's current stream; as in
tools/time_lists_transpose_densities.py, the MEDIAN of LISTS_REPS (nine) alternating samples, each at least LISTS_MIN_MS (50 ms) of back-to-back
calls, and the spread (max - min) / median of each side.
"cyc/pair" is wave-cycles per geometry pair: time x 2.36 GHz x 1024 SIMDs / (passes x pairs / 64), passes as the call ran them (a pass on
the single-density kernel counts as one).  "ratio" is several-densities time / nd single calls: below 1 the new entry wins.
    python tools/time_lists_densities.py [out.txt]      LISTS_GRIDS=64,44,32,16  LISTS_CONFIGS=Laplace3D-FxU:f64,...  LISTS_NDS=2,4,8,16"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sctl_amd
from sctl_amd.lists import grid_neighbour_lists

N = 1 << 21
GRIDS = [int(g) for g in os.environ.get("LISTS_GRIDS", "64,44,32,16").split(",")]
CONFIGS = [c.split(":") for c in os.environ.get("LISTS_CONFIGS", "Laplace3D-FxU:f64,Stokes3D-FxU:f64,Laplace3D-FxU:f32").split(",")]
NDS = [int(n) for n in os.environ.get("LISTS_NDS", "2,4,8,16").split(",")]
REPS = int(os.environ.get("LISTS_REPS", "9"))
MIN_MS = float(os.environ.get("LISTS_MIN_MS", "50"))
# widest several-densities list form per (kernel, precision): DESIGN.md §4.6
FP64_UP_TO_8 = ("Laplace3D-FxU", "Laplace3D-DxU", "Laplace3D-FxdU")        # the other kernels: 4 in fp64; every kernel 8 in fp32
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def passes_of(nd, m_max):
    p, left = 0, nd
    while left > 0:
        left -= min(left, m_max)
        p += 1
    return p


def stats(ts):
    med = float(np.median(ts))
    return med, (max(ts) - min(ts)) / med


say("%-17s %-4s %5s %3s %10s %7s %10s %7s %7s %9s" % ("kernel", "real", "leaf", "nd", "multi ms", "spread", "nd x 1 ms", "spread", "ratio", "cyc/pair"))
rng = np.random.default_rng(0)
for grid in GRIDS:
    x = rng.random((N, 3))
    box = (np.floor(x[:, 0] * grid) * grid + np.floor(x[:, 1] * grid)) * grid + np.floor(x[:, 2] * grid)
    x = x[np.argsort(box, kind="stable")].ravel().copy()
    counts = np.bincount(box.astype(np.int64), minlength=grid ** 3)
    lists = grid_neighbour_lists(grid, counts, counts)
    for name, real in CONFIGS:
        dt, tdt = (np.float64, torch.float64) if real == "f64" else (np.float32, torch.float32)
        info = sctl_amd.kernel_info(name)
        plan = sctl_amd.ListsPlan(name, dt, *lists, N, N, ctx=np.array([3.0, 0.2]) if name.startswith("Helmholtz") else None)
        dx = torch.from_numpy(x.astype(dt)).cuda()
        dn = torch.from_numpy((rng.random(N * info["nd"]) - 0.5).astype(dt)).cuda()
        for nd in NDS:
            F = torch.from_numpy((rng.random((nd, N * info["k0"])) - 0.5).astype(dt)).cuda()
            U = torch.zeros((nd, N * info["k1"]), dtype=tdt, device="cuda")

            def multi():
                plan.eval_densities_device(dx, dx, dn, F, V_trg=U)

            def singles():
                for m in range(nd):
                    plan.eval_device(dx, dx, dn, F[m], v_trg=U[m])

            multi(); singles()
            torch.cuda.synchronize()
            inner = max(1, int(np.ceil(MIN_MS / timed(singles))))      # a sample is at least MIN_MS of work: `inner` calls back to back, per-call time reported
            tm, ts = [], []
            for _ in range(REPS):
                tm.append(timed(lambda: [multi() for _ in range(inner)]) / inner)
                ts.append(timed(lambda: [singles() for _ in range(inner)]) / inner)
            (m, sm), (s, ss) = stats(tm), stats(ts)
            cyc = m * 1e-3 * 2.36e9 * 1024 / (passes_of(nd, 8 if real == "f32" or name in FP64_UP_TO_8 else 4) * plan.pairs / 64)
            say("%-17s %-4s %5d %3d %10.2f %7.3f %10.2f %7.3f %7.3f %9.1f" % (name, real, N // grid ** 3, nd, m, sm, s, ss, m / s, cyc))
            del F, U
        plan.close()
if out:
    out.close()
