"""The geometry gradients over P2P lists (sctl_amd_lists_eval_grad_device: each side alone, and both) against the forward and the transposed list entries
(sctl_amd_lists_eval_device, sctl_amd_lists_eval_transpose_device, unchanged) on the same plan in one process, alternating: 2^21 uniform points in g^3
boxes, every box against its 27 neighbours, targets == sources (one device array), at ~8, ~24, ~64 and ~512 points per leaf; Laplace3D-FxU,
Laplace3D-DxU and Stokes3D-FxU in fp64 at full precision.  Device arrays, times by device events around work on torch's current stream, best of
LISTS_REPS alternations.
"cyc/pair" is wave-cycles per pair: time x 2.36 GHz x 1024 SIMDs / (pairs / 64).  "ratio" is gradient time / forward list time, "slots" the ratio of
the issue slots per pair of pair_g to pair's (DESIGN.md §4.10's table: fp64, full precision).
    python tools/time_lists_grad.py [out.txt]      LISTS_GRIDS=64,44,32,16  LISTS_CONFIGS=Laplace3D-FxU:f64,..."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sctl_amd
from sctl_amd.lists import grid_neighbour_lists

N = 1 << 21
GRIDS = [int(g) for g in os.environ.get("LISTS_GRIDS", "64,44,32,16").split(",")]
CONFIGS = [c.split(":") for c in os.environ.get("LISTS_CONFIGS", "Laplace3D-FxU:f64,Laplace3D-DxU:f64,Stokes3D-FxU:f64").split(",")]
REPS = int(os.environ.get("LISTS_REPS", "3"))
# issue slots per pair (forward, target-owned gradient, source-owned gradient), DESIGN.md §4.10
SLOTS = {"Laplace3D-FxU": (15, 22, 22), "Laplace3D-DxU": (19, 31, 34), "Laplace3D-FxdU": (19, 30, 30), "Stokes3D-FxU": (25, 41.5, 41.5),
         "Stokes3D-DxU": (27, 48.5, 52.5), "Stokes3D-FxT": (29, 49.5, 55.5), "Stokes3D-FSxU": (25, 41.5, 41.5), "Stokes3D-FxUP": (26, 41.5, 41.5),
         "Laplace3D-FDxUdU": (29, 55.5, 62.5), "Helmholtz3D-FxU": (43.5, 55, 55)}
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


say("%-14s %-4s %5s %8s | %8s %8s %8s %8s %8s | %15s %15s %7s | %7s %7s %7s %7s" % (
    "kernel", "real", "leaf", "items", "fwd ms", "transp", "g trg", "g src", "g both", "ratio trg:slots", "ratio src:slots", "both", "cyc F", "cyc T", "cyc gt", "cyc gs"))
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
        plan = sctl_amd.ListsPlan(name, dt, *lists, N, N, ctx=np.array([3.0, 0.2]) if name.startswith("Helmholtz") else None, directions="both")
        dx = torch.from_numpy(x.astype(dt)).cuda()
        dn = torch.from_numpy((rng.random(N * info["nd"]) - 0.5).astype(dt)).cuda()
        f = torch.from_numpy((rng.random(N * info["k0"]) - 0.5).astype(dt)).cuda()
        w = torch.from_numpy((rng.random(N * info["k1"]) - 0.5).astype(dt)).cuda()
        u = torch.zeros(N * info["k1"], dtype=tdt, device="cuda")
        g = torch.zeros(N * info["k0"], dtype=tdt, device="cuda")
        gt, gs, gn = (torch.zeros(N * 3, dtype=tdt, device="cuda") for _ in range(3))
        src_want = ["src", "nrm"] if info["nd"] else ["src"]
        runs = [lambda: plan.eval_device(dx, dx, dn, f, v_trg=u),
                lambda: plan.eval_transpose_device(dx, dx, dn, w, g_src=g),
                lambda: plan.eval_grad_device(dx, dx, dn, f, w, g_trg=gt, want=["trg"]),
                lambda: plan.eval_grad_device(dx, dx, dn, f, w, g_src=gs, g_nrm=gn, want=src_want),
                lambda: plan.eval_grad_device(dx, dx, dn, f, w, g_trg=gt, g_src=gs, g_nrm=gn)]
        for fn in runs:
            fn()
        torch.cuda.synchronize()
        t = [[] for _ in runs]
        for _ in range(REPS):
            for i, fn in enumerate(runs):
                t[i].append(timed(fn))
        tf, tt, t0, t1, tb = (min(v) for v in t)
        cyc = lambda ms: ms * 1e-3 * 2.36e9 * 1024 / (plan.pairs / 64)
        s = SLOTS[name]
        say("%-14s %-4s %5d %8d | %8.2f %8.2f %8.2f %8.2f %8.2f | %7.3f:%7.3f %7.3f:%7.3f %7.3f | %7.1f %7.1f %7.1f %7.1f" % (
            name, real, N // grid ** 3, plan.work_items, tf, tt, t0, t1, tb, t0 / tf, s[1] / s[0], t1 / tf, s[2] / s[0], tb / tf, cyc(tf), cyc(tt), cyc(t0), cyc(t1)))
        plan.close()
        del dx, dn, f, w, u, g, gt, gs, gn
if out:
    out.close()
