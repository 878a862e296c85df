"""The transposed list sum (sctl_amd_lists_eval_transpose_device) against the forward list entry (sctl_amd_lists_eval_device, unchanged) on the same
plan in one process, alternating: 2^21 uniform points in g^3 boxes, every box against its 27 neighbours, targets == sources (one device array), at
~8, ~24, ~64 and ~512 points per leaf; Laplace3D-FxU and Stokes3D-FxU in fp64, and Laplace3D-DxU, whose normal the transposed kernel keeps in
registers.  Device arrays, times by device events around work on torch's current stream, best of LISTS_REPS alternations.
"cyc/pair" is wave-cycles per pair: time x 2.36 GHz x 1024 SIMDs / (pairs / 64).  "ratio" is transposed time / forward time.
    python tools/time_lists_transpose.py [out.txt]      LISTS_GRIDS=64,44,32,16  LISTS_CONFIGS=Laplace3D-FxU:f64,..."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sctl_amd
from sctl_amd.lists import grid_neighbour_lists

N = 1 << 21
GRIDS = [int(g) for g in os.environ.get("LISTS_GRIDS", "64,44,32,16").split(",")]
CONFIGS = [c.split(":") for c in os.environ.get("LISTS_CONFIGS", "Laplace3D-FxU:f64,Stokes3D-FxU:f64,Laplace3D-DxU:f64").split(",")]
REPS = int(os.environ.get("LISTS_REPS", "3"))
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


say("%-14s %-4s %5s %8s %8s %11s %10s %7s %10s %10s" % ("kernel", "real", "leaf", "items", "items T", "forward ms", "transp ms", "ratio", "cyc/pair F", "cyc/pair T"))
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

        def forward():
            plan.eval_device(dx, dx, dn, f, v_trg=u)

        def transpose():
            plan.eval_transpose_device(dx, dx, dn, w, g_src=g)

        forward(); transpose()
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(REPS):
            tf.append(timed(forward))
            tt.append(timed(transpose))
        a, b = min(tf), min(tt)
        cyc = lambda ms: ms * 1e-3 * 2.36e9 * 1024 / (plan.pairs / 64)
        say("%-14s %-4s %5d %8d %8d %11.2f %10.2f %7.3f %10.1f %10.1f" % (name, real, N // grid ** 3, plan.work_items, plan.transpose_info()["work_items"], a, b, b / a,
                                                                      cyc(a), cyc(b)))
        plan.close()
        del dx, dn, f, w, u, g
if out:
    out.close()
