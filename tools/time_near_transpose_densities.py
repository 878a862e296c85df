"""Several weight vectors through the transposed near-field application (sctl_amd_near_apply_transpose_densities_device, G[m] += N^T W[m]) against as
many calls of the single-vector entry (sctl_amd_near_apply_transpose_device) in the same process on the same operator: the four operators of
tools/time_near_transpose.py in fp64 and fp32, nd = 2, 4, 8, 16.  The two sides alternate; a figure is the median of nine HIP-event times of one
several-vectors call (or of its nd single calls) on torch's current stream, after a warm-up of both, and "spread" is (max - min) / median of the nine.
"vs one" is the several-vectors call over ONE single call.
usage: time_near_transpose_densities.py [Nelem nodes_per_elem near_targets_per_elem k0 k1 [f64|f32]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import sctl_amd

def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)

def run(nelem, nds, near, k0, k1, dtype=np.float64, rounds=9):
    rng = np.random.default_rng(0)
    nds_a = np.full(nelem, nds, dtype=np.int64); near_a = np.full(nelem, near, dtype=np.int64)
    n_near = nelem * near
    ntrg = max(1, n_near // 8)                                  # every target is near ~8 elements
    K = rng.standard_normal(nelem * nds * k0 * near * k1, dtype=np.float32 if dtype == np.float32 else np.float64)
    trg = rng.integers(0, ntrg, n_near)
    order = np.argsort(trg, kind="stable"); cnt = np.bincount(trg, minlength=ntrg); dsp = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    op = sctl_amd.NearOp(k0, k1, nds_a, near_a, K, order, cnt, dsp)
    del K
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for nd in (2, 4, 8, 16):
        W = torch.randn((nd, op.potential_len), dtype=tdt, device="cuda"); G = torch.zeros((nd, op.density_len), dtype=tdt, device="cuda")
        multi = lambda: op.apply_transpose_densities_device(W, G)
        def singles():
            for m in range(nd): op.apply_transpose_device(W[m], G[m])
        multi(); singles(); torch.cuda.synchronize()
        tm, ts, t1 = [], [], []
        for _ in range(rounds):
            tm.append(once(multi)); ts.append(once(singles)); t1.append(once(lambda: op.apply_transpose_device(W[0], G[0])))
        med = lambda t: float(np.median(t))
        spr = lambda t: (max(t) - min(t)) / med(t)
        print("Nelem %6d  block %3d x %4d  %s  K_near %7.1f MB  nd %2d   several %8.3f ms (spread %4.1f %%)   %2d single calls %8.3f ms (spread %4.1f %%)   ratio %.3f   vs one %.2f" % (
            nelem, nds * k0, near * k1, np.dtype(dtype).name, op.operator_bytes / 1e6, nd, med(tm), 100 * spr(tm), nd, med(ts), 100 * spr(ts), med(tm) / med(ts),
            med(tm) / med(t1)), flush=True)
    op.close()

if len(sys.argv) > 5:
    run(*[int(a) for a in sys.argv[1:6]], dtype=np.float32 if sys.argv[6:7] == ["f32"] else np.float64)
else:
    for dt in (np.float64, np.float32):
        run(2048, 48, 400, 3, 3, dt)      # Stokes-like: 144 x 1200 blocks (the bench's operator in fp64: 2.8 GB)
        run(8192, 24, 200, 1, 1, dt)      # Laplace-like: 24 x 200 blocks
        run(20000, 16, 30, 1, 1, dt)      # many small blocks
        run(40000, 1, 700, 3, 3, dt)      # few very wide rows: 3 x 2100 blocks
