"""Several densities through the near-field operator (sctl_amd_near_apply_densities_device) against nd calls of the single-density entry
(sctl_amd_near_apply_device), same process, same operator: the operators of tools/time_near.py in fp64 and fp32, nd = 1, 2, 4, 8, 16.
Byte model of one application: sizeof(K_near) + nd x (density + U_near written and read back + U read and written); "rate" is that
over the measured time.  Times are HIP events around `reps` applications on torch's current stream, after one warm-up application.
usage: time_near_densities.py [Nelem nodes_per_elem near_targets_per_elem k0 k1]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import sctl_amd

NDS = (1, 2, 4, 8, 16)

def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps

def run(nelem, nds, near, k0, k1, dtype=np.float64, reps=5):
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
    rs = np.dtype(dtype).itemsize
    F = torch.randn((max(NDS), op.density_len), dtype=tdt, device="cuda"); U = torch.zeros((max(NDS), op.potential_len), dtype=tdt, device="cuda")
    print("Nelem %d  block %d x %d  %s  K_near %.1f MB  %d targets  work items %d" % (nelem, nds * k0, near * k1, np.dtype(dtype).name, op.operator_bytes / 1e6, ntrg, op.workgroups), flush=True)
    t1 = None
    for nd in NDS:
        def singles():
            for m in range(nd): op.apply_device(F[m], U[m])
        ms_single = timed(singles, reps)
        ms_multi = timed(lambda: op.apply_densities_device(F[:nd], U[:nd]), reps)
        if nd == 1: t1 = ms_single
        model = op.operator_bytes + nd * (op.density_len + 2 * op.near_entries * k1 + 2 * op.potential_len) * rs
        print("  nd %2d   several %8.3f ms   %2d single %8.3f ms   several / nd single %.3f   several / ONE single %.3f   model %7.1f MB  %7.1f GB/s" % (
            nd, ms_multi, nd, ms_single, ms_multi / ms_single, ms_multi / t1, model / 1e6, model / ms_multi / 1e6), flush=True)
    op.close()

if len(sys.argv) > 5:
    run(*[int(a) for a in sys.argv[1:6]])
else:
    for dt in (np.float64, np.float32):
        run(2048, 48, 400, 3, 3, dt)      # Stokes-like: 144 x 1200 blocks (the bench's operator in fp64: 2.8 GB)
        run(8192, 24, 200, 1, 1, dt)      # Laplace-like: 24 x 200 blocks
        run(20000, 16, 30, 1, 1, dt)      # many small blocks
