"""The transposed near-field application (sctl_amd_near_apply_transpose_device, G += N^T W) against the forward single-density application
(sctl_amd_near_apply_device, U += N F) of the same library build, same process, same operator: the operators of tools/time_near_densities.py
in fp64 and fp32, and a fourth made of few very wide rows (3 x 2100 blocks), which the transposed kernel cuts over the waves of a workgroup.
Byte model of one application, either direction: sizeof(K_near) + (density + U_near / Wn written and read back + potential read and written);
"rate" is that over the measured time.  Times are HIP events around `reps` applications on torch's current stream, after one warm-up application.
usage: time_near_transpose.py [Nelem nodes_per_elem near_targets_per_elem k0 k1 [f64|f32]]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import sctl_amd

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
    F = torch.randn(op.density_len, dtype=tdt, device="cuda"); U = torch.zeros(op.potential_len, dtype=tdt, device="cuda")
    W = torch.randn(op.potential_len, dtype=tdt, device="cuda"); G = torch.zeros(op.density_len, dtype=tdt, device="cuda")
    ms_fwd = timed(lambda: op.apply_device(F, U), reps)
    ms_t = timed(lambda: op.apply_transpose_device(W, G), reps)
    ms_fwd2 = timed(lambda: op.apply_device(F, U), reps)        # the forward again, after the transposed: drift of the box within the run
    model = op.operator_bytes + (2 * op.density_len + 2 * op.near_entries * k1 + 2 * op.potential_len) * rs
    print("Nelem %6d  block %3d x %4d  %s  K_near %7.1f MB  model %7.1f MB   forward %8.3f ms %7.1f GB/s (again %8.3f ms)   transposed %8.3f ms %7.1f GB/s   transposed / forward %.3f" % (
        nelem, nds * k0, near * k1, np.dtype(dtype).name, op.operator_bytes / 1e6, model / 1e6, ms_fwd, model / ms_fwd / 1e6, ms_fwd2, ms_t, model / ms_t / 1e6,
        ms_t / min(ms_fwd, ms_fwd2)), flush=True)
    op.close()

if len(sys.argv) > 5:
    run(*[int(a) for a in sys.argv[1:6]], dtype=np.float32 if sys.argv[6:7] == ["f32"] else np.float64)
else:
    for dt in (np.float64, np.float32):
        run(2048, 48, 400, 3, 3, dt)      # Stokes-like: 144 x 1200 blocks (the bench's operator in fp64: 2.8 GB)
        run(8192, 24, 200, 1, 1, dt)      # Laplace-like: 24 x 200 blocks
        run(20000, 16, 30, 1, 1, dt)      # many small blocks
        run(40000, 1, 700, 3, 3, dt)      # few very wide rows: 3 x 2100 blocks
