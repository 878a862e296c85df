#!/usr/bin/env python3
"""Several densities in one pass against nd single-density calls (sctl_amd_eval_densities_device vs sctl_amd_eval_device), nd = 1, 2, 4, 8, 16:

    Laplace3D-FxU   fp64  2^20 x 2^20        Stokes3D-FxU  fp64  2^18 x 2^18
    Helmholtz3D-FxU fp64  2^20 x 2^20        Laplace3D-FxU fp32  2^21 x 2^21

    python tools/time_densities.py [--out profiles/r05_densities.txt]     one child process per case, each under `timeout -k 10 <s>`;
                                                                          stops at the first case that fails and writes what it has
    python tools/time_densities.py --case I                               one case (what the driver runs)

A single-density call's time is the median of 3 runs and "nd single" is nd times it (the nd calls are identical, each a whole launch).  A
multi-density call is warmed up on a small problem with the same nd (same kernels), then timed once (twice under 1 s).  Times are HIP events
around work on torch's current stream.  "cyc/pair" is wave-cycles per geometry pair: time x 2.36 GHz x 1024 SIMDs / (passes x Nt x Ns / 64),
comparable with DESIGN.md's per-pair counts of the exact kernel."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("Laplace3D-FxU", "f64", 20), ("Stokes3D-FxU", "f64", 18), ("Helmholtz3D-FxU", "f64", 20), ("Laplace3D-FxU", "f32", 21)]
NDS = (1, 2, 4, 8, 16)


def run_case(i):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import sctl_amd
    name, prec, lg = CASES[i]
    N = 1 << lg
    dt = torch.float64 if prec == "f64" else torch.float32
    real = 0 if prec == "f64" else 1
    info = sctl_amd.kernel_info(name)
    ctx = np.array([7.5, 0.3]) if name.startswith("Helmholtz") else None
    g = torch.Generator(device="cuda").manual_seed(0)
    xt = torch.rand(N * 3, dtype=dt, device="cuda", generator=g)
    xs = torch.rand(N * 3, dtype=dt, device="cuda", generator=g)
    F = torch.rand((max(NDS), N * info["k0"]), dtype=dt, device="cuda", generator=g) - 0.5
    V = torch.zeros((max(NDS), N * info["k1"]), dtype=dt, device="cuda")

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return sorted(ts)[len(ts) // 2]

    small = 1 << 12
    sctl_amd.eval_device(name, xt[:small * 3], xs[:small * 3], None, F[0, :small * info["k0"]], v_trg=V[0, :small * info["k1"]], ctx=ctx)
    sctl_amd.eval_device(name, xt, xs, None, F[0], v_trg=V[0], ctx=ctx)
    torch.cuda.synchronize()
    single = timed(lambda: sctl_amd.eval_device(name, xt, xs, None, F[0], v_trg=V[0], ctx=ctx), 3)
    path = sctl_amd.plan(name, real, N, N)["path"]
    lines = ["%s %s %d x %d: one single-density call %.1f ms (%s path)" % (name, prec, N, N, single, path)]
    lines.append("  %3s %10s %12s %7s %9s %6s %6s %7s %9s" % ("nd", "multi ms", "nd single ms", "ratio", "cyc/pair", "M", "passes", "splits", "ws MB"))
    for nd in NDS:
        if nd == 1:
            lines.append("  %3d %10.1f %12.1f %7.3f %9s %6d %6d %7s %9s" % (1, single, single, 1.0, "-", 1, 1, "-", "-"))
            continue
        pl = sctl_amd.plan_densities(name, real, nd, N, N)
        Fs, Vs = F[:nd].contiguous(), V[:nd].contiguous()
        Fw = torch.zeros((nd, small * info["k0"]), dtype=dt, device="cuda")
        sctl_amd.eval_densities_device(name, xt[:small * 3], xs[:small * 3], None, Fw, ctx=ctx)     # code objects of this nd's forms
        torch.cuda.synchronize()
        first = timed(lambda: sctl_amd.eval_densities_device(name, xt, xs, None, Fs, V_trg=Vs, ctx=ctx), 1)
        ms = timed(lambda: sctl_amd.eval_densities_device(name, xt, xs, None, Fs, V_trg=Vs, ctx=ctx), 2) if first < 1000 else first
        cyc = ms * 1e-3 * 2.36e9 * 1024 / (pl["passes"] * N * N / 64)
        lines.append("  %3d %10.1f %12.1f %7.3f %9.1f %6d %6d %7d %9.0f" % (nd, ms, nd * single, ms / (nd * single), cyc, pl["densities_per_pass"], pl["passes"],
                                                                             pl["src_splits"], pl["workspace_bytes"] / 2 ** 20))
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:
        run_case(int(sys.argv[sys.argv.index("--case") + 1]))
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r05_densities.txt")
    text = [__doc__.split("\n\n")[0].strip(), ""]
    rc = 0
    for i in range(len(CASES)):
        p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--case", str(i)], capture_output=True, text=True)
        text.append(p.stdout.rstrip())
        if p.returncode != 0:
            text.append("case %d failed with exit status %d:\n%s" % (i, p.returncode, p.stderr[-3000:]))
            rc = p.returncode
            break
        text.append("")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(text).rstrip() + "\n")
    print("\n".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
