#!/usr/bin/env python3
"""Several weight vectors through the transposed sum in one call against as many calls of the single transposed entry
(sctl_amd_eval_transpose_densities_device vs sctl_amd_eval_transpose_device), every kernel, fp64 and fp32, 2^18 x 2^18, one row per form (nd = 2, 4, 8:
nd weight vectors fill the form).

    python tools/time_transpose_densities.py [--out profiles/r12_transpose_densities.txt] [--lg 18]
                                                                one child process per kernel, each under `timeout -k 10 <s>`;
                                                                stops at the first kernel that fails and writes what it has
    python tools/time_transpose_densities.py --case I [--lg 18]  one kernel (what the driver runs)

Each figure is the median of nine timings, the two sides alternating (one multi call, then its nd single calls, nine times over), after a warm-up of
both on the timed shape; "spread" is (max - min) / median of the nine.  Times are HIP events around work on torch's current stream.  "ratio" is multi /
(nd single): a form whose ratio is not below 1 by more than the spread is not worth shipping.  The last column compares the result rows with the single
calls' (largest rel-L2 of a row)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDS = (2, 4, 8)
REPS = 9


def lg_arg():
    return int(sys.argv[sys.argv.index("--lg") + 1]) if "--lg" in sys.argv else 18


def run_case(i):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import sctl_amd
    name = sctl_amd.KERNEL_NAMES[i]
    N = 1 << lg_arg()
    info = sctl_amd.kernel_info(name)
    ctx = np.array([7.5, 0.3]) if name.startswith("Helmholtz") else None
    lines = []
    for prec, dt, real in (("f64", torch.float64, 0), ("f32", torch.float32, 1)):
        g = torch.Generator(device="cuda").manual_seed(0)
        xt = torch.rand(N * 3, dtype=dt, device="cuda", generator=g)
        xs = torch.rand(N * 3, dtype=dt, device="cuda", generator=g)
        xn = (torch.rand(N * 3, dtype=dt, device="cuda", generator=g) - 0.5) if info["nd"] else None
        W = torch.rand((max(NDS), N * info["k1"]), dtype=dt, device="cuda", generator=g) - 0.5
        G = torch.zeros((max(NDS), N * info["k0"]), dtype=dt, device="cuda")
        g1 = torch.zeros(N * info["k0"], dtype=dt, device="cuda")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def stats(ts):
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            return med, (ts[-1] - ts[0]) / med

        single_plan = sctl_amd.plan_transpose(name, real, N, N)
        lines.append("%s %s %d x %d (single: %d per lane, %d splits)" % (name, prec, N, N, single_plan["src_per_lane"], single_plan["splits"]))
        lines.append("  %3s %2s %2s %7s %9s %7s %13s %7s %7s %9s" % ("nd", "M", "T", "splits", "multi ms", "spread", "nd single ms", "spread", "ratio", "rows"))
        for nd in NDS:
            pl = sctl_amd.plan_transpose_densities(name, real, nd, N, N)
            Ws, Gs = W[:nd].contiguous(), G[:nd].contiguous()
            multi = lambda: sctl_amd.eval_transpose_densities_device(name, xt, xs, xn, Ws, G_src=Gs, ctx=ctx)

            def singles():
                for m in range(nd):
                    sctl_amd.eval_transpose_device(name, xt, xs, xn, Ws[m], g_src=g1, ctx=ctx)

            Gs.zero_()
            multi()                                               # warm-up of both sides on the timed shape, and the comparison of the rows
            err = 0.0
            for m in range(nd):
                g1.zero_()
                sctl_amd.eval_transpose_device(name, xt, xs, xn, Ws[m], g_src=g1, ctx=ctx)
                err = max(err, float((Gs[m] - g1).norm() / g1.norm()))
            torch.cuda.synchronize()
            tm, tsn = [], []
            for _ in range(REPS):
                tm.append(timed(multi))
                tsn.append(timed(singles))
            (m_med, m_spread), (s_med, s_spread) = stats(tm), stats(tsn)
            if pl["vectors_per_pass"] != nd:
                note = "  (no form of %d: %d passes of %d)" % (nd, pl["passes"], pl["vectors_per_pass"])
            else:
                note = ""
            lines.append("  %3d %2d %2d %7d %9.2f %6.1f%% %13.2f %6.1f%% %7.3f %9.1e%s" % (nd, pl["vectors_per_pass"], pl["src_per_lane"], pl["splits"], m_med,
                                                                                         100 * m_spread, s_med, 100 * s_spread, m_med / s_med, err, note))
        lines.append("")
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:
        run_case(int(sys.argv[sys.argv.index("--case") + 1]))
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r12_transpose_densities.txt")
    text = [__doc__.split("\n\n")[0].strip(), ""]
    rc = 0
    for i in range(10):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", str(i), "--lg", str(lg_arg())], capture_output=True, text=True)
        text.append(p.stdout.rstrip())
        if p.returncode != 0:
            text.append("case %d failed with exit status %d:\n%s" % (i, p.returncode, p.stderr[-3000:]))
            rc = p.returncode
            break
        text.append("")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:                               # what there is so far, after every kernel
            fh.write("\n".join(text).rstrip() + "\n")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(text).rstrip() + "\n")
    print("\n".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
