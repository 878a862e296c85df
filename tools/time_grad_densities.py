#!/usr/bin/env python3
"""Geometry gradients of several density / weight rows in one call against as many calls of the unchanged single gradient entry
(sctl_amd_eval_grad_densities_device vs sctl_amd_eval_grad_device), every kernel, each side, fp64 and fp32, full precision, 2^18 x 2^18, device arrays,
one row per form (nd = 2, 4, 8: nd rows fill the form).

    python tools/time_grad_densities.py [--out profiles/r15_grad_densities.txt] [--lg 18] [--kernels 0,1,2]
                                                                one child process per kernel, each under `timeout -k 10 <s>`;
                                                                stops at the first kernel that fails and writes what it has
    python tools/time_grad_densities.py --case I [--lg 18]      one kernel (what the driver runs)

Both sides of a comparison run in the same process and accumulate into the same outputs.  Each figure is the median of nine timings, the two sides
alternating (one multi call, then its nd single calls, nine times over), after a warm-up of both on the timed shape; "spread" is (max - min) / median of
the nine.  Times are HIP events around work on torch's current stream.  "ratio" is multi / (nd single): a form whose ratio is not below 1 by more than the
spread of its row does not stay in the dispatch.  The last column is the rel-L2 between the two results (the largest over the side's outputs: g_trg for
the target-owned side; g_src and, with a normal, g_nrm for the source-owned side)."""
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
        F = torch.rand((max(NDS), N * info["k0"]), dtype=dt, device="cuda", generator=g) - 0.5
        W = torch.rand((max(NDS), N * info["k1"]), dtype=dt, device="cuda", generator=g) - 0.5
        out = [torch.zeros(N * 3, dtype=dt, device="cuda") for _ in range(3)]          # g_trg, g_src, g_nrm: both sides of a comparison add into these
        ref = [torch.zeros(N * 3, dtype=dt, device="cuda") for _ in range(3)]

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

        single_plan = sctl_amd.plan_grad(name, real, N, N)
        for side, want in (("trg", ("trg",)), ("src", ("src", "nrm") if info["nd"] else ("src",))):
            used = [k for k, what in enumerate(("trg", "src", "nrm")) if what in want]
            lines.append("%s %s %d x %d, %s-owned side (single: %d splits)" % (name, prec, N, N, "target" if side == "trg" else "source", single_plan[side]["splits"]))
            lines.append("  %3s %2s %6s %7s %9s %7s %13s %7s %7s %9s" % ("nd", "M", "passes", "splits", "multi ms", "spread", "nd single ms", "spread", "ratio", "rel-L2"))
            for nd in NDS:
                pl = sctl_amd.plan_grad_densities(name, real, nd, N, N)
                Fs, Ws = F[:nd].contiguous(), W[:nd].contiguous()

                def multi(to=out):
                    sctl_amd.eval_grad_densities_device(name, xt, xs, xn, Fs, Ws, to[0], to[1], to[2], want=want, ctx=ctx)

                def singles(to=out):
                    for m in range(nd):
                        sctl_amd.eval_grad_device(name, xt, xs, xn, Fs[m], Ws[m], to[0], to[1], to[2], want=want, ctx=ctx)

                for k in used:
                    out[k].zero_()
                    ref[k].zero_()
                multi(out)                                            # warm-up of both sides on the timed shape, and the comparison of the results
                singles(ref)
                err = max(float((out[k] - ref[k]).norm() / ref[k].norm()) for k in used)
                torch.cuda.synchronize()
                tm, tsn = [], []
                for _ in range(REPS):
                    tm.append(timed(multi))
                    tsn.append(timed(singles))
                (m_med, m_spread), (s_med, s_spread) = stats(tm), stats(tsn)
                lines.append("  %3d %2d %6d %7d %9.2f %6.1f%% %13.2f %6.1f%% %7.3f %9.1e" % (nd, pl["rows_per_pass"], pl["passes"], pl[side]["splits"], m_med, 100 * m_spread,
                                                                                           s_med, 100 * s_spread, m_med / s_med, err))
            lines.append("")
    print("\n".join(lines), flush=True)


def main():
    if "--case" in sys.argv:
        run_case(int(sys.argv[sys.argv.index("--case") + 1]))
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r15_grad_densities.txt")
    kernels = [int(x) for x in sys.argv[sys.argv.index("--kernels") + 1].split(",")] if "--kernels" in sys.argv else list(range(10))
    text = [__doc__.split("\n\n")[0].strip(), ""]
    rc = 0

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(text).rstrip() + "\n")

    for i in kernels:
        p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--case", str(i), "--lg", str(lg_arg())], capture_output=True, text=True)
        text.append(p.stdout.rstrip())
        print(p.stdout.rstrip(), flush=True)
        if p.returncode != 0:
            text.append("case %d failed with exit status %d:\n%s" % (i, p.returncode, p.stderr[-3000:]))
            print(text[-1], flush=True)
            rc = p.returncode
            break
        text.append("")
        write()                                                  # what there is so far, after every kernel
    write()
    return rc


if __name__ == "__main__":
    sys.exit(main())
