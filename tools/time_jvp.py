#!/usr/bin/env python3
"""The tangent kernel (eval_jvp, sctl_amd/csrc/jvp_kernel.hpp) against the forward exact kernel and the target-owned pass of the gradient on the same
points: every built-in kernel, fp64, full precision, 2^18 x 2^18, device arrays, same process, alternating runs, best of 3.  The forward runs have
SCTL_AMD_CENTERED=0 so that they are eval_kernel's, not the tile-centred path's.  A central difference of two forward sums is the only other route to
a tangent, so the line says whether the tangent costs less than two forward sums.

    python tools/time_jvp.py --counts > profiles/rNN_jvp_counts.json      (no GPU: instruction mix per pair of the speculative tile loops from the
                                                                           device assembly, as tools/time_grad.py)
    python tools/time_jvp.py [--n 18] [counts.json]                       (GPU: times, ratios, share of the fp64 vector issue slots against the counts)
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_grad
from isa_loop_counts import KERNELS
from time_transpose import CLOCK_GHZ

time_grad.SYMS["jvp"] = ("inst_j_%s.hip", "_ZN8sctl_amd15eval_jvp_kernelINS_%d%sEdLi%dELi1EEEvNS_9EvalJArgsIT0_EE")
WHICH = ("forward", "grad_trg", "jvp")


def counts():
    res = {}
    for k in KERNELS:
        for which in WHICH:
            res["%s/%s/mode2" % (k.replace("_", "-", 1), which)] = time_grad.loop_counts(k, which, 2)
    json.dump({"what": "per PAIR, speculative tile loop of eval_kernel <K, double, 2, 2 per lane>, eval_grad_kernel <K, double, 2, SIDE 0, 1 per lane> and "
                       "eval_jvp_kernel <K, double, 2, 1 per lane>, gfx950, from hipcc -S", "kernels": res}, sys.stdout, indent=1)


def timings(n, isa):
    import numpy as np, torch
    import sctl_amd
    os.environ["SCTL_AMD_CENTERED"] = "0"
    N = 1 << n
    dt = torch.float64
    print("# %s; wave-cycles per pair = time x %.2f GHz x 1024 SIMDs / (Nt x Ns / 64); counted = 4.1 x fp64 + 16 x v_rsq_f64 + 4 x other VALU per pair"
          % (torch.cuda.get_device_name(0), CLOCK_GHZ), flush=True)
    for name in sctl_amd.KERNEL_NAMES:
        info = sctl_amd.kernel_info(name)
        g = torch.Generator(device="cuda").manual_seed(0)
        r = lambda m, shift=0.0: torch.rand(m, dtype=dt, device="cuda", generator=g) - shift
        xt, xs, xn, f, w = r(N * 3), r(N * 3), r(N * info["nd"], 0.5), r(N * info["k0"], 0.5), r(N * info["k1"], 0.5)
        dxt, dxs, dxn = r(N * 3, 0.5), r(N * 3, 0.5), r(N * info["nd"], 0.5)
        xn, dxn = (xn, dxn) if info["nd"] else (None, None)
        ctx = np.array([7.5, 0.3]) if name.startswith("Helm") else None
        v, du = [torch.zeros(N * info["k1"], dtype=dt, device="cuda") for _ in range(2)]
        gt = torch.zeros(N * 3, dtype=dt, device="cuda")
        runs = (("forward", lambda: sctl_amd.eval_device(name, xt, xs, xn, f, v_trg=v, ctx=ctx)),
                ("grad_trg", lambda: sctl_amd.eval_grad_device(name, xt, xs, xn, f, w, g_trg=gt, want=("trg",), ctx=ctx)),
                ("jvp", lambda: sctl_amd.eval_jvp_device(name, xt, xs, xn, f, d_trg=dxt, d_src=dxs, d_nrm=dxn, dv_trg=du, ctx=ctx)))
        for _, fn in runs:
            fn()
        torch.cuda.synchronize()
        best = {which: 1e30 for which, _ in runs}
        for _ in range(3):                                   # alternating
            for which, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                best[which] = min(best[which], e0.elapsed_time(e1))
        line = "%-17s 2^%d x 2^%d fp64 full precision forward %8.2f ms  grad_trg %8.2f ms  jvp %8.2f ms = %.3f x forward (%s two forward sums), %.3f x grad_trg" % (
            name, n, n, best["forward"], best["grad_trg"], best["jvp"], best["jvp"] / best["forward"],
            "below" if best["jvp"] < 2 * best["forward"] else "ABOVE", best["jvp"] / best["grad_trg"])
        for which, _ in runs:
            rec = isa.get("%s/%s/mode2" % (name, which))
            if rec:
                measured = best[which] * 1e-3 * CLOCK_GHZ * 1e9 * 1024 / (float(N) * N / 64)
                line += " | %s %.1f counted of %.1f measured wave-cycles/pair = %.0f %% of the fp64 vector issue slots" % (
                    which, rec["issue_cycles_per_wave_pair"], measured, 100 * rec["issue_cycles_per_wave_pair"] / measured)
        print(line, flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if "--counts" in a:
        counts()
    else:
        n = int(a[a.index("--n") + 1]) if "--n" in a else 18
        files = [x for x in a if x.endswith(".json")]
        timings(n, json.load(open(files[0]))["kernels"] if files else {})
