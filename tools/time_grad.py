#!/usr/bin/env python3
"""The two gradient kernels (targets own the sums / sources own the sums) against the forward exact kernel on the same points: every built-in
kernel, fp64, 2^18 x 2^18, full precision and 10 digits, device arrays, same process, alternating runs, best of 3.  The forward runs have
SCTL_AMD_CENTERED=0 so that they are eval_kernel's, not the tile-centred path's.

    python tools/time_grad.py --counts > profiles/rNN_grad_counts.json     (no GPU: instruction mix per pair of the speculative tile loops from the
                                                                            device assembly, as tools/time_transpose.py)
    python tools/time_grad.py [--n 18] [counts.json]                       (GPU: times, ratios, wave-cycles per pair against the counts)
"""
import json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_loop_counts import KERNELS, count, loops
from time_transpose import CLOCK_GHZ, CSRC, mk

SYMS = {"forward": ("inst_%s.hip", "_ZN8sctl_amd11eval_kernelINS_%d%sEdLi%dELi2EEEvNS_8EvalArgsIT0_EE"),
        "grad_trg": ("inst_g_%s.hip", "_ZN8sctl_amd16eval_grad_kernelINS_%d%sEdLi%dELi0ELi1EEEvNS_9EvalGArgsIT0_EE"),
        "grad_src": ("inst_g_%s.hip", "_ZN8sctl_amd16eval_grad_kernelINS_%d%sEdLi%dELi1ELi1EEEvNS_9EvalGArgsIT0_EE")}


def loop_counts(k, which, mode):
    """per pair, the unmasked unrolled tile loop of the fp64 instantiation the library launches at this size (forward: two targets per lane; gradient:
    one owner per lane)"""
    unit, sym = SYMS[which]
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + mk("print-flags") + mk("print-unit-flags", "UNIT=" + (unit % k)[:-4]) +
                       ["--offload-device-only", "-S", os.path.join(CSRC, unit % k), "-o", asm], check=True, stderr=subprocess.DEVNULL)
        src = open(asm).read()
    sym = sym % (len(k), k, mode)
    i0 = src.index("\n" + sym + ":")
    body = src[i0:src.index(".Lfunc_end", i0)].split("\n")
    tail = src[i0:]
    cands = []
    for a, b in loops(body):
        c = count(body, a, b)
        if c["rsq"] >= 2 and c["branches"] == 1 and not any("v_cndmask" in l for l in body[a:b + 1]):
            cands.append(c)
    if k == "Helmholtz3D_FxU":
        cands = [c for c in cands if c["ldexp"] == 0 and c["lds_b64"] >= c["rsq"]] or cands
    most = max(c["rsq"] for c in cands)
    c = next(c for c in cands if c["rsq"] == most)
    per = {kk: c[kk] / float(most) for kk in ("f64", "rsq", "other_valu", "lds_reads")}
    per["issue_cycles_per_wave_pair"] = 4.1 * per["f64"] + 16.0 * per["rsq"] + 4.0 * per["other_valu"]
    per["vgprs"] = int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
    per["occupancy"] = int(re.search(r"; Occupancy: (\d+)", tail).group(1))
    return per


def counts():
    res = {}
    for k in KERNELS:
        for mode in (2, 1):
            for which in SYMS:
                res["%s/%s/mode%d" % (k.replace("_", "-", 1), which, mode)] = loop_counts(k, which, mode)
    json.dump({"what": "per PAIR, speculative tile loop of eval_kernel <K, double, MODE, 2 per lane> and eval_grad_kernel <K, double, MODE, SIDE, 1 per lane>, "
                       "gfx950, from hipcc -S", "kernels": res}, sys.stdout, indent=1)


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
        xn = xn if info["nd"] else None
        ctx = np.array([7.5, 0.3]) if name.startswith("Helm") else None
        v = torch.zeros(N * info["k1"], dtype=dt, device="cuda")
        gt, gs, gn = [torch.zeros(N * 3, dtype=dt, device="cuda") for _ in range(3)]
        src_want = ("src", "nrm") if info["nd"] else ("src",)
        for digits, mode in ((-1, 2), (10, 1)):
            runs = (("forward", lambda: sctl_amd.eval_device(name, xt, xs, xn, f, v_trg=v, ctx=ctx, digits=digits)),
                    ("grad_trg", lambda: sctl_amd.eval_grad_device(name, xt, xs, xn, f, w, g_trg=gt, want=("trg",), ctx=ctx, digits=digits)),
                    ("grad_src", lambda: sctl_amd.eval_grad_device(name, xt, xs, xn, f, w, g_src=gs, g_nrm=gn, want=src_want, ctx=ctx, digits=digits)))
            for _, fn in runs:
                fn()
            torch.cuda.synchronize()
            best = {which: 1e30 for which, _ in runs}
            for _ in range(3):                                   # alternating
                for which, fn in runs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                    best[which] = min(best[which], e0.elapsed_time(e1))
            line = "%-17s 2^%d x 2^%d fp64 %-14s forward %8.2f ms  grad_trg %8.2f ms (x %.3f)  grad_src %8.2f ms (x %.3f)" % (
                name, n, n, "full precision" if digits < 0 else "%d digits" % digits, best["forward"], best["grad_trg"], best["grad_trg"] / best["forward"],
                best["grad_src"], best["grad_src"] / best["forward"])
            for which, _ in runs:
                rec = isa.get("%s/%s/mode%d" % (name, which, mode))
                if rec:
                    measured = best[which] * 1e-3 * CLOCK_GHZ * 1e9 * 1024 / (float(N) * N / 64)
                    line += " | %s %.1f counted of %.1f measured wave-cycles/pair = %.0f %% of issue" % (which, rec["issue_cycles_per_wave_pair"], measured,
                                                                                                        100 * rec["issue_cycles_per_wave_pair"] / measured)
            print(line, flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if "--counts" in a:
        counts()
    else:
        n = int(a[a.index("--n") + 1]) if "--n" in a else 18
        files = [x for x in a if x.endswith(".json")]
        timings(n, json.load(open(files[0]))["kernels"] if files else {})
