#!/usr/bin/env python3
"""The transposed all-pairs kernel against the forward exact kernel it was derived from: every built-in kernel, fp64, 2^18 x 2^18, full precision
and 10 digits, device arrays, same points, same process, alternating runs, best of 3.  The forward runs have SCTL_AMD_CENTERED=0 so that they
are eval_kernel's, not the tile-centred path's.

    python tools/time_transpose.py --counts > profiles/rNN_transpose_counts.json     (no GPU: instruction mix per pair of both speculative tile
                                                                                        loops from the device assembly, as tools/isa_loop_counts.py)
    python tools/time_transpose.py [--n 18] [counts.json]                             (GPU: times, ratios, wave-cycles per pair against the counts)
"""
import json, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_loop_counts import KERNELS, count, loops

SYMS = {"forward": ("inst_%s.hip", "_ZN8sctl_amd11eval_kernelINS_%d%sEdLi%dELi2EEEvNS_8EvalArgsIT0_EE"),
        "transposed": ("inst_t_%s.hip", "_ZN8sctl_amd21eval_transpose_kernelINS_%d%sEdLi%dELi2EEEvNS_9EvalTArgsIT0_EE")}
CLOCK_GHZ = float(os.environ.get("SCTL_AMD_CLOCK_GHZ", "2.36"))   # the clock tools/time_densities.py counts with
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")


def mk(*a):
    """the flags the library's units are built with, from the Makefile itself (as tools/check_isa_rules.py)"""
    return subprocess.run(["make", "-s", "-C", CSRC] + list(a), capture_output=True, text=True, check=True).stdout.split()


def loop_counts(k, which, mode):
    """per pair, the unmasked unrolled tile loop of the two-per-lane fp64 instantiation (the selection rule of tools/isa_loop_counts.py)"""
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
    json.dump({"what": "per PAIR, speculative tile loop of eval_kernel / eval_transpose_kernel <K, double, MODE, 2 per lane>, gfx950, from hipcc -S",
               "kernels": res}, sys.stdout, indent=1)


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
        v, gs = torch.zeros(N * info["k1"], dtype=dt, device="cuda"), torch.zeros(N * info["k0"], dtype=dt, device="cuda")
        for digits, mode in ((-1, 2), (10, 1)):
            fwd = lambda: sctl_amd.eval_device(name, xt, xs, xn, f, v_trg=v, ctx=ctx, digits=digits)
            trn = lambda: sctl_amd.eval_transpose_device(name, xt, xs, xn, w, g_src=gs, ctx=ctx, digits=digits)
            fwd(); trn(); torch.cuda.synchronize()
            best = {"forward": 1e30, "transposed": 1e30}
            for _ in range(3):                                   # alternating
                for which, fn in (("forward", fwd), ("transposed", trn)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                    best[which] = min(best[which], e0.elapsed_time(e1))
            line = "%-17s 2^%d x 2^%d fp64 %-14s forward %8.2f ms  transposed %8.2f ms  ratio %.3f" % (
                name, n, n, "full precision" if digits < 0 else "%d digits" % digits, best["forward"], best["transposed"], best["transposed"] / best["forward"])
            for which in ("forward", "transposed"):
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
