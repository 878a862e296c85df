#!/usr/bin/env python3
"""Near share of the tile-centred kernels per target cluster, for the target order the device makes and for the Z-curve order it made until round 5.

A wave of centered_kernel owns `--cluster` consecutive targets of the order (256 for the fp64 single layer); a source within sqrt(kNearFactor2) = 2 cluster
radii of the cluster's bounding-box centre takes the exact masked pair (~17 issue slots instead of 12).  This prints mean / median / maximum over the
clusters of the share of such sources, on a sample of the sources — the kernel's own centre, radius and rule (centered_kernel.hpp), the device's own key
function (sctl_amd/csrc/curve_key.hpp, compiled into tests/cpp/curve_key_main.cpp: the host twin of morton_keys_kernel + the stable radix sort).

    python tools/near_share.py [--n 1048576] [--cluster 256] [--sources 4000] [--order hilbert|morton|both]

Points: bench.py's seeded clouds (torch.rand on the GPU, seed 0: targets first, then sources) where a GPU is there, else numpy's default_rng(0) — the
same uniform distribution in [0, 1)^3, other points; the line printed says which.  None of the library's kernels is launched."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clouds(n):
    try:
        import torch
        if torch.cuda.is_available():
            g = torch.Generator(device="cuda").manual_seed(0)
            xt = torch.rand(n * 3, dtype=torch.float64, device="cuda", generator=g)
            xs = torch.rand(n * 3, dtype=torch.float64, device="cuda", generator=g)
            return xt.cpu().numpy().reshape(n, 3), xs.cpu().numpy().reshape(n, 3), "bench.py's seeded clouds (torch.rand on the GPU, seed 0)"
    except ImportError:
        pass
    rng = np.random.default_rng(0)
    return rng.random((n, 3)), rng.random((n, 3)), "numpy default_rng(0) uniform clouds (no GPU here: not bench.py's points, the same distribution)"


def hilbert_keys(x):
    with tempfile.TemporaryDirectory() as tmp:
        prog = os.path.join(tmp, "curve_key_main")
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "curve_key_main.cpp"), "-o", prog], check=True)
        text = "%d\n" % len(x) + "\n".join("%r %r %r" % tuple(r) for r in x.tolist()) + "\n"
        out = subprocess.run([prog, "points"], input=text, capture_output=True, text=True, check=True).stdout
    return np.array(out.split(), dtype=np.uint64)


def morton_keys(x):
    """the key of rounds 1-5: the same cells, bits interleaved (axis k at bit k of each triple)"""
    lo, hi = x.min(axis=0), x.max(axis=0)
    w = hi - lo
    q = np.where(w > 0, (x - lo) / np.where(w > 0, w, 1.0) * 2097151.0, 0.0)
    q = np.minimum(q, 2097151.0).astype(np.uint64)
    key = np.zeros(len(x), dtype=np.uint64)
    for b in range(21):
        for k in range(3):
            key |= ((q[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return key


def near_share(xt, xs, keys, cluster, factor2=4.0):
    order = np.argsort(keys, kind="stable")
    n = len(xt) // cluster * cluster
    c = xt[order[:n]].reshape(-1, cluster, 3)
    centre = 0.5 * c.min(axis=1) + 0.5 * c.max(axis=1)
    rt2 = ((c - centre[:, None, :]) ** 2).sum(axis=2).max(axis=1)
    share = np.empty(len(centre))
    for i in range(0, len(centre), 512):
        d2 = ((xs[None, :, :] - centre[i:i + 512, None, :]) ** 2).sum(axis=2)
        share[i:i + 512] = (d2 <= factor2 * rt2[i:i + 512, None]).mean(axis=1)
    return share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--cluster", type=int, default=256)
    ap.add_argument("--sources", type=int, default=4000)
    ap.add_argument("--order", default="both", choices=["hilbert", "morton", "both"])
    a = ap.parse_args()
    xt, xs, what = clouds(a.n)
    xs = xs[np.random.default_rng(1).choice(a.n, min(a.sources, a.n), replace=False)]
    print("near share per %d-target cluster, %d targets, %d sampled sources of %d, near <=> |x_s - c|^2 <= 4 Rt^2; %s" % (a.cluster, a.n, len(xs), a.n, what))
    for name, fn in (("morton", morton_keys), ("hilbert", hilbert_keys)):
        if a.order in (name, "both"):
            s = near_share(xt, xs, fn(xt), a.cluster)
            print("  %-8s mean %.3f %%  median %.3f %%  max %.3f %%  (all %d clusters)" % (name, 100 * s.mean(), 100 * np.median(s), 100 * s.max(), len(s)))


if __name__ == "__main__":
    sys.exit(main())
