"""The grouping of the fp64 tile-centred single layer's source pre-pass (sctl_amd/csrc/fold_prepass.hpp): which class a density falls in and which
record slot of its split a source takes.  The header is plain code, so the device's own functions run here on the CPU through a small host program
(tests/cpp/fold_prepass_main.cpp, compiled with g++) and are compared with a numpy restatement, for the density patterns that reach every branch."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, N = 256, 3 * 256 + 231          # four splits, the last one ragged and no multiple of the 64-record tile
TILE = 64


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fold") / "fold_prepass_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "fold_prepass_main.cpp"), "-o", out], check=True, timeout=300)
    return out


def densities(kind, n=N, chunk=CHUNK):
    rng = np.random.default_rng(31)
    mag = rng.random(n) + 0.1
    if kind == "all_positive":
        return mag
    if kind == "all_negative":
        return -mag
    if kind == "random_signs":
        return mag * rng.choice([-1.0, 1.0], n)
    if kind == "one_sign_runs_out":          # 99 % of one sign
        return mag * np.where(rng.random(n) < 0.01, -1.0, 1.0)
    if kind == "one_source_of_a_sign":       # exactly one negative source in every split
        f = mag.copy()
        f[np.arange(0, n, chunk) + 17] *= -1
        return f
    if kind == "zeros_mixed_in":
        f = mag * rng.choice([-1.0, 1.0], n)
        f[rng.random(n) < 0.3] = 0.0
        f[5] = -0.0
        return f
    if kind == "all_zeros":
        return np.zeros(n)
    if kind == "non_finite":
        f = mag * rng.choice([-1.0, 1.0], n)
        f[rng.choice(n, 40, replace=False)] = np.tile([np.nan, np.inf, -np.inf, -np.nan], 10)
        return f
    if kind == "huge_and_tiny":              # 1e+-160: f^2 over- or underflows (exceptions); 1e+-100: folded, the kernel's band test decides per centre
        return mag * rng.choice([-1.0, 1.0], n) * rng.choice([1e160, 1e-160, 1e100, 1e-100, 1.0], n)
    raise ValueError(kind)


KINDS = ["all_positive", "all_negative", "random_signs", "one_sign_runs_out", "one_source_of_a_sign", "zeros_mixed_in", "all_zeros", "non_finite", "huge_and_tiny"]


def group_numpy(f, chunk):
    """class, slot (or exception rank, or -1), k of every source and (positive tiles, negative tiles, exceptions) of every split"""
    cap = chunk + 2 * TILE
    with np.errstate(all="ignore"):
        k = 1.0 / (f * f)
        ok = (k >= 2.0 ** -900) & (k <= 2.0 ** 900)
    cls = np.where(f == 0, 0, np.where(ok, np.where(f > 0, 1, -1), 2))
    where = np.full(f.size, -1, dtype=np.int64)
    hdr = []
    for b in range(0, f.size, chunk):
        c = cls[b:b + chunk]
        w = where[b:b + chunk]
        rp, rn, re = (np.cumsum(c == v) - 1 for v in (1, -1, 2))
        w[c == 1] = rp[c == 1]
        w[c == -1] = cap - TILE * (rn[c == -1] // TILE + 1) + rn[c == -1] % TILE
        w[c == 2] = re[c == 2]
        hdr.append((-(-int((c == 1).sum()) // TILE), -(-int((c == -1).sum()) // TILE), int((c == 2).sum())))
    return cls, where, np.where(np.abs(cls) == 1, k, 0.0), hdr


def run(prog, f, chunk):
    text = "%d\n" % f.size + "\n".join(float(v).hex() for v in f) + "\n"
    res = subprocess.run([prog, str(chunk)], input=text, capture_output=True, text=True, check=True, timeout=120)
    lines = [l.split() for l in res.stdout.splitlines()]
    src = [l for l in lines if l[0] == "s"]
    return ([int(v) for v in lines[0][1:]], np.array([int(l[1]) for l in src]), np.array([int(l[2]) for l in src], dtype=np.int64),
            np.array([float.fromhex(l[3]) for l in src]), [tuple(int(v) for v in l[1:]) for l in lines if l[0] == "h"])


@pytest.mark.parametrize("kind", KINDS)
def test_grouping_matches_the_numpy_restatement(prog, kind):
    f = densities(kind)
    layout, cls, where, k, hdr = run(prog, f, CHUNK)
    cls0, where0, k0, hdr0 = group_numpy(f, CHUNK)
    assert np.array_equal(cls, cls0) and np.array_equal(where, where0) and hdr == hdr0
    assert np.array_equal(k.view(np.uint64), k0.view(np.uint64))          # k = 1 / f^2 to the bit, 0 where nothing is folded
    cap = layout[0]
    assert cap == CHUNK + 2 * TILE
    for s, b in enumerate(range(0, N, CHUNK)):
        c, w = cls[b:b + CHUNK], where[b:b + CHUNK]
        slots = w[np.abs(c) == 1]
        assert slots.size == np.unique(slots).size and (slots.size == 0 or (slots.min() >= 0 and slots.max() < cap))
        npt, nnt, nexc = hdr[s]
        # positive tiles from the front, negative ones from the back, never in one tile; the valid records of a tile come first and in the caller's order
        assert np.all(w[c == 1] < npt * TILE) and np.all(w[c == -1] >= cap - nnt * TILE) and npt * TILE <= cap - nnt * TILE
        assert np.array_equal(w[c == 1], np.arange((c == 1).sum()))
        rn = np.arange((c == -1).sum())
        assert np.array_equal(w[c == -1], cap - TILE * (rn // TILE + 1) + rn % TILE)
        assert np.array_equal(w[c == 2], np.arange(nexc))
    if kind == "all_zeros":
        assert np.all(cls == 0) and all(h == (0, 0, 0) for h in hdr)
    if kind == "non_finite":
        assert np.all(cls[~np.isfinite(f)] == 2)
    if kind == "huge_and_tiny":
        a = np.abs(f)
        assert np.all(cls[(a > 1e150) | (a < 1e-150)] == 2) and np.all(np.abs(cls[(a > 1e-120) & (a < 1e120)]) == 1)
    if kind == "one_source_of_a_sign":
        assert all(h[1] == 1 for h in hdr)


def test_layout_of_the_block(prog):
    """byte offsets of the four arrays: 256-byte aligned, in order, none overlapping the next"""
    for splits, chunk in ((1, 64), (4, 256), (32, 1024), (256, 64)):
        (cap, rec, idx, exc, total), *_ = run(prog, np.ones((splits - 1) * chunk + 1), chunk)
        assert cap == chunk + 128 and all(v % 256 == 0 for v in (rec, idx, exc, total))
        assert rec >= 16 * splits and idx - rec >= 32 * splits * cap and exc - idx >= 4 * splits * cap and total - exc >= 4 * splits * chunk
