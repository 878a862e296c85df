"""The sort key of the tile-centred kernels' target order (sctl_amd/csrc/curve_key.hpp): the 3-D Hilbert index of a point's cell.  The header is plain
integer code, so the device's own functions run here on the CPU through a small host program (tests/cpp/curve_key_main.cpp, compiled with g++): a
bijection, face-adjacent consecutive cells — what makes a range of the order compact, and what the Z-curve lacks —, agreement with an independent numpy
implementation of Skilling's algorithm, and degenerate boxes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("curve") / "curve_key_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "curve_key_main.cpp"), "-o", out], check=True, timeout=300)
    return out


def _keys(prog, args, rows, fmt):
    text = "%d\n" % len(rows) + "\n".join(" ".join(fmt % v for v in r) for r in rows) + "\n"
    res = subprocess.run([prog] + args, input=text, capture_output=True, text=True, check=True, timeout=120)
    return np.array([int(l) for l in res.stdout.split()], dtype=np.uint64)


def _cell_keys(prog, cells, bits):
    return _keys(prog, ["cells", str(bits)], cells, "%d")


def _point_keys(prog, pts):
    return _keys(prog, ["points"], pts, "%r")


def hilbert_numpy(cells, bits):
    """Skilling's AxesToTranspose on whole arrays, then the interleave by a loop over the bits (axis 0 most significant of each triple)."""
    X = [cells[:, k].astype(np.uint64).copy() for k in range(3)]
    q = np.uint64(1) << np.uint64(bits - 1)
    while q > 1:
        p = q - np.uint64(1)
        for i in range(3):
            hit = (X[i] & q) != 0
            X[0] = np.where(hit, X[0] ^ p, X[0])
            t = np.where(hit, np.uint64(0), (X[0] ^ X[i]) & p)
            X[0] ^= t
            X[i] ^= t
        q >>= np.uint64(1)
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    q = np.uint64(1) << np.uint64(bits - 1)
    while q > 1:
        t = np.where((X[2] & q) != 0, t ^ (q - np.uint64(1)), t)
        q >>= np.uint64(1)
    X = [x ^ t for x in X]
    key = np.zeros_like(X[0])
    for b in range(bits - 1, -1, -1):
        for i in range(3):
            key = (key << np.uint64(1)) | ((X[i] >> np.uint64(b)) & np.uint64(1))
    return key


def test_bijection_and_face_adjacency_on_a_16_cube(prog):
    g = np.arange(16)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    keys = _cell_keys(prog, cells, 4)
    assert np.array_equal(np.sort(keys), np.arange(4096, dtype=np.uint64))
    walk = cells[np.argsort(keys)]
    step = np.abs(np.diff(walk, axis=0))
    assert np.all(step.sum(axis=1) == 1) and np.all(step.max(axis=1) == 1)     # one step in exactly one axis
    assert np.array_equal(keys, hilbert_numpy(cells, 4))


def test_keys_match_an_independent_numpy_implementation(prog):
    rng = np.random.default_rng(11)
    cells = rng.integers(0, 1 << 21, (10000, 3))
    cells[:8] = [[0, 0, 0], [(1 << 21) - 1] * 3, [(1 << 21) - 1, 0, 0], [0, (1 << 21) - 1, 0], [0, 0, (1 << 21) - 1], [1 << 20, 1 << 20, 1 << 20], [(1 << 20) - 1] * 3, [1, 2, 3]]
    keys = _cell_keys(prog, cells, 21)
    assert np.array_equal(keys, hilbert_numpy(cells, 21))
    assert keys.max() < np.uint64(1) << np.uint64(63)


def test_points_in_a_box_take_the_key_of_their_cell(prog):
    """the whole pipeline of the device kernel: bounding box, cell = floor((x - lo) / w (2^21 - 1)), key"""
    rng = np.random.default_rng(12)
    pts = rng.random((2000, 3)) * [1.0, 5.0, 0.01] + [0.0, -3.0, 100.0]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    cells = np.minimum(np.floor((pts - lo) / (hi - lo) * 2097151.0), 2097151.0).astype(np.int64)
    assert np.array_equal(_point_keys(prog, pts.tolist()), hilbert_numpy(cells, 21))


@pytest.mark.parametrize("flat", [(2,), (0, 1), (0, 1, 2)])
def test_boxes_of_zero_extent_give_a_valid_stable_order(prog, flat):
    """all points on a plane, on a line, at one point: the flat axes give cell 0, the others order the points as before; the order (a stable sort of the
    keys, as the device's radix sort is) is a permutation and the same on every run"""
    rng = np.random.default_rng(13)
    pts = rng.random((3000, 3))
    pts[:, list(flat)] = 0.25
    keys = _point_keys(prog, pts.tolist())
    assert np.array_equal(keys, _point_keys(prog, pts.tolist()))
    assert keys.max() < np.uint64(1) << np.uint64(63)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(np.sort(order), np.arange(3000))
    if len(flat) == 3:
        assert np.all(keys == keys[0]) and np.array_equal(order, np.arange(3000))       # ties keep the caller's order
    else:
        free = [k for k in range(3) if k not in flat]
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        cells = np.zeros((3000, 3), dtype=np.int64)
        cells[:, free] = np.minimum(np.floor((pts[:, free] - lo[free]) / (hi[free] - lo[free]) * 2097151.0), 2097151.0)
        assert np.array_equal(keys, hilbert_numpy(cells, 21))


def test_a_single_point_and_no_point(prog):
    assert _point_keys(prog, [[0.3, -1.0, 7.0]]).tolist() == [0]
    assert _point_keys(prog, []).size == 0


def test_non_finite_coordinates_get_a_valid_key(prog):
    pts = np.random.default_rng(14).random((100, 3))
    pts[3, 0], pts[5, 1], pts[7, 2] = np.nan, np.inf, -np.inf
    text = "100\n" + "\n".join(" ".join(repr(float(v)) for v in r) for r in pts) + "\n"
    res = subprocess.run([prog, "points"], input=text, capture_output=True, text=True, check=True, timeout=60)
    keys = [int(l) for l in res.stdout.split()]
    assert len(keys) == 100 and all(0 <= k < (1 << 63) for k in keys)
