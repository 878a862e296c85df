"""The target order of the tile-centred kernels (Hilbert keys, sctl_amd/csrc/curve_key.hpp) on the GPU, at the smallest shape the path takes by itself
(2^18 targets x 2^14 sources, fp64): target clouds whose bounding box is ordinary, degenerate (a plane, a line) or mostly empty (two blobs), a ragged
count; each against the CPU oracle on a fixed subset and against a second run with the targets shuffled — the order is a pure function of the
coordinates, so a target's potential must not depend on where the caller put it."""
import os

import numpy as np
import pytest

import sctl_amd
from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAME = "Laplace3D-FxU"
NT, NS, NSEL = 1 << 18, 1 << 14, 512


def _targets(kind, rng):
    nt = NT + 37 if kind == "ragged" else NT
    x = rng.random((nt, 3))
    if kind == "plane":
        x[:, 2] = 0.375
    elif kind == "line":
        x[:, 1], x[:, 2] = 0.625, 0.375
    elif kind == "blobs":                   # two tight blobs far apart: nearly all cells of the box are empty
        x = 1e-3 * rng.standard_normal((nt, 3)) + np.where(rng.random(nt) < 0.5, 0.0, 50.0)[:, None]
    return x


def _sources(rng, dt=np.float64):
    xs = rng.random((NS, 3))
    xs[:NS // 8] *= 1e-3                    # some inside the blob at the origin
    return np.ascontiguousarray(xs.ravel()).astype(dt), (rng.random(NS) - 0.5).astype(dt)


def _eval(xt, xs, f):
    import torch
    return sctl_amd.eval_device(NAME, torch.from_numpy(np.ascontiguousarray(xt.ravel())).cuda(), torch.from_numpy(xs).cuda(), None, torch.from_numpy(f).cuda()).cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform", "plane", "line", "blobs", "ragged"])
def test_clouds_against_the_oracle_and_shuffled(O, kind):
    rng = np.random.default_rng(606)
    xt = _targets(kind, rng)
    nt = len(xt)
    xs, f = _sources(rng)
    assert sctl_amd.plan(NAME, 0, nt, NS)["path"] == "tile-centred"
    u = _eval(xt, xs, f)
    assert np.all(np.isfinite(u))
    sel = rng.choice(nt, NSEL, replace=False)
    ref = O.eval(NAME, xt[sel].ravel().copy(), xs, None, f)
    err = rel_l2(u[sel], ref)
    print(kind, "rel-L2 vs oracle on %d targets: %.3e" % (NSEL, err))
    assert err <= 1e-12, (kind, err)
    p = rng.permutation(nt)
    u_shuffled = _eval(xt[p], xs, f)
    d = float(np.abs(u_shuffled - u[p]).max() / np.linalg.norm(u) * np.sqrt(nt))   # per target, relative to the rms potential
    print(kind, "shuffled, largest difference of a target / rms potential: %.3e" % d)
    assert d <= 1e-12, (kind, d)
    assert rel_l2(u_shuffled[np.argsort(p)][sel], ref) <= 1e-12


def test_repeat_is_bit_identical():
    rng = np.random.default_rng(607)
    xt = _targets("blobs", rng)
    xs, f = _sources(rng)
    assert np.array_equal(_eval(xt, xs, f), _eval(xt, xs, f))


def test_fp32_matrix_core_kernel_on_the_new_order(O):
    """fp32 at the default accuracy through the matrix-core kernel, the bound of tests/test_gpu_centered.py::test_centred_path_fp32: within 1e-4 of the
    fp64 oracle and no worse than three times the exact fp32 kernel's own error."""
    import torch
    rng = np.random.default_rng(608)
    xt = np.ascontiguousarray(_targets("uniform", rng).ravel()).astype(np.float32)
    xs, f = _sources(rng, np.float32)
    pl = sctl_amd.plan(NAME, 1, NT, NS)
    assert pl["path"] == "tile-centred" and pl["pipe"].startswith("bf16 matrix cores"), pl
    d = [torch.from_numpy(a).cuda() for a in (xt, xs, f)]
    u = sctl_amd.eval_device(NAME, d[0], d[1], None, d[2]).cpu().numpy()
    os.environ["SCTL_AMD_CENTERED"] = "0"
    try:
        u_exact = sctl_amd.eval_device(NAME, d[0], d[1], None, d[2]).cpu().numpy()
    finally:
        del os.environ["SCTL_AMD_CENTERED"]
    sel = rng.choice(NT, NSEL, replace=False)
    ref = O.eval(NAME, xt.reshape(NT, 3)[sel].astype(np.float64).ravel().copy(), xs.astype(np.float64), None, f.astype(np.float64))
    e_c, e_x = rel_l2(u[sel], ref), rel_l2(u_exact[sel], ref)
    print("fp32: centred %.3e exact %.3e" % (e_c, e_x))
    assert e_c <= 1e-4 and e_c <= 3 * e_x + 1e-6, (e_c, e_x)
