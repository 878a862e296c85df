"""The truth of the gradient tests (tests/test_grad_cpu.py, tests/test_gpu_grad.py): the ten kernels' K0 x K1 blocks written in torch from the formulas
of the reference's include/sctl/kernel_functions.hpp (the numpy twin is tests/test_independent_math.py::_kernel_values), the scalar
L = <w, A f> they make, and its derivatives by torch's CPU autograd.  A coincident pair contributes 0, as everywhere in this library."""
import math

import torch

# the wavenumbers of tests/test_gpu_transpose.py: complex and real, one-reduction and two-reduction table forms in fp64 (the first is conftest's default)
HELMHOLTZ_KS = [(7.5, 0.3), (7.5, 0.0), (-3.0, 2.5), (0.0, 0.7)]


def kernel_blocks(name, xt, xs, xn, ctx=None, lam=None):
    """U[t, s, k0, k1] with the scale factor; xt (Nt, 3), xs (Ns, 3), xn (Ns, 3) or None, in their own dtype.  Coincident pairs: 0."""
    dt = xt.dtype
    d = xt[:, None, :] - xs[None, :, :]
    r2 = (d * d).sum(-1)
    hit = r2 == 0
    ri = torch.where(hit, torch.zeros_like(r2), 1.0 / torch.sqrt(torch.where(hit, torch.ones_like(r2), r2)))     # (no 0 * inf in the backward either)
    ri3 = ri * ri * ri
    ri5 = ri3 * ri * ri
    pi4, pi8 = 4 * math.pi, 8 * math.pi
    eye = torch.eye(3, dtype=dt)
    n = None if xn is None else xn[None, :, :].expand_as(d)
    if name == "Laplace3D-FxU":
        return (ri / pi4)[..., None, None]
    if name == "Laplace3D-DxU":
        return ((d * n).sum(-1) * ri3 / pi4)[..., None, None]
    if name == "Laplace3D-FxdU":
        return (-(d * ri3[..., None]) / pi4)[..., None, :]
    stokeslet = (eye * ri[..., None, None] + d[..., :, None] * d[..., None, :] * ri3[..., None, None]) / pi8
    if name == "Stokes3D-FxU":
        return stokeslet
    if name == "Stokes3D-DxU":
        return d[..., :, None] * d[..., None, :] * ((d * n).sum(-1) * ri5)[..., None, None] * (3 / pi4)
    if name == "Stokes3D-FxT":
        t = d[..., :, None, None] * d[..., None, :, None] * d[..., None, None, :] * ri5[..., None, None, None]
        return (-(3 / pi4) * t).reshape(d.shape[0], d.shape[1], 3, 9)
    if name == "Stokes3D-FSxU":
        return torch.cat([stokeslet, (d * ri3[..., None] / pi8)[..., None, :]], dim=-2)
    if name == "Stokes3D-FxUP":
        return torch.cat([stokeslet, (d * ri3[..., None] / pi8)[..., :, None]], dim=-1)
    if name == "Laplace3D-FDxUdU":
        rn = (d * n).sum(-1)
        row_q = torch.cat([ri[..., None], -d * ri3[..., None]], dim=-1)
        row_mu = torch.cat([(rn * ri3)[..., None], n * ri3[..., None] - 3 * d * (rn * ri5)[..., None]], dim=-1)
        return torch.stack([row_q, row_mu], dim=-2) / pi4
    if name == "Helmholtz3D-FxU":      # G = e^{ikr} / (4 pi r), k = ctx[0] + i ctx[1]; (u_re, u_im) = G (f_re, f_im) as complex numbers
        r = r2 * ri
        amp = ri * torch.exp(-ctx[1] * r) / pi4
        gr, gi = amp * torch.cos(ctx[0] * r), amp * torch.sin(ctx[0] * r)
        return torch.stack([torch.stack([gr, gi], dim=-1), torch.stack([-gi, gr], dim=-1)], dim=-2)
    if name.startswith("Yukawa3D"):    # the plugin functor of the tests: e^{-lambda r} / (4 pi r)
        r = r2 * ri
        return (ri * torch.exp(-lam * r) / pi4)[..., None, None]
    raise ValueError(name)


def loss(name, xt, xs, xn, f, w, ctx=None, lam=None, zero=None):
    """L = sum_t sum_k1 w[t,k1] sum_s sum_k0 U[t,s,k0,k1] f[s,k0]; `zero`: a (Nt, Ns) boolean mask of pairs to leave out besides the coincident ones"""
    U = kernel_blocks(name, xt, xs, xn, ctx, lam)
    if zero is not None:
        U = torch.where(zero[..., None, None], torch.zeros_like(U), U)
    return torch.einsum("tk,tsjk,sj->", w, U, f)


def gradients(name, xt, xs, xn, f, w, ctx=None, lam=None, dtype=torch.float64, zero=None):
    """(g_trg, g_src, g_nrm or None, g_f) of L, numpy arrays flattened as the library lays them out, evaluated and differentiated in `dtype` on the
    inputs rounded to it (numpy arrays, flat, as the library takes them)"""
    T = lambda a, k: None if a is None else torch.from_numpy(a).to(dtype).view(-1, k).clone().requires_grad_(True)
    k0, k1 = f.size // (xs.size // 3), w.size // (xt.size // 3)
    t_xt, t_xs, t_xn, t_f = T(xt, 3), T(xs, 3), T(xn, 3), T(f, k0)
    t_w = torch.from_numpy(w).to(dtype).view(-1, k1)
    L = loss(name, t_xt, t_xs, t_xn, t_f, t_w, ctx, lam, zero)
    L.backward()
    out = lambda t: None if t is None else t.grad.numpy().ravel()
    return out(t_xt), out(t_xs), out(t_xn), out(t_f)
