"""Back-propagation through a kernel sum: u = A v_src is linear in the densities, and the gradient of a scalar loss with respect to them
is the transposed sum A^T (dloss/du) — sctl_amd_eval_transpose_device, on the same stream as the forward pass.

    u = sctl_amd.autograd.kernel_sum("Stokes3D-FxUP", r_trg, r_src, None, v_src)      # torch CUDA tensors; v_src.requires_grad
    u.square().sum().backward()                                                      # v_src.grad = A^T (2 u)

Only the densities are differentiated: gradients with respect to the coordinates or the normals need the kernels' derivatives, which this
library does not have, so a coordinate or normal tensor that requires grad is refused instead of silently getting none."""
import torch
from torch.autograd.function import once_differentiable

from . import api


class _KernelSum(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, name, r_trg, r_src, n_src, v_src, digits, ctx):
        fn_ctx.kernel = (name, digits, ctx)
        fn_ctx.save_for_backward(r_trg, r_src, n_src)
        return api.eval_device(name, r_trg.detach(), r_src.detach(), None if n_src is None else n_src.detach(), v_src.detach().contiguous(), digits=digits, ctx=ctx)

    @staticmethod
    @once_differentiable      # the backward runs outside the graph: a double backward (create_graph=True) raises instead of getting no graph
    def backward(fn_ctx, grad_u):
        name, digits, ctx = fn_ctx.kernel
        r_trg, r_src, n_src = fn_ctx.saved_tensors
        g = None
        if fn_ctx.needs_input_grad[4]:
            g = api.eval_transpose_device(name, r_trg, r_src, n_src, grad_u.contiguous(), digits=digits, ctx=ctx)
        return None, None, None, None, g, None, None


def kernel_sum(name, r_trg, r_src, n_src, v_src, digits=-1, ctx=None):
    """GenericKernel::Eval on torch CUDA tensors (a fresh result, Nt*TrgDim values) that autograd can differentiate with respect to v_src."""
    for what, t in (("r_trg", r_trg), ("r_src", r_src), ("n_src", n_src)):
        if t is not None and t.requires_grad:
            raise api.SctlAmdError("kernel_sum differentiates with respect to the densities only: %s requires grad, and gradients with respect to "
                                   "coordinates or normals are not implemented" % what)
    return _KernelSum.apply(name, r_trg, r_src, n_src, v_src, digits, ctx)
