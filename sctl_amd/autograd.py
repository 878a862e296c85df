"""Back-propagation through a kernel sum: u = A v_src is linear in the densities, and the gradient of a scalar loss with respect to them
is the transposed sum A^T (dloss/du) — sctl_amd_eval_transpose_device, on the same stream as the forward pass.

    u = sctl_amd.autograd.kernel_sum("Stokes3D-FxUP", r_trg, r_src, None, v_src)      # torch CUDA tensors; v_src.requires_grad
    u.square().sum().backward()                                                      # v_src.grad = A^T (2 u)

kernel_sum differentiates the densities only, and refuses a coordinate or normal tensor that requires grad instead of silently giving it none.
kernel_sum_geometry differentiates the geometry as well: its backward adds sctl_amd_eval_grad_device, the kernels' derivatives (pair_g), for whichever
of r_trg, r_src, n_src need a gradient.

    u = sctl_amd.autograd.kernel_sum_geometry("Laplace3D-DxU", r_trg, r_src, n_src, v_src)   # any of the four may require grad
    u.square().sum().backward()                                                               # r_trg.grad, r_src.grad, n_src.grad, v_src.grad

kernel_sum_geometry also runs in forward mode: the tangent of u along tangents of any of the four is sctl_amd_eval_jvp_device (pair_j) for the geometry
plus A dv_src.

    u, du = torch.func.jvp(lambda x: sctl_amd.autograd.kernel_sum_geometry("Laplace3D-DxU", x, r_src, n_src, v_src), (r_trg,), (d_trg,))

kernel_sum_densities is kernel_sum for several densities on one geometry: the forward is sctl_amd_eval_densities_device, the backward
sctl_amd_eval_transpose_densities_device, A^T (dloss/dU) for all rows in one pass; densities only.

    U = sctl_amd.autograd.kernel_sum_densities("Stokes3D-FxUP", r_trg, r_src, None, V_src)    # V_src of shape (nd, Ns*SrcDim); U (nd, Nt*TrgDim)
    U.square().sum().backward()                                                      # V_src.grad[m] = A^T (2 U[m])

kernel_sum_densities_geometry differentiates the geometry of such a block as well: its backward adds sctl_amd_eval_grad_densities_device, the
gradients of sum_m <dloss/dU[m], A V_src[m]> for all rows in one pass.

    U = sctl_amd.autograd.kernel_sum_densities_geometry("Stokes3D-DxU", r_trg, r_src, n_src, V_src)   # any of the four may require grad

lists_sum is kernel_sum over the P2P lists of a ListsPlan made with directions="both": the forward is plan.eval_device, the backward
plan.eval_transpose_device; densities only.

    plan = sctl_amd.ListsPlan("Stokes3D-FxU", np.float64, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, directions="both")
    u = sctl_amd.autograd.lists_sum(plan, r_trg, r_src, None, v_src)
    u.square().sum().backward()                                                      # v_src.grad = sum over the lists of A_l^T (2 u)

lists_sum_geometry differentiates the geometry of such a sum as well: its backward adds plan.eval_grad_device (sctl_amd_lists_eval_grad_device), one launch
per side, for whichever of r_trg, r_src, n_src need a gradient.

    u = sctl_amd.autograd.lists_sum_geometry(plan, x, x, None, v_src)                # x.requires_grad: x.grad = g_trg + g_src

lists_sum_densities is lists_sum for several densities: the forward is plan.eval_densities_device, the backward
plan.eval_transpose_densities_device, all gradient rows in one launch per pass; densities only.

    U = sctl_amd.autograd.lists_sum_densities(plan, r_trg, r_src, None, V_src)       # V_src of shape (nd, Ns*SrcDim); U (nd, Nt*TrgDim)

near_apply is NearOp.apply_device (the near-zone correction of a BoundaryIntegralOp, u = N f) with backward NearOp.apply_transpose_device;
potential is DirectOp.eval_potential (ComputePotential: far field, weights, target normals and the attached near field; host tensors) with
backward DirectOp.eval_potential_transpose.  Both differentiate the densities only.

    u = sctl_amd.autograd.near_apply(near_op, f)                                     # torch CUDA tensor f of near_op.density_len values
    u = sctl_amd.autograd.potential(direct_op, f_far, f_near)                        # torch CPU tensors

near_apply_densities and potential_densities are the same for several densities in one pass: NearOp.apply_densities_device with backward
NearOp.apply_transpose_densities_device, DirectOp.eval_potential_densities with backward DirectOp.eval_potential_transpose_densities.

    U = sctl_amd.autograd.near_apply_densities(near_op, F)                           # torch CUDA tensor F of shape (nd, near_op.density_len)
    U = sctl_amd.autograd.potential_densities(direct_op, F_far, F_near)              # torch CPU tensors of shapes (nd, ...)"""
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
            raise api.SctlAmdError("kernel_sum differentiates with respect to the densities only: %s requires grad; kernel_sum_geometry differentiates "
                                   "coordinates and normals too" % what)
    return _KernelSum.apply(name, r_trg, r_src, n_src, v_src, digits, ctx)


class _KernelSumDensities(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, name, r_trg, r_src, n_src, V_src, digits, ctx):
        fn_ctx.kernel = (name, digits, ctx)
        fn_ctx.save_for_backward(r_trg, r_src, n_src)
        return api.eval_densities_device(name, r_trg.detach(), r_src.detach(), None if n_src is None else n_src.detach(), V_src.detach().contiguous(), digits=digits, ctx=ctx)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_U):
        name, digits, ctx = fn_ctx.kernel
        r_trg, r_src, n_src = fn_ctx.saved_tensors
        G = None
        if fn_ctx.needs_input_grad[4]:
            G = api.eval_transpose_densities_device(name, r_trg, r_src, n_src, grad_U.contiguous(), digits=digits, ctx=ctx)
        return None, None, None, None, G, None, None


def kernel_sum_densities(name, r_trg, r_src, n_src, V_src, digits=-1, ctx=None):
    """sctl_amd.eval_densities_device on torch CUDA tensors (a fresh result of shape (nd, Nt*TrgDim)) that autograd can differentiate with respect to
    V_src, of shape (nd, Ns*SrcDim): the backward is eval_transpose_densities_device on the forward's stream, as autograd arranges, and is
    once-differentiable."""
    for what, t in (("r_trg", r_trg), ("r_src", r_src), ("n_src", n_src)):
        if t is not None and t.requires_grad:
            raise api.SctlAmdError("kernel_sum_densities differentiates with respect to the densities only: %s requires grad; "
                                   "kernel_sum_densities_geometry differentiates coordinates and normals too" % what)
    return _KernelSumDensities.apply(name, r_trg, r_src, n_src, V_src, digits, ctx)


class _KernelSumDensitiesGeometry(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, name, r_trg, r_src, n_src, V_src, digits, ctx):
        fn_ctx.kernel = (name, digits, ctx)
        r_trg, r_src, V_src = r_trg.detach().contiguous(), r_src.detach().contiguous(), V_src.detach().contiguous()
        n_src = None if n_src is None else n_src.detach().contiguous()
        fn_ctx.has_normal = n_src is not None
        fn_ctx.shapes = (r_trg.shape, r_src.shape, None if n_src is None else n_src.shape)
        fn_ctx.save_for_backward(*([r_trg, r_src, V_src] + ([n_src] if n_src is not None else [])))
        return api.eval_densities_device(name, r_trg, r_src, n_src, V_src, digits=digits, ctx=ctx)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_U):
        name, digits, ctx = fn_ctx.kernel
        r_trg, r_src, V_src = fn_ctx.saved_tensors[:3]
        n_src = fn_ctx.saved_tensors[3] if fn_ctx.has_normal else None
        grad_U = grad_U.contiguous()
        need = fn_ctx.needs_input_grad
        G_v = api.eval_transpose_densities_device(name, r_trg, r_src, n_src, grad_U, digits=digits, ctx=ctx) if need[4] else None
        want = [what for what, i in (("trg", 1), ("src", 2), ("nrm", 3)) if need[i]]
        g_trg = g_src = g_nrm = None
        if want:
            g = api.eval_grad_densities_device(name, r_trg, r_src, n_src, V_src, grad_U, want=want, digits=digits, ctx=ctx)
            g_trg, g_src, g_nrm = [None if x is None else x.view(shape) for x, shape in zip(g, fn_ctx.shapes)]
        return None, g_trg, g_src, g_nrm, G_v, None, None


def kernel_sum_densities_geometry(name, r_trg, r_src, n_src, V_src, digits=-1, ctx=None):
    """sctl_amd.eval_densities_device on torch CUDA tensors (a fresh result of shape (nd, Nt*TrgDim)) that autograd can differentiate with respect to
    r_trg, r_src, n_src and V_src, of shape (nd, Ns*SrcDim): the backward is eval_transpose_densities_device for V_src and eval_grad_densities_device,
    all rows in one pass, for whichever of the geometry tensors need a gradient.  It runs on the forward's stream, as autograd arranges, and is
    once-differentiable."""
    return _KernelSumDensitiesGeometry.apply(name, r_trg, r_src, n_src, V_src, digits, ctx)


class _KernelSumTangent(torch.autograd.Function):
    """The tangent of _KernelSumGeometry as an operation of its own, so that its tensors arrive as plain CUDA tensors under torch.func.jvp as well:
    eval_jvp_device for the geometry plus eval_device of the density tangent, accumulated into the same tensor.  An absent tangent goes in as null.
    It has neither a backward nor a jvp of its own: differentiating a tangent again (reverse over forward, forward over forward) raises."""
    @staticmethod
    def forward(kernel, r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, d_v):
        name, digits, ctx = kernel
        flat = lambda t: None if t is None else t.detach().contiguous().view(-1)
        du = api.eval_jvp_device(name, r_trg, r_src, n_src, v_src, flat(d_trg), flat(d_src), None if n_src is None else flat(d_nrm), digits=digits, ctx=ctx)
        if d_v is not None:
            api.eval_device(name, r_trg, r_src, n_src, flat(d_v), du, digits=digits, ctx=ctx)
        return du

    @staticmethod
    def setup_context(fn_ctx, inputs, output):
        pass


class _KernelSumGeometry(torch.autograd.Function):
    @staticmethod
    def forward(name, r_trg, r_src, n_src, v_src, digits, ctx):      # contiguous tensors: kernel_sum_geometry made them so, once
        return api.eval_device(name, r_trg.detach(), r_src.detach(), None if n_src is None else n_src.detach(), v_src.detach(), digits=digits, ctx=ctx)

    @staticmethod
    def setup_context(fn_ctx, inputs, output):      # (forward takes no context: torch.func's transforms need the two apart)
        name, r_trg, r_src, n_src, v_src, digits, ctx = inputs
        fn_ctx.kernel = (name, digits, ctx)
        r_trg, r_src, v_src = r_trg.detach(), r_src.detach(), v_src.detach()      # the tensors the forward ran on (views of them: no copy)
        n_src = None if n_src is None else n_src.detach()
        fn_ctx.has_normal = n_src is not None
        fn_ctx.shapes = (r_trg.shape, r_src.shape, None if n_src is None else n_src.shape)
        saved = [r_trg, r_src, v_src] + ([n_src] if n_src is not None else [])
        fn_ctx.save_for_backward(*saved)
        fn_ctx.save_for_forward(*saved)

    @staticmethod
    def jvp(fn_ctx, _name, d_trg, d_src, d_nrm, d_v, _digits, _ctx):
        r_trg, r_src, v_src = fn_ctx.saved_tensors[:3]
        n_src = fn_ctx.saved_tensors[3] if fn_ctx.has_normal else None
        return _KernelSumTangent.apply(fn_ctx.kernel, r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, d_v)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_u):
        name, digits, ctx = fn_ctx.kernel
        r_trg, r_src, v_src = fn_ctx.saved_tensors[:3]
        n_src = fn_ctx.saved_tensors[3] if fn_ctx.has_normal else None
        grad_u = grad_u.contiguous()
        need = fn_ctx.needs_input_grad
        g_v = api.eval_transpose_device(name, r_trg, r_src, n_src, grad_u, digits=digits, ctx=ctx) if need[4] else None
        want = [what for what, i in (("trg", 1), ("src", 2), ("nrm", 3)) if need[i]]
        g_trg = g_src = g_nrm = None
        if want:
            g = api.eval_grad_device(name, r_trg, r_src, n_src, v_src, grad_u, want=want, digits=digits, ctx=ctx)
            g_trg, g_src, g_nrm = [None if x is None else x.view(shape) for x, shape in zip(g, fn_ctx.shapes)]
        return None, g_trg, g_src, g_nrm, g_v, None, None


def kernel_sum_geometry(name, r_trg, r_src, n_src, v_src, digits=-1, ctx=None):
    """GenericKernel::Eval on torch CUDA tensors (a fresh result, Nt*TrgDim values) that autograd can differentiate with respect to r_trg, r_src,
    n_src and v_src.  The backward runs on the forward's stream, as autograd arranges, and is once-differentiable.  Forward mode
    (torch.func.jvp, torch.autograd.forward_ad) works too: the tangent is eval_jvp_device for the geometry plus eval_device of the density tangent.
    The tangent itself is not differentiable: reverse over forward (a backward through the result of a jvp) and forward over forward raise.  A
    non-contiguous input is copied once, here."""
    c = lambda t: None if t is None else t.contiguous()
    return _KernelSumGeometry.apply(name, c(r_trg), c(r_src), c(n_src), c(v_src), digits, ctx)


class _ListsSum(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, plan, r_trg, r_src, n_src, v_src, digits):
        fn_ctx.plan, fn_ctx.digits = plan, digits
        fn_ctx.save_for_backward(r_trg, r_src, n_src)
        return plan.eval_device(r_trg.detach(), r_src.detach(), None if n_src is None else n_src.detach(), v_src.detach().contiguous(), digits=digits)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_u):
        r_trg, r_src, n_src = fn_ctx.saved_tensors
        g = None
        if fn_ctx.needs_input_grad[4]:
            g = fn_ctx.plan.eval_transpose_device(r_trg, r_src, n_src, grad_u.contiguous(), digits=fn_ctx.digits)
        return None, None, None, None, g, None


def lists_sum(plan, r_trg, r_src, n_src, v_src, digits=-1):
    """plan.eval_device on torch CUDA tensors (a fresh result, Nt*TrgDim values) that autograd can differentiate with respect to v_src: the backward is
    plan.eval_transpose_device on the forward's stream, as autograd arranges, and is once-differentiable.  The plan must hold both directions."""
    both = api.LISTS_FORWARD | api.LISTS_TRANSPOSE
    if plan.directions != both:
        raise api.SctlAmdError('lists_sum needs a ListsPlan made with directions="both": the backward pass is the transposed list sum')
    for what, t in (("r_trg", r_trg), ("r_src", r_src), ("n_src", n_src)):
        if t is not None and t.requires_grad:
            raise api.SctlAmdError("lists_sum differentiates with respect to the densities only: %s requires grad" % what)
    return _ListsSum.apply(plan, r_trg, r_src, n_src, v_src, digits)


class _ListsSumGeometry(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, plan, r_trg, r_src, n_src, v_src, digits):
        fn_ctx.plan, fn_ctx.digits = plan, digits
        # one tensor for both point sets stays one tensor (one address): the list kernels then know that every box meets its own points
        same = r_src is r_trg or (r_src.data_ptr() == r_trg.data_ptr() and r_src.shape == r_trg.shape)
        r_trg = r_trg.detach().contiguous()
        r_src = r_trg if same else r_src.detach().contiguous()
        v_src = v_src.detach().contiguous()
        n_src = None if n_src is None else n_src.detach().contiguous()
        fn_ctx.same, fn_ctx.has_normal = same, n_src is not None
        fn_ctx.shapes = (r_trg.shape, r_src.shape, None if n_src is None else n_src.shape)
        fn_ctx.save_for_backward(*([r_trg, v_src] + ([] if same else [r_src]) + ([n_src] if n_src is not None else [])))
        return plan.eval_device(r_trg, r_src, n_src, v_src, digits=digits)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_u):
        saved = list(fn_ctx.saved_tensors)
        r_trg, v_src = saved[0], saved[1]
        r_src = r_trg if fn_ctx.same else saved[2]
        n_src = saved[-1] if fn_ctx.has_normal else None
        grad_u = grad_u.contiguous()
        need = fn_ctx.needs_input_grad
        g_v = fn_ctx.plan.eval_transpose_device(r_trg, r_src, n_src, grad_u, digits=fn_ctx.digits) if need[4] else None
        want = [what for what, i in (("trg", 1), ("src", 2), ("nrm", 3)) if need[i]]
        g_trg = g_src = g_nrm = None
        if want:
            g = fn_ctx.plan.eval_grad_device(r_trg, r_src, n_src, v_src, grad_u, want=want, digits=fn_ctx.digits)
            g_trg, g_src, g_nrm = [None if x is None else x.view(shape) for x, shape in zip(g, fn_ctx.shapes)]
        return None, g_trg, g_src, g_nrm, g_v, None


def lists_sum_geometry(plan, r_trg, r_src, n_src, v_src, digits=-1):
    """plan.eval_device on torch CUDA tensors (a fresh result, Nt*TrgDim values) that autograd can differentiate with respect to r_trg, r_src, n_src
    and v_src: the backward is plan.eval_transpose_device for v_src and plan.eval_grad_device — one launch per side, only the sides whose inputs need
    a gradient — for the geometry.  With one tensor as r_trg and r_src (the self-interaction case) autograd adds the two coordinate gradients.  It
    runs on the forward's stream, as autograd arranges, and is once-differentiable.  The plan must hold both directions."""
    both = api.LISTS_FORWARD | api.LISTS_TRANSPOSE
    if plan.directions != both:
        raise api.SctlAmdError('lists_sum_geometry needs a ListsPlan made with directions="both": the backward pass walks the transposed work list')
    return _ListsSumGeometry.apply(plan, r_trg, r_src, n_src, v_src, digits)


class _ListsSumDensities(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, plan, r_trg, r_src, n_src, V_src, digits):
        fn_ctx.plan, fn_ctx.digits = plan, digits
        fn_ctx.save_for_backward(r_trg, r_src, n_src)
        return plan.eval_densities_device(r_trg.detach(), r_src.detach(), None if n_src is None else n_src.detach(), V_src.detach().contiguous(), digits=digits)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_U):
        r_trg, r_src, n_src = fn_ctx.saved_tensors
        g = None
        if fn_ctx.needs_input_grad[4]:
            g = fn_ctx.plan.eval_transpose_densities_device(r_trg, r_src, n_src, grad_U.contiguous(), digits=fn_ctx.digits)
        return None, None, None, None, g, None


def lists_sum_densities(plan, r_trg, r_src, n_src, V_src, digits=-1):
    """plan.eval_densities_device on torch CUDA tensors (a fresh result of shape (nd, Nt*TrgDim)) that autograd can differentiate with respect to V_src,
    of shape (nd, Ns*SrcDim): the backward is plan.eval_transpose_densities_device on the incoming gradient rows, on the forward's stream, as autograd
    arranges, and is once-differentiable.  The plan must hold both directions."""
    both = api.LISTS_FORWARD | api.LISTS_TRANSPOSE
    if plan.directions != both:
        raise api.SctlAmdError('lists_sum_densities needs a ListsPlan made with directions="both": the backward pass is the transposed list sum')
    for what, t in (("r_trg", r_trg), ("r_src", r_src), ("n_src", n_src)):
        if t is not None and t.requires_grad:
            raise api.SctlAmdError("lists_sum_densities differentiates with respect to the densities only: %s requires grad" % what)
    return _ListsSumDensities.apply(plan, r_trg, r_src, n_src, V_src, digits)


class _NearApply(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, op, F):
        fn_ctx.op = op
        return op.apply_device(F.detach().contiguous(), torch.zeros(op.potential_len, dtype=F.dtype, device=F.device))

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_u):
        op = fn_ctx.op
        return None, op.apply_transpose_device(grad_u.contiguous(), torch.zeros(op.density_len, dtype=grad_u.dtype, device=grad_u.device))


def near_apply(op, F):
    """NearOp.apply_device from zero on a torch CUDA tensor (a fresh result, potential_len values) that autograd can differentiate with
    respect to the density F: the backward is NearOp.apply_transpose_device on the forward's stream, and is once-differentiable."""
    return _NearApply.apply(op, F)


class _Potential(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, op, f_far, f_near, digits):
        fn_ctx.op, fn_ctx.digits = op, digits
        u = op.eval_potential(f_far.detach().contiguous().numpy(), f_near.detach().contiguous().numpy(), digits=digits)
        return torch.from_numpy(u)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_u):
        g_far, g_near = fn_ctx.op.eval_potential_transpose(grad_u.contiguous().numpy(), digits=fn_ctx.digits)
        need = fn_ctx.needs_input_grad
        return None, torch.from_numpy(g_far) if need[1] else None, torch.from_numpy(g_near) if need[2] else None, None


def potential(op, f_far, f_near, digits=-1):
    """DirectOp.eval_potential on torch HOST tensors (the operator handle moves densities and potential itself) that autograd can differentiate
    with respect to the far-field and the near-field density: the backward is DirectOp.eval_potential_transpose at the same digits."""
    for what, t in (("f_far", f_far), ("f_near", f_near)):
        if t.is_cuda:
            raise api.SctlAmdError("potential takes host tensors: %s is a CUDA tensor" % what)
    return _Potential.apply(op, f_far, f_near, digits)


class _NearApplyDensities(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, op, F):
        fn_ctx.op = op
        return op.apply_densities_device(F.detach().contiguous(), torch.zeros((F.shape[0], op.potential_len), dtype=F.dtype, device=F.device))

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_U):
        op = fn_ctx.op
        return None, op.apply_transpose_densities_device(grad_U.contiguous(), torch.zeros((grad_U.shape[0], op.density_len), dtype=grad_U.dtype, device=grad_U.device))


def near_apply_densities(op, F):
    """NearOp.apply_densities_device from zero on a torch CUDA tensor of shape (nd, density_len) (a fresh result of shape (nd, potential_len)) that
    autograd can differentiate with respect to the densities F: the backward is NearOp.apply_transpose_densities_device on the forward's stream,
    and is once-differentiable."""
    if F.dim() != 2 or F.shape[1] != op.density_len:
        raise api.SctlAmdError("densities must have shape (nd, %d)" % op.density_len)
    return _NearApplyDensities.apply(op, F)


class _PotentialDensities(torch.autograd.Function):
    @staticmethod
    def forward(fn_ctx, op, F_far, F_near, digits):
        fn_ctx.op, fn_ctx.digits = op, digits
        U = op.eval_potential_densities(F_far.detach().contiguous().numpy(), F_near.detach().contiguous().numpy(), digits=digits)
        return torch.from_numpy(U)

    @staticmethod
    @once_differentiable
    def backward(fn_ctx, grad_U):
        G_far, G_near = fn_ctx.op.eval_potential_transpose_densities(grad_U.contiguous().numpy(), digits=fn_ctx.digits)
        need = fn_ctx.needs_input_grad
        return None, torch.from_numpy(G_far) if need[1] else None, torch.from_numpy(G_near) if need[2] else None, None


def potential_densities(op, F_far, F_near, digits=-1):
    """DirectOp.eval_potential_densities on torch HOST tensors of shapes (nd, Ns*SrcDim) and (nd, near density length) that autograd can
    differentiate with respect to both: the backward is DirectOp.eval_potential_transpose_densities at the same digits."""
    for what, t in (("F_far", F_far), ("F_near", F_near)):
        if t.is_cuda:
            raise api.SctlAmdError("potential_densities takes host tensors: %s is a CUDA tensor" % what)
    return _PotentialDensities.apply(op, F_far, F_near, digits)
