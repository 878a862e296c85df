"""ctypes binding of include/sctl_amd.h and a GenericKernel mirror of the reference's kernel objects.

Names, argument order and semantics follow the reference (file:line relative to /root/reference):
  GenericKernel.Eval(v_trg, r_trg, r_src, n_src, v_src)   include/sctl/generic-kernel.hpp:123, generic-kernel.txx:76-189
  GenericKernel.KernelMatrix(M, Xt, Xs, Xn)               include/sctl/generic-kernel.hpp:135, generic-kernel.txx:191-307
  SrcDim / TrgDim / NormalDim / CoordDim / Name / FLOPS   include/sctl/generic-kernel.hpp:59-84, kernel_functions.hpp:16-22
numpy arrays go through the host-buffer entry points, torch CUDA tensors through the device-resident ones
(on torch's current stream).  A missing or failing library raises; nothing is computed on the CPU here.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

F64, F32 = 0, 1
KERNEL_NAMES = ["Laplace3D-FxU", "Laplace3D-DxU", "Laplace3D-FxdU", "Stokes3D-FxU", "Stokes3D-DxU", "Stokes3D-FxT", "Stokes3D-FSxU",
                "Stokes3D-FxUP", "Laplace3D-FDxUdU", "Helmholtz3D-FxU"]

# every symbol include/sctl_amd.h declares (tests/test_boundary.py checks the header against this list and the .so)
SYMBOLS = ["sctl_amd_version", "sctl_amd_last_error", "sctl_amd_device_count", "sctl_amd_init", "sctl_amd_finalize", "sctl_amd_kernel_id", "sctl_amd_kernel_name",
           "sctl_amd_kernel_info", "sctl_amd_flops_per_pair", "sctl_amd_eval_device", "sctl_amd_eval_device_slab", "sctl_amd_eval_host", "sctl_amd_eval_host_multi",
           "sctl_amd_kernel_matrix_device", "sctl_amd_kernel_matrix_host", "sctl_amd_kernel_matrix_batch_host", "sctl_amd_counters", "sctl_amd_reset_counters", "sctl_amd_trim",
           "sctl_amd_eval_plan", "sctl_amd_eval_path", "sctl_amd_eval_pipe", "sctl_amd_op_create", "sctl_amd_op_set_targets",
           "sctl_amd_op_set_sources", "sctl_amd_op_set_source_weights", "sctl_amd_op_set_target_normals", "sctl_amd_op_eval", "sctl_amd_op_destroy", "sctl_amd_near_create", "sctl_amd_near_apply_host",
           "sctl_amd_near_apply_device", "sctl_amd_near_info", "sctl_amd_near_destroy", "sctl_amd_num_kernels", "sctl_amd_register_kernel", "sctl_amd_load_plugin",
           "sctl_amd_set_debug", "sctl_amd_comm_create", "sctl_amd_comm_info", "sctl_amd_comm_allgatherv_host", "sctl_amd_comm_barrier", "sctl_amd_comm_selftest", "sctl_amd_comm_destroy",
           "sctl_amd_op_set_sources_dist", "sctl_amd_op_eval_dist", "sctl_amd_op_set_near", "sctl_amd_op_eval_potential", "sctl_amd_lists_create", "sctl_amd_lists_eval_device", "sctl_amd_lists_eval_host", "sctl_amd_lists_info", "sctl_amd_lists_destroy",
           "sctl_amd_eval_lists_device", "sctl_amd_eval_lists_host", "sctl_amd_eval_densities_device", "sctl_amd_eval_densities_host", "sctl_amd_op_eval_densities",
           "sctl_amd_eval_densities_plan", "sctl_amd_near_apply_densities_host", "sctl_amd_near_apply_densities_device", "sctl_amd_op_eval_potential_densities",
           "sctl_amd_lists_eval_densities_device", "sctl_amd_lists_eval_densities_host", "sctl_amd_eval_lists_densities_host",
           "sctl_amd_eval_transpose_device", "sctl_amd_eval_transpose_host", "sctl_amd_eval_transpose_plan",
           "sctl_amd_lists_create_directions", "sctl_amd_lists_eval_transpose_device", "sctl_amd_lists_eval_transpose_host", "sctl_amd_lists_transpose_info",
           "sctl_amd_eval_lists_transpose_host",
           "sctl_amd_lists_eval_transpose_densities_device", "sctl_amd_lists_eval_transpose_densities_host", "sctl_amd_eval_lists_transpose_densities_host",
           "sctl_amd_eval_grad_device", "sctl_amd_eval_grad_host", "sctl_amd_eval_grad_plan",
           "sctl_amd_near_apply_transpose_host", "sctl_amd_near_apply_transpose_device", "sctl_amd_op_eval_transpose", "sctl_amd_op_eval_potential_transpose",
           "sctl_amd_eval_transpose_densities_device", "sctl_amd_eval_transpose_densities_host", "sctl_amd_eval_transpose_densities_plan",
           "sctl_amd_near_apply_transpose_densities_host", "sctl_amd_near_apply_transpose_densities_device", "sctl_amd_op_eval_transpose_densities",
           "sctl_amd_op_eval_potential_transpose_densities",
           "sctl_amd_eval_grad_densities_device", "sctl_amd_eval_grad_densities_host", "sctl_amd_eval_grad_densities_plan",
           "sctl_amd_lists_eval_grad_device", "sctl_amd_lists_eval_grad_host", "sctl_amd_eval_lists_grad_host",
           "sctl_amd_eval_jvp_device", "sctl_amd_eval_jvp_host", "sctl_amd_eval_jvp_plan"]


class SctlAmdError(RuntimeError):
    pass


def library_path():
    # SCTL_AMD_LIB: explicit path of another build of the same library (kernel experiments under tools/)
    return os.environ.get("SCTL_AMD_LIB") or os.path.join(_HERE, "libsctl_amd.so")


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (soname libamdhip64.so.7, found through its
    RPATH); libsctl_amd.so asks for libamdhip64.so.7 and, loaded first, gets /opt/rocm's copy — a later `import torch` then
    loads a SECOND runtime under the other file name and finds no GPU ("No HIP GPUs are available").  Loading torch's copy
    first makes both resolve to it, whichever side is used first.  Skipped when torch is absent or already imported."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("SCTL_AMD_OWN_HIP_RUNTIME") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for loc in (spec.submodule_search_locations or []) if spec else []:
        cand = os.path.join(loc, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return


def lib():
    """The loaded C-ABI library.  Raises if it has not been built: there is no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise SctlAmdError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                           "`make -C sctl_amd/csrc` (hipcc, gfx950); sctl_amd has no CPU fallback" % path)
    _share_torch_hip_runtime()
    L = C.CDLL(path)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.sctl_amd_last_error.restype = C.c_char_p
    L.sctl_amd_kernel_name.restype = C.c_char_p
    L.sctl_amd_kernel_id.argtypes = [C.c_char_p]
    L.sctl_amd_kernel_info.argtypes = [ci] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.sctl_amd_eval_device.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_device_slab.argtypes = [ci, ci, i64, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_host.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_eval_host_multi.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, C.POINTER(C.c_int), ci]
    L.sctl_amd_kernel_matrix_device.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_kernel_matrix_host.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_kernel_matrix_batch_host.argtypes = [ci, ci, i64, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_counters.argtypes = [C.POINTER(i64), C.POINTER(i64)]
    L.sctl_amd_counters.restype = None
    L.sctl_amd_reset_counters.restype = None
    L.sctl_amd_trim.restype = None
    pi64 = C.POINTER(i64)
    L.sctl_amd_near_create.argtypes = [ci, ci, i64, ci, ci, vp, vp, vp, vp, i64, vp, vp, vp, C.POINTER(vp)]
    L.sctl_amd_near_apply_host.argtypes = [vp, vp, vp]
    L.sctl_amd_near_apply_device.argtypes = [vp, vp, vp, vp]
    L.sctl_amd_near_info.argtypes = [vp, pi64, pi64, pi64, pi64, pi64]
    L.sctl_amd_near_destroy.argtypes = [vp]
    L.sctl_amd_near_destroy.restype = None
    L.sctl_amd_eval_plan.argtypes = [ci, ci, i64, i64, i64, ci, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64)]
    L.sctl_amd_eval_path.argtypes = [ci, ci, i64, i64, i64]
    L.sctl_amd_eval_pipe.argtypes = [ci, ci, i64, i64, i64, ci]
    L.sctl_amd_op_create.argtypes = [ci, ci, C.POINTER(C.c_int), ci, C.POINTER(vp)]
    L.sctl_amd_op_set_targets.argtypes = [vp, i64, vp]
    L.sctl_amd_op_set_sources.argtypes = [vp, i64, vp, vp]
    L.sctl_amd_op_set_source_weights.argtypes = [vp, vp]
    L.sctl_amd_op_set_target_normals.argtypes = [vp, vp]
    L.sctl_amd_op_eval.argtypes = [vp, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_op_destroy.argtypes = [vp]
    L.sctl_amd_op_destroy.restype = None
    L.sctl_amd_op_set_near.argtypes = [vp, ci, ci, i64, vp, vp, vp, vp, vp, vp, vp]
    L.sctl_amd_op_eval_potential.argtypes = [vp, vp, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_load_plugin.argtypes = [C.c_char_p]
    L.sctl_amd_finalize.restype = None
    L.sctl_amd_lists_create.argtypes = [ci, ci, ci, i64, vp, vp, vp, vp, i64, i64, C.POINTER(vp)]
    L.sctl_amd_lists_eval_device.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_host.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sctl_amd_lists_info.argtypes = [vp, pi64, pi64, pi64]
    L.sctl_amd_lists_destroy.argtypes = [vp]
    L.sctl_amd_lists_destroy.restype = None
    L.sctl_amd_eval_lists_host.argtypes = [ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_eval_lists_device.argtypes = [ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_densities_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_densities_host.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sctl_amd_eval_lists_densities_host.argtypes = [ci, ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_eval_densities_device.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_densities_host.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_op_eval_densities.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_near_apply_densities_host.argtypes = [vp, ci, vp, vp]
    L.sctl_amd_near_apply_densities_device.argtypes = [vp, ci, vp, vp, vp]
    L.sctl_amd_op_eval_potential_densities.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_eval_densities_plan.argtypes = [ci, ci, ci, i64, i64, ci] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(i64)] * 2
    L.sctl_amd_lists_create_directions.argtypes = [ci, ci, ci, i64, vp, vp, vp, vp, i64, i64, ci, C.POINTER(vp)]
    L.sctl_amd_lists_eval_transpose_device.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_transpose_host.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sctl_amd_lists_transpose_info.argtypes = [vp, pi64, pi64, pi64]
    L.sctl_amd_eval_lists_transpose_host.argtypes = [ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_lists_eval_transpose_densities_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_transpose_densities_host.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sctl_amd_eval_lists_transpose_densities_host.argtypes = [ci, ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_eval_transpose_device.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_transpose_host.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    L.sctl_amd_eval_transpose_plan.argtypes = [ci, ci, i64, i64, ci, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)]
    L.sctl_amd_eval_transpose_densities_device.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_transpose_densities_host.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    L.sctl_amd_eval_transpose_densities_plan.argtypes = [ci, ci, ci, i64, i64, ci] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(i64)] * 2
    L.sctl_amd_eval_grad_device.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_grad_host.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    L.sctl_amd_eval_grad_plan.argtypes = [ci, ci, i64, i64, ci] + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)] * 2
    L.sctl_amd_eval_grad_densities_device.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_grad_densities_host.argtypes = [ci, ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    L.sctl_amd_eval_grad_densities_plan.argtypes = [ci, ci, ci, i64, i64, ci] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_int), C.POINTER(i64)] * 2
    L.sctl_amd_eval_jvp_device.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_eval_jvp_host.argtypes = [ci, ci, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci]
    L.sctl_amd_eval_jvp_plan.argtypes = [ci, ci, i64, i64, ci, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(i64)]
    L.sctl_amd_lists_eval_grad_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp]
    L.sctl_amd_lists_eval_grad_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci]
    L.sctl_amd_eval_lists_grad_host.argtypes = [ci, ci, i64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci]
    L.sctl_amd_near_apply_transpose_host.argtypes = [vp, vp, vp]
    L.sctl_amd_near_apply_transpose_device.argtypes = [vp, vp, vp, vp]
    L.sctl_amd_op_eval_transpose.argtypes = [vp, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_op_eval_potential_transpose.argtypes = [vp, vp, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_near_apply_transpose_densities_host.argtypes = [vp, ci, vp, vp]
    L.sctl_amd_near_apply_transpose_densities_device.argtypes = [vp, ci, vp, vp, vp]
    L.sctl_amd_op_eval_transpose_densities.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci]
    L.sctl_amd_op_eval_potential_transpose_densities.argtypes = [vp, ci, vp, vp, vp, ci, ci, vp, ci]
    _LIB = L
    return L


def last_error():
    return lib().sctl_amd_last_error().decode()


def _check(rc, what):
    if rc != 0:
        raise SctlAmdError("%s failed with status %d: %s" % (what, rc, last_error()))


def init():
    """Touch every visible GPU now (optional): returns their number."""
    n = lib().sctl_amd_init()
    if n < 0:
        raise SctlAmdError("init failed with status %d: %s" % (n, last_error()))
    return n


def finalize():
    """Give back everything the library keeps between calls (optional; it stays usable)."""
    lib().sctl_amd_finalize()


def device_count():
    return lib().sctl_amd_device_count()


def kernel_id(name):
    """Device kernel id for a functor Name(), or raises KeyError (the 'is it supported' query)."""
    k = name if isinstance(name, int) else lib().sctl_amd_kernel_id(name.encode())
    if k < 0 or k >= lib().sctl_amd_num_kernels():
        raise KeyError("kernel %r is not implemented on the device" % (name,))
    return k


def load_plugin(path):
    """dlopen a kernel plugin (a user functor compiled against include/sctl_amd/device/kernel_plugin.hpp): returns the names it registered."""
    n0 = lib().sctl_amd_num_kernels()
    rc = lib().sctl_amd_load_plugin(os.fspath(path).encode())
    if rc < 0:
        raise SctlAmdError("load_plugin(%s) failed with status %d: %s" % (path, rc, last_error()))
    return [lib().sctl_amd_kernel_name(i).decode() for i in range(n0, n0 + rc)]


_INFO_CACHE = {}


def kernel_info(name):
    """Shape table of a kernel (by Name() or id).  Cached: a kernel's entry never changes once registered, and the evaluation wrappers
    ask for it on every call (three ctypes round trips otherwise — visible in the step time of 2^14-point problems)."""
    hit = _INFO_CACHE.get(name)
    if hit is not None:
        return hit
    info = _kernel_info_uncached(name)
    _INFO_CACHE[name] = _INFO_CACHE[info["id"]] = _INFO_CACHE[info["name"]] = info
    return info


def _kernel_info_uncached(name):
    k = kernel_id(name)
    v = [C.c_int() for _ in range(4)]
    sc, cb = C.c_double(), C.c_int()
    _check(lib().sctl_amd_kernel_info(k, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(sc), C.byref(cb)), "kernel_info")
    return dict(id=k, name=lib().sctl_amd_kernel_name(k).decode(), k0=v[0].value, k1=v[1].value, nd=v[2].value, flops=v[3].value,
                scale=sc.value, ctx_bytes=cb.value)


def flops_per_pair(name):
    return lib().sctl_amd_flops_per_pair(kernel_id(name))


def plan(name, real, Nt, Ns, digits=-1, nt_whole=0):
    t, s = C.c_int(), C.c_int()
    wg, ws = C.c_int64(), C.c_int64()
    _check(lib().sctl_amd_eval_plan(kernel_id(name), real, Nt, Ns, nt_whole, digits, C.byref(t), C.byref(s), C.byref(wg), C.byref(ws)), "eval_plan")
    path = lib().sctl_amd_eval_path(kernel_id(name), real, Nt, Ns, nt_whole)
    pipe = lib().sctl_amd_eval_pipe(kernel_id(name), real, Nt, Ns, nt_whole, digits)
    return dict(trg_per_lane=t.value, src_splits=s.value, workgroups=wg.value, workspace_bytes=ws.value,
                path="tile-centred" if (path == 1 and pipe >= 1) else "exact",     # (eval_path answers for the default accuracy, eval_pipe for `digits`)
                pipe="bf16 matrix cores (r^2) + vector pipe (rsqrt, accumulate)" if pipe == 2 else "vector pipe")


def plan_densities(name, real, nd, Nt, Ns, digits=-1):
    """Launch plan of an nd-density evaluation (sctl_amd_eval_densities_plan): densities per pass, passes, and of the first pass targets per
    lane, source splits, workgroups; the largest partial-sum workspace of any pass."""
    v = [C.c_int() for _ in range(4)]
    wg, ws = C.c_int64(), C.c_int64()
    _check(lib().sctl_amd_eval_densities_plan(kernel_id(name), real, nd, Nt, Ns, digits, *[C.byref(x) for x in v], C.byref(wg), C.byref(ws)), "eval_densities_plan")
    return dict(densities_per_pass=v[0].value, passes=v[1].value, trg_per_lane=v[2].value, src_splits=v[3].value, workgroups=wg.value, workspace_bytes=ws.value)


def plan_transpose(name, real, Nt, Ns, digits=-1):
    """Launch plan of a transposed evaluation (sctl_amd_eval_transpose_plan): sources per lane, target splits, partial-sum workspace of one launch."""
    t, s = C.c_int(), C.c_int()
    ws = C.c_int64()
    _check(lib().sctl_amd_eval_transpose_plan(kernel_id(name), real, Nt, Ns, digits, C.byref(t), C.byref(s), C.byref(ws)), "eval_transpose_plan")
    return dict(src_per_lane=t.value, splits=s.value, workspace_bytes=ws.value)


def plan_transpose_densities(name, real, nd, Nt, Ns, digits=-1):
    """Launch plan of a transposed evaluation of nd weight vectors (sctl_amd_eval_transpose_densities_plan): weight vectors per pass, passes, and of
    the first pass sources per lane, target splits, workgroups; the largest partial-sum workspace of any pass."""
    v = [C.c_int() for _ in range(4)]
    wg, ws = C.c_int64(), C.c_int64()
    _check(lib().sctl_amd_eval_transpose_densities_plan(kernel_id(name), real, nd, Nt, Ns, digits, *[C.byref(x) for x in v], C.byref(wg), C.byref(ws)),
           "eval_transpose_densities_plan")
    return dict(vectors_per_pass=v[0].value, passes=v[1].value, src_per_lane=v[2].value, splits=v[3].value, workgroups=wg.value, workspace_bytes=ws.value)


def plan_grad(name, real, Nt, Ns, digits=-1):
    """Launch plan of a gradient evaluation (sctl_amd_eval_grad_plan), per pass ("trg": the targets own the sums, "src": the sources do): owners per
    lane, splits of the streamed range, partial-sum workspace of one launch."""
    v = [C.c_int(), C.c_int(), C.c_int64(), C.c_int(), C.c_int(), C.c_int64()]
    _check(lib().sctl_amd_eval_grad_plan(kernel_id(name), real, Nt, Ns, digits, *[C.byref(x) for x in v]), "eval_grad_plan")
    return dict(trg=dict(per_lane=v[0].value, splits=v[1].value, workspace_bytes=v[2].value),
                src=dict(per_lane=v[3].value, splits=v[4].value, workspace_bytes=v[5].value))


def plan_grad_densities(name, real, nd, Nt, Ns, digits=-1):
    """Launch plan of a gradient evaluation of nd density / weight rows (sctl_amd_eval_grad_densities_plan): rows per pass of the widest pass, passes,
    and per side ("trg", "src") the splits of the streamed range of the first pass and the largest partial-sum workspace of one launch."""
    v = [C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int(), C.c_int64()]
    _check(lib().sctl_amd_eval_grad_densities_plan(kernel_id(name), real, nd, Nt, Ns, digits, *[C.byref(x) for x in v]), "eval_grad_densities_plan")
    return dict(rows_per_pass=v[0].value, passes=v[1].value, trg=dict(splits=v[2].value, workspace_bytes=v[3].value),
                src=dict(splits=v[4].value, workspace_bytes=v[5].value))


def plan_jvp(name, real, Nt, Ns, digits=-1):
    """Launch plan of a tangent evaluation (sctl_amd_eval_jvp_plan): targets per lane, splits of the source range, partial-sum workspace of one launch."""
    t, sp, ws = C.c_int(), C.c_int(), C.c_int64()
    _check(lib().sctl_amd_eval_jvp_plan(kernel_id(name), real, Nt, Ns, digits, C.byref(t), C.byref(sp), C.byref(ws)), "eval_jvp_plan")
    return dict(per_lane=t.value, splits=sp.value, workspace_bytes=ws.value)


def counters():
    p, f = C.c_int64(), C.c_int64()
    lib().sctl_amd_counters(C.byref(p), C.byref(f))
    return dict(pair_interactions=p.value, sctl_flops=f.value)


def reset_counters():
    lib().sctl_amd_reset_counters()


def trim():
    """Release the device scratch memory cached per (device, stream)."""
    lib().sctl_amd_trim()


def _ctx_blob(info, ctx):
    if info["ctx_bytes"] == 0:
        return None, None, 0
    if ctx is None:
        raise SctlAmdError("%s needs a context of %d bytes (e.g. the complex wavenumber)" % (info["name"], info["ctx_bytes"]))
    buf = np.ascontiguousarray(ctx, dtype=np.float64)
    return buf, buf.ctypes.data_as(C.c_void_p), buf.nbytes


def _real_of(dtype):
    dt = np.dtype(dtype)
    if dt == np.float64:
        return F64
    if dt == np.float32:
        return F32
    raise SctlAmdError("only float64 and float32 are supported, got %s" % dt)


def _np_ptr(a, dt, n, what):
    if n == 0:
        return None
    if a is None or a.dtype != dt or a.size != n or not a.flags["C_CONTIGUOUS"]:
        raise SctlAmdError("%s must be a contiguous %s array of %d values" % (what, np.dtype(dt).name, n))
    return a.ctypes.data_as(C.c_void_p)


def eval_host(name, r_trg, r_src, n_src, v_src, v_trg=None, digits=-1, ctx=None, device=0, devices=None):
    """GenericKernel::Eval on host (numpy) arrays.  v_trg of the right size is ACCUMULATED into
    (generic-kernel.txx:184); any other size (or None) gives a fresh zeroed result (generic-kernel.txx:98-101)."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    if v_trg is None or v_trg.size != Nt * info["k1"]:
        v_trg = np.zeros(Nt * info["k1"], dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    args = [info["id"], real, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
            _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(v_src, dt, Ns * info["k0"], "v_src"),
            _np_ptr(v_trg, dt, Nt * info["k1"], "v_trg"), digits, cp, cb]
    if devices is None:
        _check(lib().sctl_amd_eval_host(*args, device), "eval_host")
    else:
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().sctl_amd_eval_host_multi(*args, devs, len(devices)), "eval_host_multi")
    return v_trg


def eval_densities_host(name, r_trg, r_src, n_src, V_src, V_trg=None, digits=-1, ctx=None, device=0):
    """nd densities against one geometry (sctl_amd_eval_densities_host) on numpy arrays: V_src of shape (nd, Ns*SrcDim), returns
    (nd, Nt*TrgDim).  A V_trg of that shape is accumulated into; None (or another shape) gives a fresh zeroed result."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    if V_src.ndim != 2 or V_src.shape[1] != Ns * info["k0"]:
        raise SctlAmdError("V_src must have shape (nd, %d)" % (Ns * info["k0"]))
    nd = V_src.shape[0]
    if V_trg is None or V_trg.shape != (nd, Nt * info["k1"]):
        V_trg = np.zeros((nd, Nt * info["k1"]), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_eval_densities_host(info["id"], real, nd, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                              _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(V_src, dt, nd * Ns * info["k0"], "V_src"),
                                              _np_ptr(V_trg, dt, nd * Nt * info["k1"], "V_trg"), digits, cp, cb, device), "eval_densities_host")
    return V_trg


def eval_densities_device(name, r_trg, r_src, n_src, V_src, V_trg=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_densities_device), enqueued on `stream` (default: torch's current stream);
    V_src of shape (nd, Ns*SrcDim), V_trg (nd, Nt*TrgDim) accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if V_src.dim() != 2 or V_src.shape[1] != Ns * info["k0"]:
        raise SctlAmdError("V_src must have shape (nd, %d)" % (Ns * info["k0"]))
    nd = V_src.shape[0]
    if V_trg is None or tuple(V_trg.shape) != (nd, Nt * info["k1"]):
        V_trg = torch.zeros((nd, Nt * info["k1"]), dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_densities_device(info["id"], real, nd, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                                    _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(V_src, tdt, nd * Ns * info["k0"], "V_src"),
                                                    _t_ptr(V_trg, tdt, nd * Nt * info["k1"], "V_trg"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
               "eval_densities_device")
    return V_trg


def _t_ptr(t, torch_dtype, n, what):
    if n == 0:
        return None
    if t is None or t.dtype != torch_dtype or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
        raise SctlAmdError("%s must be a contiguous CUDA tensor of %d %s values" % (what, n, torch_dtype))
    return C.c_void_p(t.data_ptr())


def eval_device(name, r_trg, r_src, n_src, v_src, v_trg=None, digits=-1, ctx=None, stream=None, nt_whole=None):
    """GenericKernel::Eval on torch CUDA tensors, enqueued on `stream` (default: torch's current stream).
    nt_whole: the targets are a spatially compact slab of a set of that many (sctl_amd_eval_device_slab)."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if v_trg is None or v_trg.numel() != Nt * info["k1"]:
        v_trg = torch.zeros(Nt * info["k1"], dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_device_slab(info["id"], real, Nt, Ns, Nt if nt_whole is None else nt_whole, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"),
                                               _t_ptr(r_src, tdt, Ns * 3, "r_src"), _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"),
                                               _t_ptr(v_src, tdt, Ns * info["k0"], "v_src"), _t_ptr(v_trg, tdt, Nt * info["k1"], "v_trg"), digits, cp, cb,
                                               C.c_void_p(st.cuda_stream)), "eval_device")
    return v_trg


def eval_transpose_host(name, r_trg, r_src, n_src, w_trg, g_src=None, digits=-1, ctx=None, device=0, accumulate=True):
    """The transposed sum g_src += A^T w_trg on host (numpy) arrays (sctl_amd_eval_transpose_host): w_trg holds Nt*TrgDim target weights, the
    result Ns*SrcDim values.  A g_src of the right size is accumulated into (overwritten with accumulate=False); any other size (or None)
    gives a fresh zeroed result, as Eval does."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    if g_src is None or g_src.size != Ns * info["k0"]:
        g_src = np.zeros(Ns * info["k0"], dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_eval_transpose_host(info["id"], real, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                              _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(w_trg, dt, Nt * info["k1"], "w_trg"),
                                              _np_ptr(g_src, dt, Ns * info["k0"], "g_src"), 1 if accumulate else 0, digits, cp, cb, device), "eval_transpose_host")
    return g_src


def eval_transpose_device(name, r_trg, r_src, n_src, w_trg, g_src=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_transpose_device), enqueued on `stream` (default: torch's current stream); g_src of the
    right size is accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if g_src is None or g_src.numel() != Ns * info["k0"]:
        g_src = torch.zeros(Ns * info["k0"], dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_transpose_device(info["id"], real, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                                    _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(w_trg, tdt, Nt * info["k1"], "w_trg"),
                                                    _t_ptr(g_src, tdt, Ns * info["k0"], "g_src"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
               "eval_transpose_device")
    return g_src


def eval_transpose_densities_host(name, r_trg, r_src, n_src, W_trg, G_src=None, digits=-1, ctx=None, device=0, accumulate=True):
    """nd weight vectors through the transposed sum, G_src[m] += A^T W_trg[m], on numpy arrays (sctl_amd_eval_transpose_densities_host): W_trg of
    shape (nd, Nt*TrgDim), returns (nd, Ns*SrcDim).  A G_src of that shape is accumulated into (overwritten with accumulate=False); None (or another
    shape) gives a fresh zeroed result."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    if W_trg.ndim != 2 or W_trg.shape[1] != Nt * info["k1"]:
        raise SctlAmdError("W_trg must have shape (nd, %d)" % (Nt * info["k1"]))
    nd = W_trg.shape[0]
    if G_src is None or G_src.shape != (nd, Ns * info["k0"]):
        G_src = np.zeros((nd, Ns * info["k0"]), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_eval_transpose_densities_host(info["id"], real, nd, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                                        _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(W_trg, dt, nd * Nt * info["k1"], "W_trg"),
                                                        _np_ptr(G_src, dt, nd * Ns * info["k0"], "G_src"), 1 if accumulate else 0, digits, cp, cb, device),
           "eval_transpose_densities_host")
    return G_src


def eval_transpose_densities_device(name, r_trg, r_src, n_src, W_trg, G_src=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_transpose_densities_device), enqueued on `stream` (default: torch's current stream);
    W_trg of shape (nd, Nt*TrgDim), G_src (nd, Ns*SrcDim) accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if W_trg.dim() != 2 or W_trg.shape[1] != Nt * info["k1"]:
        raise SctlAmdError("W_trg must have shape (nd, %d)" % (Nt * info["k1"]))
    nd = W_trg.shape[0]
    if G_src is None or tuple(G_src.shape) != (nd, Ns * info["k0"]):
        G_src = torch.zeros((nd, Ns * info["k0"]), dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_transpose_densities_device(info["id"], real, nd, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                                              _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(W_trg, tdt, nd * Nt * info["k1"], "W_trg"),
                                                              _t_ptr(G_src, tdt, nd * Ns * info["k0"], "G_src"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
               "eval_transpose_densities_device")
    return G_src


def _grad_wanted(info, want):
    if want is None:
        want = ("trg", "src", "nrm") if info["nd"] else ("trg", "src")
    bad = [x for x in want if x not in ("trg", "src", "nrm")]
    if bad:
        raise SctlAmdError("want holds 'trg', 'src' and 'nrm' only, not %r" % (bad,))
    return tuple(x in want for x in ("trg", "src", "nrm"))


def eval_grad_host(name, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1, ctx=None, device=0, accumulate=True):
    """Gradients of L = <w_trg, A v_src> with respect to the target coordinates, the source coordinates and the source normals on host (numpy)
    arrays (sctl_amd_eval_grad_host).  `want` names the outputs to compute, of "trg", "src", "nrm" (default: all the kernel has); returns
    (g_trg, g_src, g_nrm), each Nt*3 or Ns*3 values, None where not wanted.  An output array of the right size is accumulated into (overwritten
    with accumulate=False); any other size (or None) gives a fresh zeroed result, as Eval does."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    out = []
    for wanted, g, n in zip(_grad_wanted(info, want), (g_trg, g_src, g_nrm), (Nt * 3, Ns * 3, Ns * 3)):
        out.append(None if not wanted else g if g is not None and g.size == n else np.zeros(n, dtype=dt))
    keep, cp, cb = _ctx_blob(info, ctx)
    ptr = [None if g is None else _np_ptr(g, dt, g.size, what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
    _check(lib().sctl_amd_eval_grad_host(info["id"], real, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                         _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(v_src, dt, Ns * info["k0"], "v_src"),
                                         _np_ptr(w_trg, dt, Nt * info["k1"], "w_trg"), ptr[0], ptr[1], ptr[2], 1 if accumulate else 0, digits, cp, cb, device),
           "eval_grad_host")
    return tuple(out)


def eval_grad_device(name, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_grad_device), enqueued on `stream` (default: torch's current stream); outputs of the right
    size are accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    out = []
    for wanted, g, n in zip(_grad_wanted(info, want), (g_trg, g_src, g_nrm), (Nt * 3, Ns * 3, Ns * 3)):
        out.append(None if not wanted else g if g is not None and g.numel() == n else torch.zeros(n, dtype=tdt, device=r_trg.device))
    keep, cp, cb = _ctx_blob(info, ctx)
    ptr = [None if g is None else _t_ptr(g, tdt, g.numel(), what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_grad_device(info["id"], real, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                               _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(v_src, tdt, Ns * info["k0"], "v_src"),
                                               _t_ptr(w_trg, tdt, Nt * info["k1"], "w_trg"), ptr[0], ptr[1], ptr[2], digits, cp, cb,
                                               C.c_void_p(st.cuda_stream)), "eval_grad_device")
    return tuple(out)


def eval_jvp_host(name, r_trg, r_src, n_src, v_src, d_trg=None, d_src=None, d_nrm=None, dv_trg=None, digits=-1, ctx=None, device=0, accumulate=True):
    """The tangent of v_trg = A v_src along a perturbation of the geometry on host (numpy) arrays (sctl_amd_eval_jvp_host): d_trg (Nt*3), d_src (Ns*3)
    and d_nrm (Ns*NormalDim) perturb the target coordinates, the source coordinates and the source normals; None is a field of zeros, and with all
    three None nothing is computed.  Returns dv_trg, Nt*TrgDim values: an array of the right size is accumulated into (overwritten with
    accumulate=False); any other size (or None) gives a fresh zeroed result, as Eval does.  The densities are held fixed: their tangent is
    eval_host(name, r_trg, r_src, n_src, dv_src, dv_trg)."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    if dv_trg is None or dv_trg.size != Nt * info["k1"]:
        dv_trg = np.zeros(Nt * info["k1"], dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    # a normal tangent for a kernel without a normal goes down as it is: the library refuses it
    tan = [None if a is None else _np_ptr(a, dt, n if n else a.size, what)
           for a, n, what in ((d_trg, Nt * 3, "d_trg"), (d_src, Ns * 3, "d_src"), (d_nrm, Ns * info["nd"], "d_nrm"))]
    _check(lib().sctl_amd_eval_jvp_host(info["id"], real, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                        _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(v_src, dt, Ns * info["k0"], "v_src"), tan[0], tan[1], tan[2],
                                        _np_ptr(dv_trg, dt, Nt * info["k1"], "dv_trg"), 1 if accumulate else 0, digits, cp, cb, device), "eval_jvp_host")
    return dv_trg


def eval_jvp_device(name, r_trg, r_src, n_src, v_src, d_trg=None, d_src=None, d_nrm=None, dv_trg=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_jvp_device), enqueued on `stream` (default: torch's current stream); dv_trg of the right size is
    accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if dv_trg is None or dv_trg.numel() != Nt * info["k1"]:
        dv_trg = torch.zeros(Nt * info["k1"], dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    tan = [None if a is None else _t_ptr(a, tdt, n if n else a.numel(), what)
           for a, n, what in ((d_trg, Nt * 3, "d_trg"), (d_src, Ns * 3, "d_src"), (d_nrm, Ns * info["nd"], "d_nrm"))]
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_jvp_device(info["id"], real, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                              _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(v_src, tdt, Ns * info["k0"], "v_src"), tan[0], tan[1], tan[2],
                                              _t_ptr(dv_trg, tdt, Nt * info["k1"], "dv_trg"), digits, cp, cb, C.c_void_p(st.cuda_stream)), "eval_jvp_device")
    return dv_trg


def _grad_rows(info, V_src, W_trg, Nt, Ns, dim):
    """the number of rows of V_src (nd, Ns*SrcDim) and W_trg (nd, Nt*TrgDim)"""
    if dim(V_src) != 2 or V_src.shape[1] != Ns * info["k0"]:
        raise SctlAmdError("V_src must have shape (nd, %d)" % (Ns * info["k0"]))
    if dim(W_trg) != 2 or W_trg.shape[1] != Nt * info["k1"]:
        raise SctlAmdError("W_trg must have shape (nd, %d)" % (Nt * info["k1"]))
    if V_src.shape[0] != W_trg.shape[0]:
        raise SctlAmdError("V_src and W_trg must have the same number of rows, not %d and %d" % (V_src.shape[0], W_trg.shape[0]))
    return V_src.shape[0]


def eval_grad_densities_host(name, r_trg, r_src, n_src, V_src, W_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1, ctx=None, device=0,
                             accumulate=True):
    """Gradients of L = sum_m <W_trg[m], A V_src[m]> with respect to the target coordinates, the source coordinates and the source normals on host
    (numpy) arrays (sctl_amd_eval_grad_densities_host): V_src of shape (nd, Ns*SrcDim), W_trg (nd, Nt*TrgDim); the outputs are the sums over the rows
    of what eval_grad_host gives, one of each whatever nd is.  `want`, the outputs and `accumulate` are as there."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    if r_trg.size != Nt * 3 or r_src.size != Ns * 3:
        raise SctlAmdError("coordinate arrays must hold 3 values per point")
    nd = _grad_rows(info, V_src, W_trg, Nt, Ns, lambda a: a.ndim)
    out = []
    for wanted, g, n in zip(_grad_wanted(info, want), (g_trg, g_src, g_nrm), (Nt * 3, Ns * 3, Ns * 3)):
        out.append(None if not wanted else g if g is not None and g.size == n else np.zeros(n, dtype=dt))
    keep, cp, cb = _ctx_blob(info, ctx)
    ptr = [None if g is None else _np_ptr(g, dt, g.size, what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
    _check(lib().sctl_amd_eval_grad_densities_host(info["id"], real, nd, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                                   _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(V_src, dt, nd * Ns * info["k0"], "V_src"),
                                                   _np_ptr(W_trg, dt, nd * Nt * info["k1"], "W_trg"), ptr[0], ptr[1], ptr[2], 1 if accumulate else 0, digits,
                                                   cp, cb, device), "eval_grad_densities_host")
    return tuple(out)


def eval_grad_densities_device(name, r_trg, r_src, n_src, V_src, W_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1, ctx=None, stream=None):
    """The same on torch CUDA tensors (sctl_amd_eval_grad_densities_device), enqueued on `stream` (default: torch's current stream); outputs of the
    right size are accumulated into."""
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else _real_of(np.float32 if tdt == torch.float32 else np.int8)
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    nd = _grad_rows(info, V_src, W_trg, Nt, Ns, lambda a: a.dim())
    out = []
    for wanted, g, n in zip(_grad_wanted(info, want), (g_trg, g_src, g_nrm), (Nt * 3, Ns * 3, Ns * 3)):
        out.append(None if not wanted else g if g is not None and g.numel() == n else torch.zeros(n, dtype=tdt, device=r_trg.device))
    keep, cp, cb = _ctx_blob(info, ctx)
    ptr = [None if g is None else _t_ptr(g, tdt, g.numel(), what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_eval_grad_densities_device(info["id"], real, nd, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"), _t_ptr(r_src, tdt, Ns * 3, "r_src"),
                                                         _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"), _t_ptr(V_src, tdt, nd * Ns * info["k0"], "V_src"),
                                                         _t_ptr(W_trg, tdt, nd * Nt * info["k1"], "W_trg"), ptr[0], ptr[1], ptr[2], digits, cp, cb,
                                                         C.c_void_p(st.cuda_stream)), "eval_grad_densities_device")
    return tuple(out)


def kernel_matrix_host(name, r_trg, r_src, n_src, digits=-1, ctx=None, device=0):
    """GenericKernel::KernelMatrix on numpy arrays: returns M of shape (Ns*SrcDim, Nt*TrgDim), scale included."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    M = np.zeros((Ns * info["k0"], Nt * info["k1"]), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_kernel_matrix_host(info["id"], real, Nt, Ns, _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                             _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(M, dt, M.size, "M"), digits, cp, cb, device),
           "kernel_matrix_host")
    return M


def kernel_matrix_batch_host(name, Nt, Ns, r_trg, r_src, n_src, digits=-1, ctx=None, device=0):
    """Many KernelMatrix blocks in one launch (sctl_amd_kernel_matrix_batch_host): returns the list of (Ns[b]*K0, Nt[b]*K1) blocks."""
    info = kernel_info(name)
    dt = r_trg.dtype
    real = _real_of(dt)
    Nt, Ns = np.ascontiguousarray(Nt, dtype=np.int64), np.ascontiguousarray(Ns, dtype=np.int64)
    sizes = Ns * info["k0"] * Nt * info["k1"]
    M = np.zeros(int(sizes.sum()), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_kernel_matrix_batch_host(info["id"], real, Nt.size, Nt.ctypes.data_as(C.c_void_p), Ns.ctypes.data_as(C.c_void_p),
                                                   _np_ptr(r_trg, dt, int(Nt.sum()) * 3, "r_trg"), _np_ptr(r_src, dt, int(Ns.sum()) * 3, "r_src"),
                                                   _np_ptr(n_src, dt, int(Ns.sum()) * info["nd"], "n_src"), _np_ptr(M, dt, M.size, "M"), digits, cp, cb, device),
           "kernel_matrix_batch_host")
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [M[off[b]:off[b + 1]].reshape(int(Ns[b]) * info["k0"], int(Nt[b]) * info["k1"]) for b in range(Nt.size)]


def kernel_matrix_device(name, r_trg, r_src, n_src, M=None, digits=-1, ctx=None, stream=None):
    import torch
    info = kernel_info(name)
    tdt = r_trg.dtype
    real = F64 if tdt == torch.float64 else F32
    Nt, Ns = r_trg.numel() // 3, r_src.numel() // 3
    if M is None or M.numel() != Ns * info["k0"] * Nt * info["k1"]:
        M = torch.empty((Ns * info["k0"], Nt * info["k1"]), dtype=tdt, device=r_trg.device)
    keep, cp, cb = _ctx_blob(info, ctx)
    with torch.cuda.device(r_trg.device):
        st = stream if stream is not None else torch.cuda.current_stream()
        _check(lib().sctl_amd_kernel_matrix_device(info["id"], real, Nt, Ns, _t_ptr(r_trg, tdt, Nt * 3, "r_trg"),
                                                   _t_ptr(r_src, tdt, Ns * 3, "r_src"), _t_ptr(n_src, tdt, Ns * info["nd"], "n_src"),
                                                   _t_ptr(M, tdt, M.numel(), "M"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
               "kernel_matrix_device")
    return M


class GenericKernel:
    """Python mirror of a reference kernel object (GenericKernel<uKernel>, generic-kernel.hpp:31-152)."""

    def __init__(self, name, ctx=None):
        self._info = kernel_info(name)
        self._ctx = ctx

    def Name(self):
        return self._info["name"]

    def FLOPS(self):
        return self._info["flops"]

    def uKerScaleFactor(self):
        return self._info["scale"]

    def CoordDim(self):
        return 3

    def NormalDim(self):
        return self._info["nd"]

    def SrcDim(self):
        return self._info["k0"]

    def TrgDim(self):
        return self._info["k1"]

    def SetCtxPtr(self, ctx):
        self._ctx = ctx

    def GetCtxPtr(self):
        return self._ctx

    def Eval(self, v_trg, r_trg, r_src, n_src, v_src, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_host(self._info["id"], r_trg, r_src, n_src, v_src, v_trg, digits, self._ctx, **kw)
        return eval_device(self._info["id"], r_trg, r_src, n_src, v_src, v_trg, digits, self._ctx, **kw)

    def EvalTranspose(self, g_src, r_trg, r_src, n_src, w_trg, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_transpose_host(self._info["id"], r_trg, r_src, n_src, w_trg, g_src, digits, self._ctx, **kw)
        return eval_transpose_device(self._info["id"], r_trg, r_src, n_src, w_trg, g_src, digits, self._ctx, **kw)

    def EvalTransposeDensities(self, G_src, r_trg, r_src, n_src, W_trg, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_transpose_densities_host(self._info["id"], r_trg, r_src, n_src, W_trg, G_src, digits, self._ctx, **kw)
        return eval_transpose_densities_device(self._info["id"], r_trg, r_src, n_src, W_trg, G_src, digits, self._ctx, **kw)

    def EvalGrad(self, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_grad_host(self._info["id"], r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits=digits, ctx=self._ctx, **kw)
        return eval_grad_device(self._info["id"], r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits=digits, ctx=self._ctx, **kw)

    def EvalJvp(self, r_trg, r_src, n_src, v_src, d_trg=None, d_src=None, d_nrm=None, dv_trg=None, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_jvp_host(self._info["id"], r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, dv_trg, digits=digits, ctx=self._ctx, **kw)
        return eval_jvp_device(self._info["id"], r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, dv_trg, digits=digits, ctx=self._ctx, **kw)

    def EvalListsGrad(self, r_trg, r_src, n_src, v_src, w_trg, trg_off, trg_cnt, src_off, src_cnt, g_trg=None, g_src=None, g_nrm=None, digits=-1, **kw):
        """EvalGrad over P2P lists (sctl_amd_eval_lists_grad_host): returns (g_trg, g_src, g_nrm)."""
        return eval_lists_grad_host(self._info["id"], trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits=digits,
                                    ctx=self._ctx, **kw)

    def EvalGradDensities(self, r_trg, r_src, n_src, V_src, W_trg, g_trg=None, g_src=None, g_nrm=None, digits=-1, **kw):
        if isinstance(r_trg, np.ndarray):
            return eval_grad_densities_host(self._info["id"], r_trg, r_src, n_src, V_src, W_trg, g_trg, g_src, g_nrm, digits=digits, ctx=self._ctx, **kw)
        return eval_grad_densities_device(self._info["id"], r_trg, r_src, n_src, V_src, W_trg, g_trg, g_src, g_nrm, digits=digits, ctx=self._ctx, **kw)

    def KernelMatrix(self, M, Xt, Xs, Xn, digits=-1, **kw):
        if isinstance(Xt, np.ndarray):
            return kernel_matrix_host(self._info["id"], Xt, Xs, Xn, digits, self._ctx, **kw)
        return kernel_matrix_device(self._info["id"], Xt, Xs, Xn, M, digits, self._ctx, **kw)


class DirectOp:
    """Device-resident operator (sctl_amd_op_*): coordinates are uploaded once, each eval() moves only density and
    potential.  The Python face of what ParticleFMM keeps between SetSrcCoord/SetTrgCoord and repeated Eval calls."""

    def __init__(self, name, dtype=np.float64, devices=(0,), ctx=None):
        self.info = kernel_info(name)
        self.dtype = np.dtype(dtype)
        self.real = _real_of(dtype)
        self.ctx = ctx
        self.Nt = self.Ns = 0
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().sctl_amd_op_create(self.info["id"], self.real, devs, len(devices), C.byref(self._h)), "op_create")

    def set_targets(self, r_trg):
        self.Nt = r_trg.size // 3
        self._dot = False
        _check(lib().sctl_amd_op_set_targets(self._h, self.Nt, _np_ptr(r_trg, self.dtype, self.Nt * 3, "r_trg")), "op_set_targets")

    def set_sources(self, r_src, n_src=None):
        self.Ns = r_src.size // 3
        _check(lib().sctl_amd_op_set_sources(self._h, self.Ns, _np_ptr(r_src, self.dtype, self.Ns * 3, "r_src"),
                                             _np_ptr(n_src, self.dtype, self.Ns * self.info["nd"], "n_src")), "op_set_sources")

    def set_source_weights(self, weights):
        """Quadrature weights applied to every density on the device (None clears); after set_sources."""
        self._weights = weights is not None
        _check(lib().sctl_amd_op_set_source_weights(self._h, None if weights is None else _np_ptr(weights, self.dtype, self.Ns, "weights")), "op_set_source_weights")

    def set_target_normals(self, n_trg):
        """The kernel's output is contracted with these normals on the device, TrgDim -> TrgDim/3 (None clears); after set_targets."""
        _check(lib().sctl_amd_op_set_target_normals(self._h, None if n_trg is None else _np_ptr(n_trg, self.dtype, self.Nt * 3, "n_trg")), "op_set_target_normals")
        self._dot = n_trg is not None

    def eval(self, v_src, v_trg=None, accumulate=False, digits=-1):
        k1 = self.info["k1"] // 3 if getattr(self, "_dot", False) else self.info["k1"]
        if v_trg is None or v_trg.size != self.Nt * k1:
            v_trg = np.zeros(self.Nt * k1, dtype=self.dtype)
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval(self._h, _np_ptr(v_src, self.dtype, self.Ns * self.info["k0"], "v_src"),
                                      _np_ptr(v_trg, self.dtype, self.Nt * k1, "v_trg"), 1 if accumulate else 0, digits, cp, cb), "op_eval")
        return v_trg

    def eval_densities(self, V_src, V_trg=None, accumulate=False, digits=-1):
        """eval() for nd densities in one pass (sctl_amd_op_eval_densities): V_src of shape (nd, Ns*SrcDim), returns (nd, Nt*k1) with
        k1 = TrgDim, or TrgDim/3 with target normals."""
        k1 = self.info["k1"] // 3 if getattr(self, "_dot", False) else self.info["k1"]
        if V_src.ndim != 2 or V_src.shape[1] != self.Ns * self.info["k0"]:
            raise SctlAmdError("V_src must have shape (nd, %d)" % (self.Ns * self.info["k0"]))
        nd = V_src.shape[0]
        if V_trg is None or V_trg.shape != (nd, self.Nt * k1):
            V_trg = np.zeros((nd, self.Nt * k1), dtype=self.dtype)
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_densities(self._h, nd, _np_ptr(V_src, self.dtype, nd * self.Ns * self.info["k0"], "V_src"),
                                                _np_ptr(V_trg, self.dtype, nd * self.Nt * k1, "V_trg"), 1 if accumulate else 0, digits, cp, cb), "op_eval_densities")
        return V_trg

    def set_near(self, trg_dim, elem_nds_cnt, near_elem_cnt, K_near, near_scatter_index, near_trg_cnt, near_trg_dsp, K_near_cnt=None):
        """Attach the near-field operator of the same BoundaryIntegralOp (the arrays of NearOp) for the current targets."""
        i8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        nds, near, kcnt, sc, tc, td = i8(elem_nds_cnt), i8(near_elem_cnt), i8(K_near_cnt), i8(near_scatter_index), i8(near_trg_cnt), i8(near_trg_dsp)
        K = np.ascontiguousarray(K_near, dtype=self.dtype)
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_op_set_near(self._h, self.info["k0"], trg_dim, nds.size, p(nds), p(near), p(kcnt), p(K), p(sc), p(tc), p(td)), "op_set_near")
        self._near_len, self._near_k1 = int(nds.sum()) * self.info["k0"], trg_dim

    def eval_potential(self, v_src_far, f_near, v_trg=None, accumulate=False, digits=-1):
        """Far field + attached near field in one pass over the devices (sctl_amd_op_eval_potential): ComputePotential."""
        k1 = self._near_k1
        if v_trg is None or v_trg.size != self.Nt * k1:
            v_trg = np.zeros(self.Nt * k1, dtype=self.dtype)
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_potential(self._h, _np_ptr(v_src_far, self.dtype, self.Ns * self.info["k0"], "v_src_far"),
                                                _np_ptr(f_near, self.dtype, self._near_len, "f_near"), _np_ptr(v_trg, self.dtype, self.Nt * k1, "v_trg"),
                                                1 if accumulate else 0, digits, cp, cb), "op_eval_potential")
        return v_trg

    def eval_potential_densities(self, V_src_far, F_near, V_trg=None, accumulate=False, digits=-1):
        """eval_potential() for nd densities in one pass over the devices (sctl_amd_op_eval_potential_densities): V_src_far of shape
        (nd, Ns*SrcDim), F_near of shape (nd, near density length), returns (nd, Nt*trg_dim)."""
        k1 = self._near_k1
        if V_src_far.ndim != 2 or V_src_far.shape[1] != self.Ns * self.info["k0"]:
            raise SctlAmdError("V_src_far must have shape (nd, %d)" % (self.Ns * self.info["k0"]))
        nd = V_src_far.shape[0]
        if F_near.shape != (nd, self._near_len):
            raise SctlAmdError("F_near must have shape (%d, %d)" % (nd, self._near_len))
        if V_trg is None or V_trg.shape != (nd, self.Nt * k1):
            V_trg = np.zeros((nd, self.Nt * k1), dtype=self.dtype)
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_potential_densities(self._h, nd, _np_ptr(V_src_far, self.dtype, nd * self.Ns * self.info["k0"], "V_src_far"),
                                                          _np_ptr(F_near, self.dtype, nd * self._near_len, "F_near"),
                                                          _np_ptr(V_trg, self.dtype, nd * self.Nt * k1, "V_trg"), 1 if accumulate else 0, digits, cp, cb),
               "op_eval_potential_densities")
        return V_trg

    def _out(self, a, n, what):
        if a is None:
            return np.zeros(n, dtype=self.dtype)
        if not isinstance(a, np.ndarray) or a.size != n or a.dtype != self.dtype or not a.flags.c_contiguous:
            raise SctlAmdError("%s must be a contiguous %s array of %d values" % (what, self.dtype, n))
        return a

    def eval_transpose(self, w_trg, g_src=None, accumulate=False, digits=-1):
        """The adjoint of eval() (sctl_amd_op_eval_transpose): g_src = D_w A^T C_n^T w_trg, with the source weights and target normals
        that are set; w_trg holds Nt*TrgDim values (Nt*TrgDim/3 with target normals), g_src Ns*SrcDim."""
        k1 = self.info["k1"] // 3 if getattr(self, "_dot", False) else self.info["k1"]
        if np.size(w_trg) != self.Nt * k1:
            raise SctlAmdError("w_trg must hold %d values" % (self.Nt * k1))
        g_src = self._out(g_src, self.Ns * self.info["k0"], "g_src")
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_transpose(self._h, _np_ptr(w_trg, self.dtype, self.Nt * k1, "w_trg"), _np_ptr(g_src, self.dtype, g_src.size, "g_src"),
                                                1 if accumulate else 0, digits, cp, cb), "op_eval_transpose")
        return g_src

    def eval_potential_transpose(self, w_trg, g_src_far=None, g_near=None, accumulate=False, digits=-1):
        """The adjoint of eval_potential() (sctl_amd_op_eval_potential_transpose): returns (g_src_far, g_near), the gradients with respect
        to the far-field density (Ns*SrcDim values) and the near-field density (element nodes x SrcDim)."""
        if not hasattr(self, "_near_k1"):
            raise SctlAmdError("no near-field operator attached: call set_near first")
        k1 = self._near_k1
        if np.size(w_trg) != self.Nt * k1:
            raise SctlAmdError("w_trg must hold %d values" % (self.Nt * k1))
        g_src_far = self._out(g_src_far, self.Ns * self.info["k0"], "g_src_far")
        g_near = self._out(g_near, self._near_len, "g_near")
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_potential_transpose(self._h, _np_ptr(w_trg, self.dtype, self.Nt * k1, "w_trg"),
                                                          _np_ptr(g_src_far, self.dtype, g_src_far.size, "g_src_far"), _np_ptr(g_near, self.dtype, g_near.size, "g_near"),
                                                          1 if accumulate else 0, digits, cp, cb), "op_eval_potential_transpose")
        return g_src_far, g_near

    def _out2(self, a, nd, n, what):
        if a is None:
            return np.zeros((nd, n), dtype=self.dtype)
        if not isinstance(a, np.ndarray) or a.shape != (nd, n) or a.dtype != self.dtype or not a.flags.c_contiguous:
            raise SctlAmdError("%s must be a contiguous %s array of shape (%d, %d)" % (what, self.dtype, nd, n))
        return a

    def eval_transpose_densities(self, W_trg, G_src=None, accumulate=False, digits=-1):
        """eval_transpose() for nd weight vectors in one pass over the devices (sctl_amd_op_eval_transpose_densities): W_trg of shape
        (nd, Nt*k1) with k1 = TrgDim, or TrgDim/3 with target normals; returns G_src of shape (nd, Ns*SrcDim)."""
        k1 = self.info["k1"] // 3 if getattr(self, "_dot", False) else self.info["k1"]
        if np.ndim(W_trg) != 2 or np.shape(W_trg)[1] != self.Nt * k1:
            raise SctlAmdError("W_trg must have shape (nd, %d)" % (self.Nt * k1))
        nd = np.shape(W_trg)[0]
        G_src = self._out2(G_src, nd, self.Ns * self.info["k0"], "G_src")
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_transpose_densities(self._h, nd, _np_ptr(W_trg, self.dtype, nd * self.Nt * k1, "W_trg"),
                                                          _np_ptr(G_src, self.dtype, G_src.size, "G_src"), 1 if accumulate else 0, digits, cp, cb),
               "op_eval_transpose_densities")
        return G_src

    def eval_potential_transpose_densities(self, W_trg, G_src_far=None, G_near=None, accumulate=False, digits=-1):
        """eval_potential_transpose() for nd weight vectors in one pass over the devices (sctl_amd_op_eval_potential_transpose_densities):
        W_trg of shape (nd, Nt*trg_dim); returns (G_src_far, G_near) of shapes (nd, Ns*SrcDim) and (nd, near density length)."""
        if not hasattr(self, "_near_k1"):
            raise SctlAmdError("no near-field operator attached: call set_near first")
        k1 = self._near_k1
        if np.ndim(W_trg) != 2 or np.shape(W_trg)[1] != self.Nt * k1:
            raise SctlAmdError("W_trg must have shape (nd, %d)" % (self.Nt * k1))
        nd = np.shape(W_trg)[0]
        G_src_far = self._out2(G_src_far, nd, self.Ns * self.info["k0"], "G_src_far")
        G_near = self._out2(G_near, nd, self._near_len, "G_near")
        keep, cp, cb = _ctx_blob(self.info, self.ctx)
        _check(lib().sctl_amd_op_eval_potential_transpose_densities(self._h, nd, _np_ptr(W_trg, self.dtype, nd * self.Nt * k1, "W_trg"),
                                                                    _np_ptr(G_src_far, self.dtype, G_src_far.size, "G_src_far"),
                                                                    _np_ptr(G_near, self.dtype, G_near.size, "G_near"), 1 if accumulate else 0, digits, cp, cb),
               "op_eval_potential_transpose_densities")
        return G_src_far, G_near

    def close(self):
        if self._h:
            lib().sctl_amd_op_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NearOp:
    """BoundaryIntegralOp::ComputeNearInterac with the operator blocks resident on one GPU (sctl_amd_near_*): built from the
    arrays SetupNear leaves behind (boundary_integral.txx:816-1012), applied once per solver iteration."""

    def __init__(self, src_dim, trg_dim, elem_nds_cnt, near_elem_cnt, K_near, near_scatter_index, near_trg_cnt, near_trg_dsp, K_near_cnt=None, device=0):
        i8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        self._keep = [i8(elem_nds_cnt), i8(near_elem_cnt), i8(K_near_cnt), np.ascontiguousarray(K_near), i8(near_scatter_index), i8(near_trg_cnt), i8(near_trg_dsp)]
        nds, near, kcnt, K, sc, tc, td = self._keep
        self.dtype = K.dtype
        self.real = _real_of(K.dtype)
        self.device = device
        h = C.c_void_p()
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_near_create(self.real, device, nds.size, src_dim, trg_dim, p(nds), p(near), p(kcnt), p(K), tc.size, p(sc), p(tc), p(td), C.byref(h)),
               "near_create")
        self._h = h
        v = [C.c_int64() for _ in range(5)]
        _check(lib().sctl_amd_near_info(self._h, *[C.byref(x) for x in v]), "near_info")
        self.density_len, self.potential_len, self.near_entries, self.operator_bytes, self.workgroups = (x.value for x in v)

    def apply(self, F, U=None):
        """U += near field of density F (numpy arrays); U=None starts from zero."""
        F = np.ascontiguousarray(F, dtype=self.dtype)
        if F.size != self.density_len:
            raise SctlAmdError("density must hold %d values" % self.density_len)
        if U is None:
            U = np.zeros(self.potential_len, dtype=self.dtype)
        if U.size != self.potential_len or U.dtype != self.dtype or not U.flags.c_contiguous:
            raise SctlAmdError("potential must be a contiguous %s array of %d values" % (self.dtype, self.potential_len))
        p = lambda a: None if a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_near_apply_host(self._h, p(F), p(U)), "near_apply_host")
        return U

    def apply_device(self, F, U, stream=None):
        """The same on torch CUDA tensors, enqueued on `stream` (default: torch's current stream); U is accumulated into."""
        import torch
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        with torch.cuda.device(F.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_near_apply_device(self._h, _t_ptr(F, tdt, self.density_len, "F"), _t_ptr(U, tdt, self.potential_len, "U"),
                                                    C.c_void_p(st.cuda_stream)), "near_apply_device")
        return U

    def apply_transpose(self, W, G=None):
        """G += N^T W (numpy arrays, sctl_amd_near_apply_transpose_host): W of potential_len values, G of density_len; G=None starts from zero."""
        W = np.ascontiguousarray(W, dtype=self.dtype)
        if W.size != self.potential_len:
            raise SctlAmdError("weights must hold %d values" % self.potential_len)
        if G is None:
            G = np.zeros(self.density_len, dtype=self.dtype)
        if G.size != self.density_len or G.dtype != self.dtype or not G.flags.c_contiguous:
            raise SctlAmdError("density gradient must be a contiguous %s array of %d values" % (self.dtype, self.density_len))
        p = lambda a: None if a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_near_apply_transpose_host(self._h, p(W), p(G)), "near_apply_transpose_host")
        return G

    def apply_transpose_device(self, W, G, stream=None):
        """The same on torch CUDA tensors, enqueued on `stream` (default: torch's current stream); G is accumulated into."""
        import torch
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if W.numel() != self.potential_len or G.numel() != self.density_len:
            raise SctlAmdError("weights and density gradient must hold %d and %d values" % (self.potential_len, self.density_len))
        with torch.cuda.device(W.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_near_apply_transpose_device(self._h, _t_ptr(W, tdt, self.potential_len, "W"), _t_ptr(G, tdt, self.density_len, "G"),
                                                              C.c_void_p(st.cuda_stream)), "near_apply_transpose_device")
        return G

    def apply_densities(self, F, U=None):
        """apply() for nd densities with the operator read once per pass (sctl_amd_near_apply_densities_host): F of shape
        (nd, density_len); every row of U (nd, potential_len) is accumulated into, U=None starts from zero."""
        F = np.ascontiguousarray(F, dtype=self.dtype)
        if F.ndim != 2 or F.shape[1] != self.density_len:
            raise SctlAmdError("densities must have shape (nd, %d)" % self.density_len)
        nd = F.shape[0]
        if U is None:
            U = np.zeros((nd, self.potential_len), dtype=self.dtype)
        if U.shape != (nd, self.potential_len) or U.dtype != self.dtype or not U.flags.c_contiguous:
            raise SctlAmdError("potentials must be a contiguous %s array of shape (%d, %d)" % (self.dtype, nd, self.potential_len))
        p = lambda a: None if a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_near_apply_densities_host(self._h, nd, p(F), p(U)), "near_apply_densities_host")
        return U

    def apply_densities_device(self, F, U, stream=None):
        """The same on torch CUDA tensors of shapes (nd, density_len) and (nd, potential_len), enqueued on `stream` (default: torch's
        current stream); every row of U is accumulated into."""
        import torch
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if F.dim() != 2 or U.dim() != 2 or U.shape[0] != F.shape[0]:
            raise SctlAmdError("densities and potentials must have shapes (nd, %d) and (nd, %d)" % (self.density_len, self.potential_len))
        nd = F.shape[0]
        with torch.cuda.device(F.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_near_apply_densities_device(self._h, nd, _t_ptr(F, tdt, nd * self.density_len, "F"), _t_ptr(U, tdt, nd * self.potential_len, "U"),
                                                              C.c_void_p(st.cuda_stream)), "near_apply_densities_device")
        return U

    def apply_transpose_densities(self, W, G=None):
        """apply_transpose() for nd weight vectors with the operator read once per pass (sctl_amd_near_apply_transpose_densities_host): W of
        shape (nd, potential_len); every row of G (nd, density_len) is accumulated into, G=None starts from zero."""
        W = np.ascontiguousarray(W, dtype=self.dtype)
        if W.ndim != 2 or W.shape[1] != self.potential_len:
            raise SctlAmdError("weights must have shape (nd, %d)" % self.potential_len)
        nd = W.shape[0]
        if G is None:
            G = np.zeros((nd, self.density_len), dtype=self.dtype)
        if not isinstance(G, np.ndarray) or G.shape != (nd, self.density_len) or G.dtype != self.dtype or not G.flags.c_contiguous:
            raise SctlAmdError("density gradients must be a contiguous %s array of shape (%d, %d)" % (self.dtype, nd, self.density_len))
        p = lambda a: None if a.size == 0 else a.ctypes.data_as(C.c_void_p)
        _check(lib().sctl_amd_near_apply_transpose_densities_host(self._h, nd, p(W), p(G)), "near_apply_transpose_densities_host")
        return G

    def apply_transpose_densities_device(self, W, G, stream=None):
        """The same on torch CUDA tensors of shapes (nd, potential_len) and (nd, density_len), enqueued on `stream` (default: torch's
        current stream); every row of G is accumulated into."""
        import torch
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if W.dim() != 2 or G.dim() != 2 or G.shape[0] != W.shape[0] or W.shape[1] != self.potential_len or G.shape[1] != self.density_len:
            raise SctlAmdError("weights and density gradients must have shapes (nd, %d) and (nd, %d)" % (self.potential_len, self.density_len))
        if W.dtype != tdt or G.dtype != tdt:
            raise SctlAmdError("weights and density gradients must be %s tensors" % tdt)
        nd = W.shape[0]
        with torch.cuda.device(W.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_near_apply_transpose_densities_device(self._h, nd, _t_ptr(W, tdt, nd * self.potential_len, "W"),
                                                                        _t_ptr(G, tdt, nd * self.density_len, "G"), C.c_void_p(st.cuda_stream)),
                   "near_apply_transpose_densities_device")
        return G

    def close(self):
        if getattr(self, "_h", None):
            lib().sctl_amd_near_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LISTS_FORWARD, LISTS_TRANSPOSE = 1, 2
_LISTS_DIRECTIONS = {"forward": LISTS_FORWARD, "transpose": LISTS_TRANSPOSE, "both": LISTS_FORWARD | LISTS_TRANSPOSE}


class ListsPlan:
    """Many (target range x source range) direct sums in one launch (sctl_amd_lists_*): the P2P / U-list shape of a tree code
    (fmm-wrapper.txx:756-786).  Offsets and counts are in points.  directions: "forward" (eval_*: target ranges must be identical or
    disjoint), "transpose" (eval_transpose_*: the same of the source ranges) or "both"."""

    def __init__(self, name, dtype, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, device=0, ctx=None, directions="forward"):
        self.info = kernel_info(name)
        self.dtype = np.dtype(dtype)
        self.real = _real_of(dtype)
        self.ctx, self.Nt, self.Ns, self.device = ctx, int(Nt), int(Ns), device
        if directions not in _LISTS_DIRECTIONS:
            raise SctlAmdError('directions must be "forward", "transpose" or "both"')
        self.directions = _LISTS_DIRECTIONS[directions]
        arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (trg_off, trg_cnt, src_off, src_cnt)]
        if len({a.size for a in arrs}) != 1:
            raise SctlAmdError("the four list arrays must have one entry per list")
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        self._h = C.c_void_p()
        if self.directions == LISTS_FORWARD:
            _check(lib().sctl_amd_lists_create(self.info["id"], self.real, device, arrs[0].size, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), self.Nt, self.Ns,
                                               C.byref(self._h)), "lists_create")
        else:
            _check(lib().sctl_amd_lists_create_directions(self.info["id"], self.real, device, arrs[0].size, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), self.Nt,
                                                          self.Ns, self.directions, C.byref(self._h)), "lists_create_directions")
        v = [C.c_int64() for _ in range(3)]
        _check(lib().sctl_amd_lists_info(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])), "lists_info")
        self.pairs, self.work_items, self.source_ranges = v[0].value, v[1].value, v[2].value

    def transpose_info(self):
        """pairs, work items and target ranges of the transposed side (sctl_amd_lists_transpose_info); all 0 for a forward-only plan."""
        v = [C.c_int64() for _ in range(3)]
        _check(lib().sctl_amd_lists_transpose_info(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2])), "lists_transpose_info")
        return dict(pairs=v[0].value, work_items=v[1].value, target_ranges=v[2].value)

    def eval_transpose_host(self, r_trg, r_src, n_src, w_trg, g_src=None, digits=-1):
        """g_src += A^T w_trg over the lists on numpy arrays (sctl_amd_lists_eval_transpose_host): w_trg holds Nt*TrgDim target weights; a g_src
        of Ns*SrcDim values is accumulated into, otherwise a fresh zeroed result is returned."""
        dt, i = self.dtype, self.info
        if np.size(w_trg) != self.Nt * i["k1"]:
            raise SctlAmdError("w_trg must be Nt*TrgDim = %d values" % (self.Nt * i["k1"]))
        if g_src is None:
            g_src = np.zeros(self.Ns * i["k0"], dtype=dt)
        elif g_src.size != self.Ns * i["k0"]:
            raise SctlAmdError("g_src must be Ns*SrcDim = %d values" % (self.Ns * i["k0"]))
        keep, cp, cb = _ctx_blob(i, self.ctx)
        _check(lib().sctl_amd_lists_eval_transpose_host(self._h, _np_ptr(r_trg, dt, self.Nt * 3, "r_trg"), _np_ptr(r_src, dt, self.Ns * 3, "r_src"),
                                                        _np_ptr(n_src, dt, self.Ns * i["nd"], "n_src"), _np_ptr(w_trg, dt, self.Nt * i["k1"], "w_trg"),
                                                        _np_ptr(g_src, dt, self.Ns * i["k0"], "g_src"), digits, cp, cb), "lists_eval_transpose_host")
        return g_src

    def eval_transpose_device(self, r_trg, r_src, n_src, w_trg, g_src=None, digits=-1, stream=None):
        """The same on torch CUDA tensors on the plan's device (sctl_amd_lists_eval_transpose_device), enqueued on `stream` (default: torch's
        current stream); g_src is accumulated into."""
        import torch
        i = self.info
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if w_trg.numel() != self.Nt * i["k1"]:
            raise SctlAmdError("w_trg must be Nt*TrgDim = %d values" % (self.Nt * i["k1"]))
        if g_src is None:
            g_src = torch.zeros(self.Ns * i["k0"], dtype=tdt, device=r_trg.device)
        elif g_src.numel() != self.Ns * i["k0"]:
            raise SctlAmdError("g_src must be Ns*SrcDim = %d values" % (self.Ns * i["k0"]))
        keep, cp, cb = _ctx_blob(i, self.ctx)
        with torch.cuda.device(r_trg.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_lists_eval_transpose_device(self._h, _t_ptr(r_trg, tdt, self.Nt * 3, "r_trg"), _t_ptr(r_src, tdt, self.Ns * 3, "r_src"),
                                                              _t_ptr(n_src, tdt, self.Ns * i["nd"], "n_src"), _t_ptr(w_trg, tdt, self.Nt * i["k1"], "w_trg"),
                                                              _t_ptr(g_src, tdt, self.Ns * i["k0"], "g_src"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
                   "lists_eval_transpose_device")
        return g_src

    def eval_grad_host(self, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1):
        """Gradients of L = sum over the lists of <w_trg, A_l v_src> with respect to the target coordinates, the source coordinates and the source
        normals on numpy arrays (sctl_amd_lists_eval_grad_host).  `want` names the outputs to compute, of "trg", "src", "nrm" (default: all the
        kernel has), as sctl_amd.eval_grad_host does; "trg" needs a plan with the forward direction, "src" and "nrm" one with the transposed.
        Returns (g_trg, g_src, g_nrm), each Nt*3 or Ns*3 values, None where not wanted; an output of the right size is accumulated into, any
        other size (or None) gives a fresh zeroed result."""
        dt, i = self.dtype, self.info
        out = []
        for wanted, g, n in zip(_grad_wanted(i, want), (g_trg, g_src, g_nrm), (self.Nt * 3, self.Ns * 3, self.Ns * 3)):
            out.append(None if not wanted else g if g is not None and g.size == n else np.zeros(n, dtype=dt))
        keep, cp, cb = _ctx_blob(i, self.ctx)
        ptr = [None if g is None else _np_ptr(g, dt, g.size, what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
        _check(lib().sctl_amd_lists_eval_grad_host(self._h, _np_ptr(r_trg, dt, self.Nt * 3, "r_trg"), _np_ptr(r_src, dt, self.Ns * 3, "r_src"),
                                                   _np_ptr(n_src, dt, self.Ns * i["nd"], "n_src"), _np_ptr(v_src, dt, self.Ns * i["k0"], "v_src"),
                                                   _np_ptr(w_trg, dt, self.Nt * i["k1"], "w_trg"), ptr[0], ptr[1], ptr[2], digits, cp, cb), "lists_eval_grad_host")
        return tuple(out)

    def eval_grad_device(self, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1, stream=None):
        """The same on torch CUDA tensors on the plan's device (sctl_amd_lists_eval_grad_device), enqueued on `stream` (default: torch's current
        stream): one launch for g_trg, one for g_src and g_nrm; outputs of the right size are accumulated into."""
        import torch
        i = self.info
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        out = []
        for wanted, g, n in zip(_grad_wanted(i, want), (g_trg, g_src, g_nrm), (self.Nt * 3, self.Ns * 3, self.Ns * 3)):
            out.append(None if not wanted else g if g is not None and g.numel() == n else torch.zeros(n, dtype=tdt, device=r_trg.device))
        keep, cp, cb = _ctx_blob(i, self.ctx)
        ptr = [None if g is None else _t_ptr(g, tdt, g.numel(), what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
        with torch.cuda.device(r_trg.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_lists_eval_grad_device(self._h, _t_ptr(r_trg, tdt, self.Nt * 3, "r_trg"), _t_ptr(r_src, tdt, self.Ns * 3, "r_src"),
                                                         _t_ptr(n_src, tdt, self.Ns * i["nd"], "n_src"), _t_ptr(v_src, tdt, self.Ns * i["k0"], "v_src"),
                                                         _t_ptr(w_trg, tdt, self.Nt * i["k1"], "w_trg"), ptr[0], ptr[1], ptr[2], digits, cp, cb,
                                                         C.c_void_p(st.cuda_stream)), "lists_eval_grad_device")
        return tuple(out)

    def eval_host(self, r_trg, r_src, n_src, v_src, v_trg=None, digits=-1):
        """numpy arrays; v_trg of the right size is accumulated into, otherwise a fresh zeroed result is returned."""
        dt, i = self.dtype, self.info
        if v_trg is None or v_trg.size != self.Nt * i["k1"]:
            v_trg = np.zeros(self.Nt * i["k1"], dtype=dt)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        _check(lib().sctl_amd_lists_eval_host(self._h, _np_ptr(r_trg, dt, self.Nt * 3, "r_trg"), _np_ptr(r_src, dt, self.Ns * 3, "r_src"),
                                              _np_ptr(n_src, dt, self.Ns * i["nd"], "n_src"), _np_ptr(v_src, dt, self.Ns * i["k0"], "v_src"),
                                              _np_ptr(v_trg, dt, self.Nt * i["k1"], "v_trg"), digits, cp, cb), "lists_eval_host")
        return v_trg

    def eval_device(self, r_trg, r_src, n_src, v_src, v_trg=None, digits=-1, stream=None):
        """torch CUDA tensors on the plan's device; enqueued on `stream` (default: torch's current stream); v_trg is accumulated into."""
        import torch
        i = self.info
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if v_trg is None or v_trg.numel() != self.Nt * i["k1"]:
            v_trg = torch.zeros(self.Nt * i["k1"], dtype=tdt, device=r_trg.device)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        with torch.cuda.device(r_trg.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_lists_eval_device(self._h, _t_ptr(r_trg, tdt, self.Nt * 3, "r_trg"), _t_ptr(r_src, tdt, self.Ns * 3, "r_src"),
                                                    _t_ptr(n_src, tdt, self.Ns * i["nd"], "n_src"), _t_ptr(v_src, tdt, self.Ns * i["k0"], "v_src"),
                                                    _t_ptr(v_trg, tdt, self.Nt * i["k1"], "v_trg"), digits, cp, cb, C.c_void_p(st.cuda_stream)), "lists_eval_device")
        return v_trg

    def eval_densities_host(self, r_trg, r_src, n_src, F, V_trg=None, digits=-1):
        """eval_host() for nd densities in one launch per pass (sctl_amd_lists_eval_densities_host): F of shape (nd, Ns*SrcDim), returns
        (nd, Nt*k1); a V_trg of that shape is accumulated into, otherwise a fresh zeroed result is returned."""
        dt, i = self.dtype, self.info
        F = np.asarray(F)
        if F.ndim != 2 or F.shape[1] != self.Ns * i["k0"]:
            raise SctlAmdError("densities must have shape (nd, %d)" % (self.Ns * i["k0"]))
        nd = F.shape[0]
        if V_trg is None or V_trg.shape != (nd, self.Nt * i["k1"]):
            V_trg = np.zeros((nd, self.Nt * i["k1"]), dtype=dt)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        _check(lib().sctl_amd_lists_eval_densities_host(self._h, nd, _np_ptr(r_trg, dt, self.Nt * 3, "r_trg"), _np_ptr(r_src, dt, self.Ns * 3, "r_src"),
                                                        _np_ptr(n_src, dt, self.Ns * i["nd"], "n_src"), _np_ptr(F, dt, nd * self.Ns * i["k0"], "F"),
                                                        _np_ptr(V_trg, dt, nd * self.Nt * i["k1"], "V_trg"), digits, cp, cb), "lists_eval_densities_host")
        return V_trg

    def eval_densities_device(self, r_trg, r_src, n_src, F, V_trg=None, digits=-1, stream=None):
        """The same on torch CUDA tensors on the plan's device (sctl_amd_lists_eval_densities_device), enqueued on `stream` (default:
        torch's current stream); V_trg of shape (nd, Nt*k1) is accumulated into."""
        import torch
        i = self.info
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if F.dim() != 2 or F.shape[1] != self.Ns * i["k0"]:
            raise SctlAmdError("densities must have shape (nd, %d)" % (self.Ns * i["k0"]))
        nd = F.shape[0]
        if V_trg is None or tuple(V_trg.shape) != (nd, self.Nt * i["k1"]):
            V_trg = torch.zeros((nd, self.Nt * i["k1"]), dtype=tdt, device=r_trg.device)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        with torch.cuda.device(r_trg.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_lists_eval_densities_device(self._h, nd, _t_ptr(r_trg, tdt, self.Nt * 3, "r_trg"), _t_ptr(r_src, tdt, self.Ns * 3, "r_src"),
                                                              _t_ptr(n_src, tdt, self.Ns * i["nd"], "n_src"), _t_ptr(F, tdt, nd * self.Ns * i["k0"], "F"),
                                                              _t_ptr(V_trg, tdt, nd * self.Nt * i["k1"], "V_trg"), digits, cp, cb, C.c_void_p(st.cuda_stream)),
                   "lists_eval_densities_device")
        return V_trg

    def eval_transpose_densities_host(self, r_trg, r_src, n_src, W_trg, G_src=None, digits=-1):
        """eval_transpose_host() for nd weight vectors in one launch per pass (sctl_amd_lists_eval_transpose_densities_host): W_trg of shape
        (nd, Nt*TrgDim), returns (nd, Ns*SrcDim); a G_src of that shape is accumulated into, otherwise a fresh zeroed result is returned."""
        dt, i = self.dtype, self.info
        W_trg = np.asarray(W_trg)
        if W_trg.ndim != 2 or W_trg.shape[1] != self.Nt * i["k1"]:
            raise SctlAmdError("weights must have shape (nd, %d)" % (self.Nt * i["k1"]))
        nd = W_trg.shape[0]
        if G_src is None or G_src.shape != (nd, self.Ns * i["k0"]):
            G_src = np.zeros((nd, self.Ns * i["k0"]), dtype=dt)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        _check(lib().sctl_amd_lists_eval_transpose_densities_host(self._h, nd, _np_ptr(r_trg, dt, self.Nt * 3, "r_trg"), _np_ptr(r_src, dt, self.Ns * 3, "r_src"),
                                                                  _np_ptr(n_src, dt, self.Ns * i["nd"], "n_src"),
                                                                  _np_ptr(W_trg, dt, nd * self.Nt * i["k1"], "W_trg"),
                                                                  _np_ptr(G_src, dt, nd * self.Ns * i["k0"], "G_src"), digits, cp, cb),
               "lists_eval_transpose_densities_host")
        return G_src

    def eval_transpose_densities_device(self, r_trg, r_src, n_src, W_trg, G_src=None, digits=-1, stream=None):
        """The same on torch CUDA tensors on the plan's device (sctl_amd_lists_eval_transpose_densities_device), enqueued on `stream` (default:
        torch's current stream); G_src of shape (nd, Ns*SrcDim) is accumulated into."""
        import torch
        i = self.info
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if W_trg.dim() != 2 or W_trg.shape[1] != self.Nt * i["k1"]:
            raise SctlAmdError("weights must have shape (nd, %d)" % (self.Nt * i["k1"]))
        nd = W_trg.shape[0]
        if G_src is None or tuple(G_src.shape) != (nd, self.Ns * i["k0"]):
            G_src = torch.zeros((nd, self.Ns * i["k0"]), dtype=tdt, device=r_trg.device)
        keep, cp, cb = _ctx_blob(i, self.ctx)
        with torch.cuda.device(r_trg.device):
            st = stream if stream is not None else torch.cuda.current_stream()
            _check(lib().sctl_amd_lists_eval_transpose_densities_device(self._h, nd, _t_ptr(r_trg, tdt, self.Nt * 3, "r_trg"), _t_ptr(r_src, tdt, self.Ns * 3, "r_src"),
                                                                        _t_ptr(n_src, tdt, self.Ns * i["nd"], "n_src"),
                                                                        _t_ptr(W_trg, tdt, nd * self.Nt * i["k1"], "W_trg"),
                                                                        _t_ptr(G_src, tdt, nd * self.Ns * i["k0"], "G_src"), digits, cp, cb,
                                                                        C.c_void_p(st.cuda_stream)), "lists_eval_transpose_densities_device")
        return G_src

    def close(self):
        if getattr(self, "_h", None):
            lib().sctl_amd_lists_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_lists_host(name, trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, v_src, v_trg=None, digits=-1, ctx=None, device=0):
    """One-shot sctl_amd_eval_lists_host."""
    plan = ListsPlan(name, r_trg.dtype, trg_off, trg_cnt, src_off, src_cnt, r_trg.size // 3, r_src.size // 3, device=device, ctx=ctx)
    try:
        return plan.eval_host(r_trg, r_src, n_src, v_src, v_trg, digits)
    finally:
        plan.close()


def eval_lists_densities_host(name, trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, F, V_trg=None, digits=-1, ctx=None, device=0):
    """One-shot sctl_amd_eval_lists_densities_host: F of shape (nd, Ns*SrcDim), returns (nd, Nt*k1)."""
    info = kernel_info(name)
    dt = np.dtype(r_trg.dtype)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    F = np.asarray(F)
    if F.ndim != 2 or F.shape[1] != Ns * info["k0"]:
        raise SctlAmdError("densities must have shape (nd, %d)" % (Ns * info["k0"]))
    nd = F.shape[0]
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (trg_off, trg_cnt, src_off, src_cnt)]
    if len({a.size for a in arrs}) != 1:
        raise SctlAmdError("the four list arrays must have one entry per list")
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    if V_trg is None or V_trg.shape != (nd, Nt * info["k1"]):
        V_trg = np.zeros((nd, Nt * info["k1"]), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_eval_lists_densities_host(info["id"], _real_of(dt), nd, arrs[0].size, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), Nt, Ns,
                                                    _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                                    _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(F, dt, nd * Ns * info["k0"], "F"),
                                                    _np_ptr(V_trg, dt, nd * Nt * info["k1"], "V_trg"), digits, cp, cb, device), "eval_lists_densities_host")
    return V_trg


def eval_lists_transpose_host(name, trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, w_trg, g_src=None, digits=-1, ctx=None, device=0):
    """One-shot sctl_amd_eval_lists_transpose_host: a plan of the transposed side only, evaluated once and released."""
    plan = ListsPlan(name, r_trg.dtype, trg_off, trg_cnt, src_off, src_cnt, r_trg.size // 3, r_src.size // 3, device=device, ctx=ctx, directions="transpose")
    try:
        return plan.eval_transpose_host(r_trg, r_src, n_src, w_trg, g_src, digits)
    finally:
        plan.close()


def eval_lists_grad_host(name, trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, v_src, w_trg, g_trg=None, g_src=None, g_nrm=None, want=None, digits=-1,
                         ctx=None, device=0):
    """One-shot sctl_amd_eval_lists_grad_host: both directions planned, the wanted gradients evaluated, the plan released.  Arguments and result as
    ListsPlan.eval_grad_host."""
    info = kernel_info(name)
    dt = np.dtype(r_trg.dtype)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (trg_off, trg_cnt, src_off, src_cnt)]
    if len({a.size for a in arrs}) != 1:
        raise SctlAmdError("the four list arrays must have one entry per list")
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    out = []
    for wanted, g, n in zip(_grad_wanted(info, want), (g_trg, g_src, g_nrm), (Nt * 3, Ns * 3, Ns * 3)):
        out.append(None if not wanted else g if g is not None and g.size == n else np.zeros(n, dtype=dt))
    keep, cp, cb = _ctx_blob(info, ctx)
    ptr = [None if g is None else _np_ptr(g, dt, g.size, what) for g, what in zip(out, ("g_trg", "g_src", "g_nrm"))]
    _check(lib().sctl_amd_eval_lists_grad_host(info["id"], _real_of(dt), arrs[0].size, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), Nt, Ns,
                                               _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"), _np_ptr(n_src, dt, Ns * info["nd"], "n_src"),
                                               _np_ptr(v_src, dt, Ns * info["k0"], "v_src"), _np_ptr(w_trg, dt, Nt * info["k1"], "w_trg"), ptr[0], ptr[1], ptr[2],
                                               digits, cp, cb, device), "eval_lists_grad_host")
    return tuple(out)


def eval_lists_transpose_densities_host(name, trg_off, trg_cnt, src_off, src_cnt, r_trg, r_src, n_src, W_trg, G_src=None, digits=-1, ctx=None, device=0):
    """One-shot sctl_amd_eval_lists_transpose_densities_host: W_trg of shape (nd, Nt*TrgDim), returns (nd, Ns*SrcDim)."""
    info = kernel_info(name)
    dt = np.dtype(r_trg.dtype)
    Nt, Ns = r_trg.size // 3, r_src.size // 3
    W_trg = np.asarray(W_trg)
    if W_trg.ndim != 2 or W_trg.shape[1] != Nt * info["k1"]:
        raise SctlAmdError("weights must have shape (nd, %d)" % (Nt * info["k1"]))
    nd = W_trg.shape[0]
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (trg_off, trg_cnt, src_off, src_cnt)]
    if len({a.size for a in arrs}) != 1:
        raise SctlAmdError("the four list arrays must have one entry per list")
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    if G_src is None or G_src.shape != (nd, Ns * info["k0"]):
        G_src = np.zeros((nd, Ns * info["k0"]), dtype=dt)
    keep, cp, cb = _ctx_blob(info, ctx)
    _check(lib().sctl_amd_eval_lists_transpose_densities_host(info["id"], _real_of(dt), nd, arrs[0].size, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), Nt, Ns,
                                                              _np_ptr(r_trg, dt, Nt * 3, "r_trg"), _np_ptr(r_src, dt, Ns * 3, "r_src"),
                                                              _np_ptr(n_src, dt, Ns * info["nd"], "n_src"), _np_ptr(W_trg, dt, nd * Nt * info["k1"], "W_trg"),
                                                              _np_ptr(G_src, dt, nd * Ns * info["k0"], "G_src"), digits, cp, cb, device),
           "eval_lists_transpose_densities_host")
    return G_src
