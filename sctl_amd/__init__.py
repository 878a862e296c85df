"""sctl_amd — MI355X-native direct kernel summation behind SCTL's kernel-functor interface.

The product is libsctl_amd.so (hand-written HIP for gfx950, C ABI in include/sctl_amd.h) plus the header-only C++
host surface in include/sctl_amd/.  This Python package is plumbing for tests, benchmarks and multi-GPU runs:
ctypes access to the C ABI, torch device memory / streams, and the torch.distributed (RCCL) slab driver.
There is no CPU fallback anywhere in this package: if the library is missing, importing the API raises.
"""
from .api import (DirectOp, GenericKernel, ListsPlan, NearOp, KERNEL_NAMES, eval_lists_host, eval_lists_densities_host, eval_lists_transpose_host, eval_lists_grad_host, eval_lists_transpose_densities_host, load_plugin, counters, device_count, init, finalize, eval_densities_device, eval_densities_host, eval_device, eval_host, eval_grad_device, eval_grad_host, eval_jvp_device, eval_jvp_host, eval_grad_densities_device, eval_grad_densities_host, eval_transpose_device, eval_transpose_host, eval_transpose_densities_device, eval_transpose_densities_host, flops_per_pair, kernel_id,  # noqa: F401
                  kernel_info, kernel_matrix_batch_host, kernel_matrix_device, kernel_matrix_host, last_error, lib, library_path, plan, plan_densities, plan_grad, plan_grad_densities, plan_jvp, plan_transpose, plan_transpose_densities, reset_counters)
from .build import build_library  # noqa: F401

__all__ = ["DirectOp", "GenericKernel", "ListsPlan", "NearOp", "KERNEL_NAMES", "eval_lists_host", "eval_lists_densities_host", "eval_lists_transpose_host", "eval_lists_grad_host", "eval_lists_transpose_densities_host", "load_plugin", "build_library", "counters", "device_count", "init", "finalize", "eval_densities_device", "eval_densities_host", "eval_device", "eval_host", "eval_grad_device", "eval_grad_host", "eval_jvp_device", "eval_jvp_host", "eval_grad_densities_device", "eval_grad_densities_host", "eval_transpose_device", "eval_transpose_host", "eval_transpose_densities_device", "eval_transpose_densities_host", "flops_per_pair",
           "kernel_id", "kernel_info", "kernel_matrix_batch_host", "kernel_matrix_device", "kernel_matrix_host", "last_error", "lib", "library_path", "plan", "plan_densities", "plan_grad", "plan_grad_densities", "plan_jvp", "plan_transpose", "plan_transpose_densities",
           "reset_counters"]
