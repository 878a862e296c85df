/* sctl_amd.h — C ABI of the MI355X (gfx950) direct kernel-summation library, libsctl_amd.so.
 *
 * Drop-in boundary for ONE hot path of SCTL (reference snapshot iostanin1/SCTL @ 2024-11-08; file:line
 * citations are relative to that tree): the all-pairs source->target kernel summation
 *
 *     v_trg[t,k1] += scale * sum_s sum_k0 U(x_t - x_s, n_s)[k0][k1] * v_src[s,k0]
 *
 * that the reference performs in GenericKernel<uKernel>::Eval (include/sctl/generic-kernel.txx:76-189),
 * reached from ParticleFMM::EvalDirect (include/sctl/fmm-wrapper.txx:557) and
 * BoundaryIntegralOp::ComputeFarField (include/sctl/boundary_integral.txx:1063,1073), plus the dense
 * operator build GenericKernel::KernelMatrix (generic-kernel.txx:191-307).
 *
 * Only PODs cross this boundary: plain pointers, sizes, enums.  No C++ types, no torch types.
 * All arrays are contiguous AoS exactly as SCTL's Vector<Real> holds them (generic-kernel.txx:127-129):
 *     r_trg[Nt*3], r_src[Ns*3], n_src[Ns*NormalDim] (NULL when NormalDim == 0), v_src[Ns*SrcDim],
 *     v_trg[Nt*TrgDim].
 * Every function returns SCTL_AMD_OK (0) or a negative error code; sctl_amd_last_error() gives the text
 * for the calling thread.  The reference's convention (SCTL_ASSERT -> abort, common.hpp:59-70) is restored
 * by the header-only C++ wrapper include/sctl_amd/generic-kernel.hpp, not here.
 * Thread safety: every entry point is re-entrant (KernelMatrix is called from inside an OpenMP parallel
 * region by boundary_integral.txx:949-986); there is no global mutable state beyond per-thread error text.
 * There is NO CPU fallback: without a HIP device every compute entry returns SCTL_AMD_ERR_NO_DEVICE.
 */
#ifndef SCTL_AMD_H_
#define SCTL_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCTL_AMD_VERSION 200 /* 0.2.0 */

/* Precision of every array in a call (the reference's template parameter Real). */
enum sctl_amd_real { SCTL_AMD_F64 = 0, SCTL_AMD_F32 = 1 };

/* Kernel identities.  0-7 replace the functors of include/sctl/kernel_functions.hpp:15-198 (same Name()
 * strings, scale factors and FLOPS()); 8 and 9 are functors the reference does not have. */
enum sctl_amd_kernel {
  SCTL_AMD_LAPLACE3D_FXU = 0,    /* "Laplace3D-FxU"    1x1, 1/(4 pi) / r                        kernel_functions.hpp:15-31   */
  SCTL_AMD_LAPLACE3D_DXU = 1,    /* "Laplace3D-DxU"    1x1, normal, (r.n) / r^3                 kernel_functions.hpp:33-51   */
  SCTL_AMD_LAPLACE3D_FXDU = 2,   /* "Laplace3D-FxdU"   1x3, -1/(4 pi) r_j / r^3                 kernel_functions.hpp:53-72   */
  SCTL_AMD_STOKES3D_FXU = 3,     /* "Stokes3D-FxU"     3x3, Stokeslet, 1/(8 pi)                 kernel_functions.hpp:74-95   */
  SCTL_AMD_STOKES3D_DXU = 4,     /* "Stokes3D-DxU"     3x3, normal, stresslet, 3/(4 pi)         kernel_functions.hpp:97-120  */
  SCTL_AMD_STOKES3D_FXT = 5,     /* "Stokes3D-FxT"     3x9, traction tensor, -3/(4 pi)          kernel_functions.hpp:122-146 */
  SCTL_AMD_STOKES3D_FSXU = 6,    /* "Stokes3D-FSxU"    4x3, Stokeslet + source/sink             kernel_functions.hpp:148-172 */
  SCTL_AMD_STOKES3D_FXUP = 7,    /* "Stokes3D-FxUP"    3x4, velocity + pressure                 kernel_functions.hpp:174-198 */
  SCTL_AMD_LAPLACE3D_FDXUDU = 8, /* "Laplace3D-FDxUdU" 2x4, normal, {q, mu} -> {u, grad u}      (new, BASELINE config 2)     */
  SCTL_AMD_HELMHOLTZ3D_FXU = 9,  /* "Helmholtz3D-FxU"  2x2, exp(ikr)/(4 pi r), ctx = {Re k, Im k} as 2 doubles (new, config 5) */
  SCTL_AMD_NUM_KERNELS = 10      /* built-in kernels; ids from here on belong to kernels registered by plugins (below) */
};

enum sctl_amd_status {
  SCTL_AMD_OK = 0,
  SCTL_AMD_ERR_UNKNOWN_KERNEL = -1, /* functor not implemented on the device: caller keeps its own CPU path          */
  SCTL_AMD_ERR_BAD_ARGUMENT = -2,   /* the size checks of generic-kernel.txx:94-97                                     */
  SCTL_AMD_ERR_NO_DEVICE = -3,      /* no HIP device / bad device index: there is no CPU fallback behind this ABI      */
  SCTL_AMD_ERR_HIP = -4,            /* a HIP runtime call failed; text in sctl_amd_last_error()                        */
  SCTL_AMD_ERR_BAD_CONTEXT = -5,    /* kernel needs a context blob (Helmholtz wavenumber) of another size              */
  SCTL_AMD_ERR_PEER = -6            /* rank-parallel call: another rank failed, left or never joined; no rank is left waiting */
};

/* ---- library / registry -------------------------------------------------------------------------------- */
int sctl_amd_version(void);
const char* sctl_amd_last_error(void);          /* message of the last failure on the calling thread ("" if none) */
int sctl_amd_device_count(void);                /* number of HIP devices visible, 0 if none (never an error)       */
/* Optional (everything initialises lazily).  init: touch every visible GPU now, so that the first evaluation does not pay the runtime's
 * first-use cost; returns the number of GPUs (0 without any: not an error) or a negative status.  finalize: give back what the library
 * keeps between calls (sctl_amd_trim + the calling thread's cached streams, device buffers and pinned staging); the library stays
 * usable afterwards.  Neither exists in the reference, whose CPU path has no such state; a patched SCTL calls them from Comm::MPI_Init /
 * MPI_Finalize (comm.txx:117-140) if at all. */
int sctl_amd_init(void);
void sctl_amd_finalize(void);

/* Kernel id for a functor's Name() string (kernel_functions.hpp:16-19), or SCTL_AMD_ERR_UNKNOWN_KERNEL:
 * the "is this kernel supported on the device" query of the header wrapper. */
int sctl_amd_kernel_id(const char* name);
const char* sctl_amd_kernel_name(int kernel);   /* NULL for an unknown id */
/* Shape table: SrcDim, TrgDim, NormalDim (generic-kernel.hpp:59-84), FLOPS() (kernel_functions.hpp:20-22),
 * uKerScaleFactor<double>() (:23-25) and the size in bytes of the context blob the kernel needs (0 = none).
 * Any output pointer may be NULL. */
int sctl_amd_kernel_info(int kernel, int* src_dim, int* trg_dim, int* normal_dim, int* flops, double* scale, int* ctx_bytes);
/* Algorithmic flops per pair interaction by SURVEY.md §8(d): 3 + FLOPS() + 2*SrcDim*TrgDim. */
int sctl_amd_flops_per_pair(int kernel);
int sctl_amd_num_kernels(void);                 /* built-in + registered: valid ids are 0 .. sctl_amd_num_kernels()-1 */

/* ---- user-defined kernel functors (the device side of doc/tutorial/kernels.rst:11-84) ------------------------ */
/* SCTL lets a user write a functor (Name, FLOPS, uKerScaleFactor, uKerMatrix) and get Eval / KernelMatrix for it from
 * GenericKernel<uKernel> (generic-kernel.hpp:31-152).  The device counterpart: the user writes the functor's device form (a struct
 * with pack()/pair(), see include/sctl_amd/device/kernel_plugin.hpp and the built-in ones in device/ukernels.hpp), compiles it
 * with hipcc for gfx950 into a shared object, and registers it; every entry of this ABI then accepts its id, and the header
 * wrappers find it by Name().  desc->launch_table points at the sctl_amd::KernelEntry that device/launch.hpp's
 * make_entry<Ker>() builds (function pointers into the plugin's own code object); abi_version and desc_bytes guard against a
 * plugin compiled with other device headers.  Returns the new kernel id (>= SCTL_AMD_NUM_KERNELS) or a negative error code
 * (a name that is already registered is refused).  Registered kernels live until the process ends. */
#define SCTL_AMD_DEVICE_ABI 4
typedef struct sctl_amd_kernel_desc {
  int abi_version;          /* SCTL_AMD_DEVICE_ABI of the headers the plugin was compiled with */
  int desc_bytes;           /* sizeof(sctl_amd_kernel_desc) */
  int entry_bytes;          /* sizeof(sctl_amd::KernelEntry) */
  int src_dim, trg_dim, normal_dim, flops, ctx_bytes;
  double scale;             /* uKerScaleFactor<double>() */
  const char* name;         /* Name() */
  const void* launch_table; /* const sctl_amd::KernelEntry* */
} sctl_amd_kernel_desc;
int sctl_amd_register_kernel(const sctl_amd_kernel_desc* desc);
/* dlopen()s a plugin; its static initialisers (SCTL_AMD_REGISTER_KERNEL in device/kernel_plugin.hpp) register its kernels.
 * Returns the number of kernels the plugin added, 0 when this very object had been loaded before, or a negative error code —
 * also when the object loads but every registration in it was refused (ABI mismatch, duplicate name, incomplete table:
 * sctl_amd_last_error() carries the reason) or it registers nothing.  A C++ program may instead simply link the plugin's object file. */
int sctl_amd_load_plugin(const char* path);

/* ---- the hot path: GenericKernel::Eval ------------------------------------------------------------------- */
/* Device-resident form.  All five arrays are DEVICE pointers on the current HIP device; `stream` is a
 * hipStream_t (NULL = default stream); the call only enqueues work on that stream and returns.
 * v_trg must already hold Nt*TrgDim values and is ACCUMULATED into (generic-kernel.txx:182-186);
 * resizing-and-zeroing (generic-kernel.txx:98-101) is the host wrapper's job.
 * digits: requested decimal digits, -1 = full precision of `real` (generic-kernel.txx:46-74,77).
 * ctx/ctx_bytes: HOST pointer to the kernel's context blob, copied at launch (replaces the unsized
 * ctx_ptr of generic-kernel.hpp:90,150); NULL/0 for kernels without one. */
int sctl_amd_eval_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                         const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream);

/* The same for a SPATIALLY COMPACT slab of a larger target set: the Nt targets are a contiguous run of the Nt_whole
 * targets in space-filling-curve order, as a rank of a multi-GPU job holds them (fmm-wrapper.txx:504-512 partitions the
 * targets; here the partition follows a Morton curve so that a slab keeps the point density of the whole set).  The
 * result is the same as sctl_amd_eval_device's; Nt_whole informs the choice between the exact kernel and the tile-centred
 * one, which depends on the target density and not on the count, and a proper slab (Nt_whole > Nt) is taken to be in curve order
 * already, so the tile-centred path skips its own sort.  Nt_whole >= Nt. */
int sctl_amd_eval_device_slab(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, const void* r_trg, const void* r_src,
                              const void* n_src, const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes,
                              void* stream);

/* Host-buffer form: the drop-in for GenericKernel<uKer>::Eval<Real,enable_openmp,digits>
 * (generic-kernel.hpp:123) and for the type-erased static entry ParticleFMM stores
 * (generic-kernel.hpp:110, fmm-wrapper.txx:152-153).  All arrays are HOST pointers; the call uploads,
 * evaluates on `device`, downloads and accumulates into v_trg, and returns when v_trg is final. */
int sctl_amd_eval_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                       const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device);

/* Host-buffer form over several GPUs of one node from ONE process: targets are block-partitioned,
 * GPU g of G gets [Nt*g/G, Nt*(g+1)/G) — the rank partition formula of fmm-wrapper.txx:507 — and sources are
 * replicated.  devices == NULL means devices 0..n_devices-1. */
int sctl_amd_eval_host_multi(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                             const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, const int* devices,
                             int n_devices);

/* ---- GenericKernel::KernelMatrix (generic-kernel.txx:191-307) ---------------------------------------------- */
/* M is (Ns*SrcDim) x (Nt*TrgDim), row-major, OVERWRITTEN, scale factor included. */
int sctl_amd_kernel_matrix_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src,
                                  const void* n_src, void* M, int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_kernel_matrix_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src,
                                const void* n_src, void* M, int digits, const void* ctx, int ctx_bytes, int device);

/* Many operator blocks in one launch: block b = KernelMatrix of targets [sum(Nt[:b]), +Nt[b]) of r_trg against sources
 * [sum(Ns[:b]), +Ns[b]) of r_src / n_src, stored (Ns[b]*SrcDim) x (Nt[b]*TrgDim) row-major; the blocks are concatenated in
 * M in batch order.  This is the shape of BoundaryIntegralOp::SetupNear's direct-part subtraction, which calls KernelMatrix
 * once per element on that element's near targets and far-field nodes (boundary_integral.txx:946-1009, Xtrg_near by
 * near_elem_dsp, X_far by elem_nds_dsp_far): one call here replaces that loop.  HOST arrays. */
int sctl_amd_kernel_matrix_batch_host(int kernel, int real, int64_t nbatch, const int64_t* Nt, const int64_t* Ns, const void* r_trg,
                                      const void* r_src, const void* n_src, void* M, int digits, const void* ctx, int ctx_bytes,
                                      int device);

/* ---- device-resident operator: coordinates stay on the GPUs between evaluations ------------------------------- */
/* The MI355X-first form of what ParticleFMM keeps between SetSrcCoord/SetTrgCoord and repeated Eval calls
 * (fmm-wrapper.txx:444-479: the object owns copies of X, Xn, F; boundary_integral.txx:1054,1063: an iterative solver
 * changes only the density between evaluations).  Coordinates are uploaded once — targets block-partitioned over the
 * device list with the formula of fmm-wrapper.txx:507 (with more than one device the blocks are cut from the Morton order
 * of the targets; results always come back in the caller's order), sources replicated — and every sctl_amd_op_eval moves
 * only the density down and the potential up.  A handle may be used from one thread at a time. */
typedef struct sctl_amd_op sctl_amd_op;
int sctl_amd_op_create(int kernel, int real, const int* devices, int n_devices, sctl_amd_op** op);
/* HOST arrays, copied to the devices before returning; either may be called again at any time (new coordinates). */
int sctl_amd_op_set_targets(sctl_amd_op* op, int64_t Nt, const void* r_trg);
int sctl_amd_op_set_sources(sctl_amd_op* op, int64_t Ns, const void* r_src, const void* n_src);
/* The far-field pre/post steps of BoundaryIntegralOp::ComputeFarField, kept on the device (both optional, HOST arrays, NULL clears):
 * weights[Ns]: every evaluation multiplies the uploaded density by the quadrature weights, f[s][k] *= w[s] (boundary_integral.txx:
 * 1040-1052); call after sctl_amd_op_set_sources (new sources drop the weights).  n_trg[Nt*3]: the TrgDim = 3*m output of the kernel is
 * contracted with the target normal, u[t][k] = sum_l v[t][k][l] n_trg[t][l] (:1060-1071), and sctl_amd_op_eval's v_trg then holds
 * Nt*TrgDim/3 values; call after sctl_amd_op_set_targets (new targets drop the normals). */
int sctl_amd_op_set_source_weights(sctl_amd_op* op, const void* weights);
int sctl_amd_op_set_target_normals(sctl_amd_op* op, const void* n_trg);
/* v_src[Ns*SrcDim] and v_trg[Nt*TrgDim] are HOST arrays.  accumulate != 0: v_trg += result (GenericKernel::Eval,
 * generic-kernel.txx:184); accumulate == 0: v_trg = result (ParticleFMM::EvalDirect, fmm-wrapper.txx:501-502). */
int sctl_amd_op_eval(sctl_amd_op* op, const void* v_src, void* v_trg, int accumulate, int digits, const void* ctx, int ctx_bytes);
void sctl_amd_op_destroy(sctl_amd_op* op);

/* ---- several densities against one geometry (block Krylov solves, several incident fields, the six rigid motions of a body) -------- */
/* nd densities on the same sources and targets in one evaluation: what nd calls of the single-density entry compute, with the work of a
 * pair that does not depend on the density (distance, reciprocal square root, Helmholtz's e^{ikr}) done once for several densities.
 * Layout is DENSITY-MAJOR: v_src holds nd consecutive density vectors, [nd][Ns*SrcDim], and v_trg [nd][Nt*TrgDim]; row m is exactly
 * what a single-density call takes and returns.  nd < 0 is SCTL_AMD_ERR_BAD_ARGUMENT, nd == 0 does nothing, and nd == 1 IS the
 * single-density entry (bit-identical results).  Argument errors return the codes of sctl_amd_eval_host, before any device work.
 * The built-in kernels run up to 8 densities (4 for the Stokes kernels with 4 outputs or inputs, the traction and the fused Laplace
 * kernel) per pass on the exact all-pairs kernel; a plugin kernel is evaluated one density at a time on the same stream (correct, no
 * faster).  Counters grow by what nd single calls add.
 * Accuracy: fp64 as the single-density exact kernel at every `digits` (mode_for: seed, Newton, cubic step).  fp32 always runs the exact
 * vector-pipe pair here — there is no matrix-core or tile-centred form of several densities — so an fp32 result has full fp32 accuracy
 * (~5e-7 relative per pair) at every `digits`, also where a single-density call at digits <= 7 would take the bf16 matrix cores. */
/* DEVICE arrays; enqueued on `stream`, accumulated into v_trg. */
int sctl_amd_eval_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                   const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream);
/* HOST arrays, one device; returns when v_trg (accumulated into) is final. */
int sctl_amd_eval_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                 const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device);
/* The operator's far field (as sctl_amd_op_eval) for nd densities, HOST arrays v_src[nd][Ns*SrcDim], v_trg[nd][Nt*TrgDim] (TrgDim/3 with
 * target normals); source weights and target normals apply to every density; any device list. */
int sctl_amd_op_eval_densities(sctl_amd_op* op, int nd, const void* v_src, void* v_trg, int accumulate, int digits, const void* ctx, int ctx_bytes);
/* The plan of such a call (no side effects, no GPU needed): densities per pass of the widest pass and the number of passes (the last pass
 * takes the narrowest form that holds what is left, one density the 2-density form), and of the first pass the targets per lane, source splits, workgroups over all its target
 * launches, and the largest partial-sum workspace of any pass.  The partial sums of one launch stay within 2 GB: a pass cuts its targets
 * into several launches rather than take fewer source splits than the L2 rule asks for.  nd == 1 is sctl_amd_eval_plan's answer. */
int sctl_amd_eval_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* densities_per_pass, int* passes,
                                 int* trg_per_lane, int* src_splits, int64_t* workgroups, int64_t* workspace_bytes);

/* ---- the transposed sum: g_src += A^T w_trg ------------------------------------------------------------------------------------ */
/* With A the operator sctl_amd_eval_* applies, v_trg = A v_src, these entries apply its transpose to a vector of TARGET weights:
 *     g_src[s*SrcDim + k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w_trg[t*TrgDim + k1]
 * i.e. KernelMatrix (generic-kernel.txx:191-307, (Ns*SrcDim) x (Nt*TrgDim)) times w_trg, without the matrix: the adjoint a BiCG / QMR /
 * LSQR iteration, an adjoint solve or a norm estimate needs, and the gradient of <w, A v_src> with respect to v_src.  The normals stay
 * with the sources, a coincident pair contributes 0, and `digits`, `ctx` and every argument check are those of the forward entries; a
 * registered kernel whose functor has no transposed form (no pair_t: device/kernel_plugin.hpp) is SCTL_AMD_ERR_UNKNOWN_KERNEL here and
 * evaluates forward as before.  The exact all-pairs kernel on one device (device/eval_transpose_kernel.hpp): sums in a fixed order,
 * bit-reproducible.  Counters grow by Nt*Ns pairs.  Nt == 0 or Ns == 0: nothing is read or written. */
/* DEVICE arrays; enqueued on `stream`; g_src (Ns*SrcDim values) is accumulated into. */
int sctl_amd_eval_transpose_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                   const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream);
/* HOST arrays, one device; returns when g_src is final.  accumulate != 0 adds to g_src, 0 overwrites it. */
int sctl_amd_eval_transpose_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                 const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes, int device);
/* The plan of such a call (no side effects, no GPU needed): sources per lane, splits of the target range, and the bytes of partial sums
 * of one launch.  Those stay within 2 GB: the sources are cut into several launches rather than the targets into fewer splits. */
int sctl_amd_eval_transpose_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* src_per_lane, int* splits, int64_t* workspace_bytes);

/* ---- several weight vectors through the transposed sum: g_src[m] += A^T w_trg[m] --------------------------------------------------- */
/* nd weight vectors on the same targets and sources in one evaluation: what nd calls of the single transposed entry compute,
 *     g_src[m][s*SrcDim + k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w_trg[m][t*TrgDim + k1],   m = 0 .. nd-1,
 * with the work of a pair that does not depend on the weights (distance, reciprocal square root, d.n, Helmholtz's e^{ikr}) done once for
 * several of them: A^T W for the block a block BiCG / QMR / LSQR iteration sent through A V (sctl_amd_eval_densities_*), an adjoint solve
 * for several right-hand sides, back-propagation through sctl_amd_eval_densities_*.  Layout is ROW-MAJOR as there: w_trg holds nd
 * consecutive weight vectors, [nd][Nt*TrgDim], and g_src [nd][Ns*SrcDim]; row m is exactly what a single transposed call takes and
 * returns.  nd < 0 is SCTL_AMD_ERR_BAD_ARGUMENT, nd == 0 does nothing, and nd == 1 IS the single transposed entry (bit-identical results,
 * the same plan).  Argument errors return the codes of sctl_amd_eval_transpose_*, before any device work.  The built-in kernels run up to 8
 * weight vectors per pass (4 for the traction kernel) on the exact all-pairs kernel (csrc/rows_kernel.hpp): sums in a fixed
 * order, bit-reproducible; a registered kernel with pair_t (which has no several-vectors form) is evaluated one row at a time on the same
 * stream, one without pair_t is SCTL_AMD_ERR_UNKNOWN_KERNEL.  fp32 runs this exact pair at every `digits`, as the single transposed entry
 * does.  Counters grow by nd*Nt*Ns pairs.  Several weight vectors over the P2P lists:
 * sctl_amd_lists_eval_transpose_densities_*; the near field and the operator handle have their forms too
 * (sctl_amd_near_apply_transpose_densities_*, sctl_amd_op_eval_transpose_densities).  Not provided: an all-pairs multi-GPU form. */
/* DEVICE arrays; enqueued on `stream`; g_src is accumulated into. */
int sctl_amd_eval_transpose_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                             const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream);
/* HOST arrays, one device; returns when g_src is final.  accumulate != 0 adds to g_src, 0 overwrites it. */
int sctl_amd_eval_transpose_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                           const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes, int device);
/* The plan of such a call (no side effects, no GPU needed): weight vectors per pass of the widest pass and the number of passes (the last
 * pass takes the narrowest form that holds what is left, one vector the form of 2), and of the first pass the sources per lane, the splits
 * of the target range, the workgroups over all its source launches, and the largest partial-sum workspace of any pass.  The partial sums
 * of one launch stay within 2 GB: a pass cuts its sources into several launches rather than take fewer splits than the L2 rule asks for.
 * nd == 1 is sctl_amd_eval_transpose_plan's answer. */
int sctl_amd_eval_transpose_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* vectors_per_pass, int* passes,
                                           int* src_per_lane, int* splits, int64_t* workgroups, int64_t* workspace_bytes);

/* ---- gradients of <w_trg, A v_src> with respect to the geometry ------------------------------------------------------------------ */
/* With L = sum_t sum_k1 w_trg[t*TrgDim + k1] * v_trg[t*TrgDim + k1], v_trg = A v_src as sctl_amd_eval_* computes it, d = x_t - x_s and the pair's scalar
 *     phi_ts = sum_k0 sum_k1 w_trg[t*TrgDim + k1] * U(d, n_s)[k0][k1] * v_src[s*SrcDim + k0],
 * these entries add the derivatives of L with respect to the coordinates of both point sets and to the source normals:
 *     g_trg[t*3 + j] +=  scale * sum_s d phi_ts / d d_j        (Nt x 3)
 *     g_src[s*3 + j] += -scale * sum_t d phi_ts / d d_j        (Ns x 3)
 *     g_nrm[s*3 + j] +=  scale * sum_t d phi_ts / d n_j        (Ns x NormalDim; kernels with a normal only)
 * — forces of a pair potential, shape derivatives of a boundary, the geometry half of a differentiable kernel sum (the density half is
 * sctl_amd_eval_transpose_*).  Any of the three outputs may be null and is then not computed; g_trg comes from a pass whose lanes own targets, g_src and
 * g_nrm together from one whose lanes own sources, and a pass none of whose outputs is asked for is not launched.  g_nrm non-null for a kernel without a
 * normal is SCTL_AMD_ERR_BAD_ARGUMENT.  A coincident pair contributes 0 to all three; Helmholtz: v_src, w_trg are (re, im) pairs, L is the real sum over
 * both components, and k is not differentiated.  `digits`, `ctx` and the argument checks are those of the forward and transposed entries; a registered
 * kernel whose functor has no gradient form (no pair_g: device/kernel_plugin.hpp) is SCTL_AMD_ERR_UNKNOWN_KERNEL here only.  The exact all-pairs scheme
 * on one device (device/eval_grad_kernel.hpp): sums in a fixed order, no atomics, bit-reproducible.  Counters grow by Nt*Ns pairs per pass launched.
 * Nt == 0 or Ns == 0: nothing is read or written. */
/* DEVICE arrays; enqueued on `stream`; the outputs are accumulated into. */
int sctl_amd_eval_grad_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                              const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes, void* stream);
/* HOST arrays, one device; returns when the outputs are final.  accumulate != 0 adds to them, 0 overwrites them. */
int sctl_amd_eval_grad_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                            const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int accumulate, int digits, const void* ctx, int ctx_bytes, int device);
/* The plan of such a call (no side effects, no GPU needed), per pass: owners per lane, splits of the streamed range, and the bytes of partial sums of
 * one launch (3 sums per target; 3, or 6 with a normal, per source).  Those stay within 2 GB: the owners are cut into several launches rather than the
 * streamed set into fewer splits. */
int sctl_amd_eval_grad_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* trg_per_lane, int* trg_splits, int64_t* trg_workspace_bytes,
                            int* src_per_lane, int* src_splits, int64_t* src_workspace_bytes);

/* ---- geometry gradients for several density / weight rows in one pass ---------------------------------------------------------------- */
/* nd density rows v_src[m] and nd weight rows w_trg[m] on the same geometry: for L = sum_m <w_trg[m], A v_src[m]> — several incident fields, the six
 * rigid motions of a body, the block of a block Krylov adjoint — the outputs are the SUMS over m of what nd calls of sctl_amd_eval_grad_* add,
 *     g_trg (Nt x 3), g_src (Ns x 3), g_nrm (Ns x 3): one of each whatever nd is,
 * with the work of a pair that does not depend on the rows (distance, reciprocal square root and its refinement, the powers of 1/r, d.n, Helmholtz's
 * e^{ikr}) done once for several of them.  Layout is ROW-MAJOR as in sctl_amd_eval_densities_*: v_src is [nd][Ns*SrcDim], w_trg [nd][Nt*TrgDim].
 * nd < 0 is SCTL_AMD_ERR_BAD_ARGUMENT, nd == 0 does nothing, and nd == 1 IS sctl_amd_eval_grad_* (bit-identical results, the same plan).  Everything
 * else is as there: any output may be null and is then not computed, a pass none of whose outputs is asked for is not launched, g_nrm for a kernel
 * without a normal is SCTL_AMD_ERR_BAD_ARGUMENT, argument errors come before any device work, Nt == 0 or Ns == 0 touches nothing.  The built-in
 * kernels run up to 8 rows per pass (4 for the traction kernel) on csrc/multi_grad_kernel.hpp: sums in a fixed order, no atomics, bit-reproducible;
 * a registered kernel with pair_g but no pair_gm is evaluated one row at a time into the same outputs on the same stream (exact: the outputs are
 * sums), one without pair_g is SCTL_AMD_ERR_UNKNOWN_KERNEL.  Counters grow by nd*Nt*Ns pairs per side launched.  Not provided: the P2P lists, the near
 * operator, the operator handle and any multi-GPU form. */
/* DEVICE arrays; enqueued on `stream`; the outputs are accumulated into. */
int sctl_amd_eval_grad_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                        const void* v_src, const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes,
                                        void* stream);
/* HOST arrays, one device; returns when the outputs are final.  accumulate != 0 adds to them, 0 overwrites them. */
int sctl_amd_eval_grad_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                      const void* v_src, const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int accumulate, int digits, const void* ctx,
                                      int ctx_bytes, int device);
/* The plan of such a call (no side effects, no GPU needed): rows per pass of the widest pass and the number of passes (the last pass takes the
 * narrowest form that holds what is left, one row the form of 2), and per side the splits of the streamed range of the first pass and the largest
 * partial-sum workspace of one launch of any pass: [splits][owners * 3] (6 for the sources of a kernel with a normal), without a factor nd.  It stays
 * within 2 GB as the single gradient's does, by cutting the owners into launches.  nd == 1 is sctl_amd_eval_grad_plan's answer. */
int sctl_amd_eval_grad_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* rows_per_pass, int* passes, int* trg_splits,
                                      int64_t* trg_workspace_bytes, int* src_splits, int64_t* src_workspace_bytes);

/* ---- directional derivative (tangent) of v_trg = A v_src along a perturbation of the geometry ------------------------------------------- */
/* The forward-mode counterpart of sctl_amd_eval_grad_*.  With d = x_t - x_s, a perturbation d_trg of the target coordinates (Nt x 3), d_src of the
 * source coordinates (Ns x 3) and d_nrm of the source normals (Ns x NormalDim), and the densities held fixed, these entries add the tangent of the
 * whole field:
 *     dv_trg[t*TrgDim + k1] += scale * sum_s sum_k0 [(e . grad_d) U(d, n_s) + (d_nrm_s . grad_n) U(d, n_s)][k0][k1] * v_src[s*SrcDim + k0],
 *     e = d_trg[t] - d_src[s],
 * scaled as sctl_amd_eval_* scales v_trg — J delta for Gauss-Newton and Newton-Krylov on shapes and placements, the linearisation of a boundary
 * integral about a moving surface, the sensitivity of a field to one design parameter; <w, dv_trg> = <g_trg, d_trg> + <g_src, d_src> + <g_nrm, d_nrm>
 * with the outputs of sctl_amd_eval_grad_* for the weights w.  The tangent with respect to the densities is A dv_src: the caller adds it with
 * sctl_amd_eval_device into the same array.  Any of the three tangents may be null and is then a field of zeros (bit for bit the call with an array
 * of zeros in its place); with all three null nothing is launched.  d_nrm non-null for a kernel without a normal is SCTL_AMD_ERR_BAD_ARGUMENT.  A
 * coincident pair contributes 0; Helmholtz: v_src, dv_trg are (re, im) pairs, and k is not differentiated.  `digits`, `ctx` and the argument checks
 * are those of the forward entries, and they come before any device work.  The exact all-pairs scheme on one device (csrc/jvp_kernel.hpp): the
 * targets own the sums, the sources stream; sums in a fixed order, no atomics, bit-reproducible.  Counters grow by Nt*Ns pairs.  Nt == 0 or Ns == 0:
 * nothing is read or written.  Built for the ten built-in kernels: a registered (plugin) kernel is SCTL_AMD_ERR_UNKNOWN_KERNEL here only.  Not
 * provided: the P2P lists, several density rows in one pass, plugin kernels, the operator handle and any multi-GPU form. */
/* DEVICE arrays; enqueued on `stream`; dv_trg is accumulated into. */
int sctl_amd_eval_jvp_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                             const void* d_trg, const void* d_src, const void* d_nrm, void* dv_trg, int digits, const void* ctx, int ctx_bytes, void* stream);
/* HOST arrays, one device; returns when dv_trg is final.  accumulate != 0 adds to it, 0 overwrites it. */
int sctl_amd_eval_jvp_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                           const void* d_trg, const void* d_src, const void* d_nrm, void* dv_trg, int accumulate, int digits, const void* ctx, int ctx_bytes,
                           int device);
/* The plan of such a call (no side effects, no GPU needed): targets per lane, splits of the source range, and the bytes of partial sums of one launch
 * (TrgDim sums per target).  Those stay within 2 GB: the targets are cut into several launches rather than the sources into fewer splits. */
int sctl_amd_eval_jvp_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* trg_per_lane, int* splits, int64_t* workspace_bytes);

/* ---- rank-parallel evaluation: one process per GPU (ParticleFMM::EvalDirect under MPI, fmm-wrapper.txx:504-561) --------------- */
/* The reference partitions targets and sources over MPI ranks and rotates the source blocks round a ring (:537-558).  Here every
 * rank keeps ITS targets, and the sources (and, per evaluation, the densities) of ALL ranks are all-gathered into each rank's
 * device-resident operator: over RCCL / xGMI, GPU buffer to GPU buffer, when every rank drives its own GPU.  There is no MPI
 * behind this: ranks meet through a TCP rendezvous (rank 0 listens on master_addr:master_port; dotted IPv4), which carries the
 * RCCL unique id, the small host-side collectives below, and — when ranks SHARE a GPU, which RCCL refuses: a one-GPU rehearsal —
 * the data itself.  create() is collective (every rank calls it; blocks until all have connected).  device: the HIP device of
 * this rank, or -1 for a host-only communicator (the host collectives work without any GPU).  flags: SCTL_AMD_COMM_SOCKETS_ONLY
 * keeps RCCL out even when it could be used. */
typedef struct sctl_amd_comm sctl_amd_comm;
enum { SCTL_AMD_COMM_SOCKETS_ONLY = 1, SCTL_AMD_COMM_FORCE_RCCL = 2 /* size == 1 only: build a one-rank RCCL communicator (for sctl_amd_comm_selftest) */ };
enum { SCTL_AMD_COMM_SOCKETS = 0, SCTL_AMD_COMM_RCCL = 1 };   /* sctl_amd_comm_info: transport of the data path */
int sctl_amd_comm_create(int rank, int size, const char* master_addr, int master_port, int device, int flags, sctl_amd_comm** comm);
int sctl_amd_comm_info(const sctl_amd_comm* comm, int* rank, int* size, int* device, int* transport);
/* Host-side collectives over the rendezvous sockets (counts, small arrays): every rank contributes send_bytes bytes, recv gets
 * the concatenation in rank order (at most recv_capacity bytes) and bytes_of_rank[size] the contributions. */
int sctl_amd_comm_allgatherv_host(sctl_amd_comm* comm, const void* send, int64_t send_bytes, void* recv, int64_t recv_capacity, int64_t* bytes_of_rank);
int sctl_amd_comm_barrier(sctl_amd_comm* comm);
/* Checks the RCCL data path: every rank sends `bytes` bytes to its right neighbour (itself, with one rank) with the grouped
 * ncclSend / ncclRecv the gathers use, and verifies what arrives.  Collective.  BAD_ARGUMENT if the data path is the sockets. */
int sctl_amd_comm_selftest(sctl_amd_comm* comm, int64_t bytes);
void sctl_amd_comm_destroy(sctl_amd_comm* comm);
/* Collective forms of sctl_amd_op_set_sources / sctl_amd_op_eval for an operator with ONE device (this rank's): the operator's
 * sources become the concatenation, in rank order, of all ranks' Ns_local sources (HOST arrays); eval_dist gathers the ranks'
 * densities the same way and evaluates THIS rank's targets (set with sctl_amd_op_set_targets), v_trg holding their Nt*TrgDim
 * values.  Every rank must call them, in the same order; a rank may own no sources or no targets. */
int sctl_amd_op_set_sources_dist(sctl_amd_op* op, sctl_amd_comm* comm, int64_t Ns_local, const void* r_src, const void* n_src);
int sctl_amd_op_eval_dist(sctl_amd_op* op, sctl_amd_comm* comm, int64_t Ns_local, const void* v_src_local, void* v_trg, int accumulate, int digits,
                          const void* ctx, int ctx_bytes);

/* ---- BoundaryIntegralOp near field: ComputeNearInterac (boundary_integral.txx:1079-1142) -------------------------- */
/* The step that follows the far field in ComputePotential (:608-614): for every element the precomputed operator block
 * K_near_ ((elem_nds_cnt[e]*src_dim) x (near_elem_cnt[e]*trg_dim), row-major) is applied to the element's density,
 * U_ = F_ . K_near_ (:1092-1102); the results are permuted by near_scatter_index (ScatterForward, :1129: out[i] =
 * in[index[i]]) and each target adds its near_trg_cnt[i] entries starting at near_trg_dsp[i] (:1131-1140).
 * create() takes exactly the HOST arrays BoundaryIntegralOp::SetupNear leaves behind (:816-1012) and keeps them on the
 * device; K_near is the concatenation of the blocks in element order (the reference's K_near with K_near_dsp, :854-857).
 * K_near_cnt may be NULL (every block present); K_near_cnt[e] == 0 marks an element without a matrix (MatrixFree, :849),
 * whose near targets receive nothing from this routine.  trg_dim is the number of potential components per target
 * (KDIM1, or KDIM1/3 when the operator was set up with trg_normal_dot_prod, :1080).
 * apply: F holds sum(elem_nds_cnt)*src_dim densities in element order; U (Ntrg*trg_dim) is ACCUMULATED into.
 * A handle may be used from one thread at a time. */
typedef struct sctl_amd_near sctl_amd_near;
int sctl_amd_near_create(int real, int device, int64_t Nelem, int src_dim, int trg_dim, const int64_t* elem_nds_cnt,
                         const int64_t* near_elem_cnt, const int64_t* K_near_cnt, const void* K_near, int64_t Ntrg,
                         const int64_t* near_scatter_index, const int64_t* near_trg_cnt, const int64_t* near_trg_dsp,
                         sctl_amd_near** op);
int sctl_amd_near_apply_host(sctl_amd_near* op, const void* F, void* U);                   /* HOST arrays            */
int sctl_amd_near_apply_device(sctl_amd_near* op, const void* F, void* U, void* stream);   /* DEVICE arrays, enqueue */
/* Sizes of an operator: density and potential lengths, near-list entries, bytes of K_near resident in HBM (the
 * algorithmic traffic of one application), workgroups of the GEMV launch.  Any output pointer may be NULL. */
/* The whole of BoundaryIntegralOp::ComputePotential (boundary_integral.txx:608-614: far field, then the near-zone correction added
 * to it) on the devices of a direct-sum operator handle.  set_near attaches the near-field operator of the same BoundaryIntegralOp —
 * the arrays of sctl_amd_near_create, for the operator's CURRENT targets (Ntrg = the Nt of sctl_amd_op_set_targets; call again
 * after new targets) — block-partitioned like the targets: device g keeps, of every element block, the columns whose targets lie
 * in its slab.  eval_potential then uploads both densities once (v_src_far at the far-field nodes, f_near at the element nodes:
 * sum(elem_nds_cnt)*SrcDim values), runs far field (+ weights, + target-normal contraction) and near field back to back on each
 * device's stream, the near field ACCUMULATING into the far-field result where it lies, and downloads the potential once.
 * trg_dim: TrgDim, or TrgDim/3 when target normals are set.  Results equal sctl_amd_op_eval followed by sctl_amd_near_apply_host up
 * to the order in which the far field and a target's near entries are added (and do not depend on the number of devices).
 * Nelem = 0 with null arrays detaches. */
int sctl_amd_op_set_near(sctl_amd_op* op, int src_dim, int trg_dim, int64_t Nelem, const int64_t* elem_nds_cnt, const int64_t* near_elem_cnt,
                         const int64_t* K_near_cnt, const void* K_near, const int64_t* near_scatter_index, const int64_t* near_trg_cnt,
                         const int64_t* near_trg_dsp);
int sctl_amd_op_eval_potential(sctl_amd_op* op, const void* v_src_far, const void* f_near, void* v_trg, int accumulate, int digits, const void* ctx,
                               int ctx_bytes);

/* ---- several densities through the near field and ComputePotential ------------------------------------------------------------- */
/* nd densities against one near-field operator: U_ = F_ . K_near_ with nd rows in F_ (the reference writes the step as
 * Matrix::GEMM(U_, F_, K_near_), boundary_integral.txx:1092-1102), every operator entry read from HBM ONCE per pass instead of once
 * per density, then the scatter and the per-target accumulation (:1129-1140) with a target's indices read once for all rows.
 * Density-major: F[nd][density_len], U[nd][Ntrg*trg_dim]; row m is what sctl_amd_near_apply_* takes and returns, and every row of U
 * is ACCUMULATED into.  nd == 1 IS the single-density entry (bit-identical), nd == 0 does nothing, nd < 0 is
 * SCTL_AMD_ERR_BAD_ARGUMENT; argument errors come back before any device work.  Any nd is legal: a call runs passes of 8 densities
 * (fp64 and fp32 alike) and a last pass of the narrowest form (2, 4 or 8) that takes what is left, one density left over going through
 * the single-density kernels.  Within a several-densities pass a row's terms are summed in another order than the single-density
 * kernel's (fewer partial sums per density), so row m agrees with a single application to rounding, not bit for bit; results are
 * bit-identical from run to run.  The workspace of a pass belongs to the handle and is allocated on the first several-densities call. */
int sctl_amd_near_apply_densities_host(sctl_amd_near* op, int nd, const void* F, void* U);                   /* HOST arrays            */
int sctl_amd_near_apply_densities_device(sctl_amd_near* op, int nd, const void* F, void* U, void* stream);   /* DEVICE arrays, enqueue */
/* sctl_amd_op_eval_potential (ComputePotential, boundary_integral.txx:608-614) for nd densities, HOST arrays v_src_far[nd][Ns*SrcDim],
 * f_near[nd][sum(elem_nds_cnt)*SrcDim], v_trg[nd][Nt*trg_dim]: on every device of the handle all densities go down once, the far field
 * runs as sctl_amd_op_eval_densities does (weights and target normals applied to every row; its pass widths per kernel and precision),
 * the near field of all rows (passes of up to 8) is accumulated into the far-field result where it lies, and the potential comes up
 * once.  Errors as sctl_amd_op_eval_potential; nd == 1 is that entry, nd == 0 does nothing after the argument checks. */
int sctl_amd_op_eval_potential_densities(sctl_amd_op* op, int nd, const void* v_src_far, const void* f_near, void* v_trg, int accumulate,
                                         int digits, const void* ctx, int ctx_bytes);

/* ---- the adjoint of the near field and of ComputePotential --------------------------------------------------------------------- */
/* G += N^T W for the near-field operator N of sctl_amd_near_apply_* (U += N F): W[Ntrg*trg_dim] is gathered into near-list order
 * (Wn[near_scatter_index[p]*trg_dim + k] = W[i*trg_dim + k] for the entries p of target i, the inverse of the per-target
 * accumulation) and every element's block is applied transposed, G[f_off_e + s] += sum_t K_e[s][t] Wn[u_off_e + t]; G has
 * density_len values and is ACCUMULATED into.  Every entry of K_near is read once per application; the sums go across the lanes of a
 * wave by a fixed tree (no atomics), so results are bit-identical from run to run.  Elements without a matrix (K_near_cnt[e] == 0) or
 * without near targets add nothing: their entries of G keep their bits.  What the transposed direction needs beyond the forward's
 * device arrays (its work list, the gathered W) is allocated on the first transposed call, not by sctl_amd_near_create.  That first call
 * therefore allocates and copies the work list synchronously before it enqueues (it cannot be captured into a graph); later calls only enqueue.  Null handle
 * or arrays: SCTL_AMD_ERR_BAD_ARGUMENT before any device work; an operator without entries returns SCTL_AMD_OK and touches nothing.
 * Several weight vectors per call: sctl_amd_near_apply_transpose_densities_* below. */
int sctl_amd_near_apply_transpose_host(sctl_amd_near* op, const void* W, void* G);                   /* HOST arrays, G accumulated into            */
int sctl_amd_near_apply_transpose_device(sctl_amd_near* op, const void* W, void* G, void* stream);   /* DEVICE arrays, enqueue, G accumulated into */
/* The adjoint of sctl_amd_op_eval (g_src = D_w A^T C_n^T w) and of sctl_amd_op_eval_potential (that, and g_near = N^T w) on the
 * operator's devices: A the far-field kernel sum, D_w the source weights and C_n the contraction with the target normals where they
 * are set, N the attached near field.  HOST arrays: w_trg[Nt*TrgDim] (Nt*TrgDim/3 with target normals), g_src / g_src_far[Ns*SrcDim],
 * g_near[sum(elem_nds_cnt)*SrcDim].  Every device takes its target slab of w (in the operator's own target order), expands it with the
 * normals, runs the transposed kernel sum of the slab against all sources, scales by the weights and applies its near sub-operator
 * transposed on the same stream; the host adds the devices' partial results in device order, so results agree between device lists to
 * rounding, not bit for bit.  accumulate != 0 adds to the output arrays, else they are overwritten.  Errors as
 * sctl_amd_op_eval_potential; a registered kernel whose functor supplies no pair_t gives SCTL_AMD_ERR_UNKNOWN_KERNEL.  The counters
 * grow by Nt*Ns.  There are no rank-parallel (_dist) forms of these entries. */
int sctl_amd_op_eval_transpose(sctl_amd_op* op, const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes);
int sctl_amd_op_eval_potential_transpose(sctl_amd_op* op, const void* w_trg, void* g_src_far, void* g_near, int accumulate, int digits,
                                         const void* ctx, int ctx_bytes);

/* ---- several weight vectors through the adjoint of the near field and of ComputePotential ----------------------------------------- */
/* G[m] += N^T W[m] for nd weight vectors against one near-field operator, every entry of K_near read from HBM ONCE per pass instead of
 * once per vector, a target's scatter indices read once for all rows of the gather.  Row-major, the layouts of
 * sctl_amd_near_apply_densities_*: W[nd][Ntrg*trg_dim], G[nd][density_len]; row m is what sctl_amd_near_apply_transpose_* takes and
 * returns, and every row of G is ACCUMULATED into.  nd == 1 IS the single-vector entry (bit-identical), nd == 0 does nothing, nd < 0 is
 * SCTL_AMD_ERR_BAD_ARGUMENT; null handle or arrays are reported as the single entries report them, before any device work.  Any nd is
 * legal: fp64 runs passes of 4 vectors and a last pass of the narrower form (2 or 4) that takes what is left, fp32 passes of 2 (its form
 * of 4 measured slower than four single calls; a form of 8 does not fit the registers), one vector left over going through the
 * single-vector kernels.  The sums use the single-vector kernel's order of additions in a lane and its tree
 * across lanes (no atomics): results are bit-identical from run to run and between the host and the device entry.  Entries of G that
 * belong to elements without a matrix or without near targets keep their bits in every row.  The gathered weights of a pass,
 * M * near_entries * trg_dim values for the widest pass M the handle has run, belong to the handle; they are allocated and zero-filled
 * on the first several-vectors call (on the caller's stream) and grow with the widest pass.  If they cannot be allocated the call
 * returns SCTL_AMD_ERR_HIP and the handle stays usable.  The host entry keeps nd * (density_len + Ntrg*trg_dim) values of device and
 * pinned staging memory, shared with sctl_amd_near_apply_densities_host.  Not provided: the P2P lists and rank-parallel forms. */
int sctl_amd_near_apply_transpose_densities_host(sctl_amd_near* op, int nd, const void* W, void* G);                   /* HOST arrays            */
int sctl_amd_near_apply_transpose_densities_device(sctl_amd_near* op, int nd, const void* W, void* G, void* stream);   /* DEVICE arrays, enqueue */
/* sctl_amd_op_eval_transpose / _potential_transpose for nd weight vectors, HOST arrays w_trg[nd][Nt*TrgDim] (Nt*TrgDim/3 with target
 * normals), g_src / g_src_far[nd][Ns*SrcDim], g_near[nd][sum(elem_nds_cnt)*SrcDim]: on every device the slab of every row of w goes
 * down once, the normals expand every row, the far leg runs as sctl_amd_eval_transpose_densities_device does (its pass widths per
 * kernel and precision), the weights scale every row, the near sub-operator takes all rows through
 * sctl_amd_near_apply_transpose_densities_device on the same stream, and the results come up once; the host adds the devices' partial
 * results in device order, row by row.  Errors as the single entries; nd < 0 is SCTL_AMD_ERR_BAD_ARGUMENT, nd == 0 does nothing after
 * the argument checks, nd == 1 runs exactly what the single entries run.  The counters grow by nd*Nt*Ns. */
int sctl_amd_op_eval_transpose_densities(sctl_amd_op* op, int nd, const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx,
                                         int ctx_bytes);
int sctl_amd_op_eval_potential_transpose_densities(sctl_amd_op* op, int nd, const void* w_trg, void* g_src_far, void* g_near, int accumulate,
                                                   int digits, const void* ctx, int ctx_bytes);

int sctl_amd_near_info(const sctl_amd_near* op, int64_t* density_len, int64_t* potential_len, int64_t* near_entries,
                       int64_t* operator_bytes, int64_t* workgroups);
void sctl_amd_near_destroy(sctl_amd_near* op);

/* ---- batched list evaluation: many (target range x source range) direct sums in ONE launch ------------------------ */
/* The near-field (P2P, U-list) shape of a tree code — SURVEY.md §8f row 4, second half: PVFMM calls the kernel once per
 * (target box, source box) pair through pvfmm::GenericKernel<PVFMMKernelFn_<Ker>> on sub-ranges of the particle arrays
 * (fmm-wrapper.txx:756-786); boxes hold 1-500 points, so on a GPU the pairs must share a launch.  List l adds to the targets
 * [trg_off[l], trg_off[l] + trg_cnt[l]) the potential of the sources [src_off[l], src_off[l] + src_cnt[l]):
 *     v_trg[t] += scale * sum_{s in list l} U(x_t - x_s, n_s) v_src[s]         (ACCUMULATED into, like GenericKernel::Eval)
 * Offsets and counts are in POINTS.  The target ranges of any two lists must be IDENTICAL or DISJOINT (the leaf boxes of a
 * tree): every target is then owned by one wave, sums run in list order in registers and are written once — deterministic, no
 * atomics; anything else is SCTL_AMD_ERR_BAD_ARGUMENT.  Source ranges may overlap freely.  The four index arrays are HOST
 * arrays (nlists entries each), read by create() only.
 * A plan keeps the grouped, cost-ordered work list on `device`; evaluating it is one kernel launch.  eval_device: DEVICE
 * arrays on the plan's device, which must be the current device; enqueues on `stream` and returns.  eval_host: HOST arrays.
 * A handle may be used from one thread at a time. */
typedef struct sctl_amd_lists sctl_amd_lists;
int sctl_amd_lists_create(int kernel, int real, int device, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                          const int64_t* src_cnt, int64_t Nt, int64_t Ns, sctl_amd_lists** plan);
int sctl_amd_lists_eval_device(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg,
                               int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_lists_eval_host(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg,
                             int digits, const void* ctx, int ctx_bytes);
/* pair interactions of one evaluation, work items (waves) and source ranges of the launch.  NULL = skip. */
int sctl_amd_lists_info(const sctl_amd_lists* plan, int64_t* pairs, int64_t* work_items, int64_t* source_ranges);
void sctl_amd_lists_destroy(sctl_amd_lists* plan);
/* One-shot forms (plan, evaluate, release).  _device: arrays on the current device; returns after the stream has finished. */
int sctl_amd_eval_lists_device(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                               const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                               const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_eval_lists_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                             const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                             const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device);

/* ---- the transposed sum over the lists: g_src += A^T w_trg, the adjoint of sctl_amd_lists_eval_* over the same lists ----
 *     g_src[s*SrcDim + k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w_trg[t*TrgDim + k1]
 * with the conventions of sctl_amd_eval_transpose_*: d = x_t - x_s keeps the forward sign, the normal stays with the source, a coincident
 * pair contributes 0, digits / ctx / scale as in the forward entries, fp32 runs the exact vector-pipe pair; g_src is ACCUMULATED into.
 * A plan serves the directions it was made for: `directions` is a bit set of SCTL_AMD_LISTS_FORWARD and SCTL_AMD_LISTS_TRANSPOSE
 * (sctl_amd_lists_create means FORWARD).  The transposed side asks of the SOURCE ranges what the forward side asks of the target ranges:
 * any two must be IDENTICAL or DISJOINT, so that every source is owned by one wave, its sums run in list order in registers and are
 * written once — no atomics, no partial-sum workspace, bit-identical results from run to run.  Each direction checks its own rule only:
 * a TRANSPOSE-only plan may have overlapping target ranges, a FORWARD-only plan overlapping source ranges.  directions of 0 or with an
 * unknown bit, and evaluating a direction the plan was not made for, are SCTL_AMD_ERR_BAD_ARGUMENT; a kernel without a transposed form
 * (a plugin functor without pair_t) gets SCTL_AMD_ERR_UNKNOWN_KERNEL from a create that asks for TRANSPOSE.  The counters grow by the
 * plan's pairs.  _host reuses the handle's stream, staging and device buffers (w_trg has the size of v_trg, g_src that of v_src).
 * Several weight vectors: sctl_amd_lists_eval_transpose_densities_* below; geometry gradients: sctl_amd_lists_eval_grad_*.  Not built: several GPUs over lists. */
#define SCTL_AMD_LISTS_FORWARD 1
#define SCTL_AMD_LISTS_TRANSPOSE 2
int sctl_amd_lists_create_directions(int kernel, int real, int device, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt,
                                     const int64_t* src_off, const int64_t* src_cnt, int64_t Nt, int64_t Ns, int directions, sctl_amd_lists** plan);
int sctl_amd_lists_eval_transpose_device(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg, void* g_src,
                                         int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_lists_eval_transpose_host(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg, void* g_src,
                                       int digits, const void* ctx, int ctx_bytes);
/* pair interactions of one transposed evaluation, its work items (waves) and target ranges; all 0 for a FORWARD-only plan.  NULL = skip. */
int sctl_amd_lists_transpose_info(const sctl_amd_lists* plan, int64_t* pairs, int64_t* work_items, int64_t* target_ranges);
/* One-shot form (plan TRANSPOSE, evaluate, release), HOST arrays. */
int sctl_amd_eval_lists_transpose_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                       const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                       const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, int device);

/* ---- geometry gradients over the lists: the gradients of L = sum over the lists of <w_trg, A_l v_src> with respect to the target coordinates
 * (g_trg, Nt*3 values), the source coordinates (g_src, Ns*3) and the source normals (g_nrm, Ns*3; kernels with a normal), with the definitions
 * and signs of sctl_amd_eval_grad_*: d = x_t - x_s, a coincident pair contributes 0, a pair named by several lists counts once per list, every
 * output is ACCUMULATED into.  A NULL output is not computed: g_trg comes from ONE launch over the plan's FORWARD work list (the targets own the
 * sums), g_src and g_nrm from ONE launch over its TRANSPOSE work list (the sources own them); a side none of whose outputs is asked for is not
 * launched.  No atomics, no workspace: results are bit-identical from run to run.  All ten built-in kernels, fp64 and fp32 (the exact
 * vector-pipe pair), every digits.  Checks, in order: a null handle (SCTL_AMD_ERR_BAD_ARGUMENT); a plugin kernel (SCTL_AMD_ERR_UNKNOWN_KERNEL:
 * the gradient forms are built for the built-in kernels); g_trg with a plan made without SCTL_AMD_LISTS_FORWARD, g_src or g_nrm with one made
 * without SCTL_AMD_LISTS_TRANSPOSE, g_nrm for a kernel without a normal (SCTL_AMD_ERR_BAD_ARGUMENT); the context.  The counters grow by the
 * pairs of each launched side.  _host goes through the handle's stream, staging and device buffers; sources that ARE the targets (one array)
 * keep one device copy.  The one-shot form plans both directions.  Not built: several rows, plugins, the operator handle, several GPUs. */
int sctl_amd_lists_eval_grad_device(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, const void* w_trg,
                                    void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_lists_eval_grad_host(sctl_amd_lists* plan, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, const void* w_trg,
                                  void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes);
int sctl_amd_eval_lists_grad_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                  const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                  const void* v_src, const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx,
                                  int ctx_bytes, int device);

/* Several densities over the lists of one plan (the several-densities text above applies): density-major v_src[nd][Ns*SrcDim] and
 * v_trg[nd][Nt*TrgDim], every row ACCUMULATED into.  The plan does not depend on nd: one handle serves the single-density entries and any
 * nd.  nd < 0 is SCTL_AMD_ERR_BAD_ARGUMENT, nd == 0 does nothing, nd == 1 IS sctl_amd_lists_eval_* (bit-identical results); argument and
 * context errors come back before any device work, with the codes of sctl_amd_lists_eval_*; a plan without work items returns OK without a
 * device.  A call is ONE launch per pass: passes of the kernel's widest form (8, 4 or 2 densities, per kernel and precision: DESIGN.md
 * §4.6), then the narrowest form that holds the rest; a single density left over takes the single-density list kernel, and a plugin
 * kernel (no several-densities form) is evaluated one density at a time on the same stream.  Within a several-densities pass a row's
 * terms may be summed in another grouping than the single-density kernel's (rel-L2 ~1e-16 in fp64); results are bit-identical from run to
 * run.  fp32 runs the exact vector-pipe pair.  The counters grow by nd x pairs.  _host: coordinates and normals are staged once, the nd
 * density rows in one transfer; sources that ARE the targets (one array) keep one device copy. */
int sctl_amd_lists_eval_densities_device(sctl_amd_lists* plan, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                                         void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_lists_eval_densities_host(sctl_amd_lists* plan, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                                       void* v_trg, int digits, const void* ctx, int ctx_bytes);
/* One-shot form (plan, evaluate, release), HOST arrays. */
int sctl_amd_eval_lists_densities_host(int kernel, int real, int nd, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt,
                                       const int64_t* src_off, const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src,
                                       const void* n_src, const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device);

/* Several weight vectors through the transposed sum over the lists of one plan: row-major w_trg[nd][Nt*TrgDim] and g_src[nd][Ns*SrcDim],
 * every row ACCUMULATED into,
 *     g_src[m][s*SrcDim + k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w_trg[m][t*TrgDim + k1].
 * The plan is the transposed plan of sctl_amd_lists_create_directions and does not depend on nd.  Checks, in order: a null handle; the
 * context (SCTL_AMD_ERR_BAD_CONTEXT whatever nd is); nd < 0 (SCTL_AMD_ERR_BAD_ARGUMENT); a plan made without SCTL_AMD_LISTS_TRANSPOSE
 * (SCTL_AMD_ERR_BAD_ARGUMENT, as sctl_amd_lists_eval_transpose_*).  nd == 0 does nothing and touches nothing, nd == 1 IS
 * sctl_amd_lists_eval_transpose_* (same launch, same bits); a plan without transposed work items returns OK without a device and without
 * reading the arrays.  A call is ONE launch per pass, all on the same stream: passes of the kernel's widest form (8, 4 or 2 weight
 * vectors, per kernel and precision: DESIGN.md §4.15), then the narrowest form that holds the rest; a single row left over takes the
 * single-vector transposed list kernel, and a plugin kernel with pair_t (no several-vectors form) runs its rows one at a time on the same
 * stream.  Within a several-vectors pass a row's terms may be summed in another grouping than the single-vector kernel's (rel-L2 ~1e-16
 * in fp64); there are no atomics and no workspace: results are bit-identical from run to run.  fp32 runs the exact vector-pipe pair.  The
 * counters grow by nd x the plan's pairs.  _host: coordinates and normals are staged once, the nd weight rows go up in one transfer, the nd
 * result rows come back in one; sources that ARE the targets (one array) keep one device copy; the handle's stream, staging and device
 * buffers are reused and grown as needed. */
int sctl_amd_lists_eval_transpose_densities_device(sctl_amd_lists* plan, int nd, const void* r_trg, const void* r_src, const void* n_src,
                                                   const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream);
int sctl_amd_lists_eval_transpose_densities_host(sctl_amd_lists* plan, int nd, const void* r_trg, const void* r_src, const void* n_src,
                                                 const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes);
/* One-shot form (plan TRANSPOSE, evaluate, release), HOST arrays; nd < 0 comes back before the plan is made. */
int sctl_amd_eval_lists_transpose_densities_host(int kernel, int real, int nd, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt,
                                                 const int64_t* src_off, const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg,
                                                 const void* r_src, const void* n_src, const void* w_trg, void* g_src, int digits, const void* ctx,
                                                 int ctx_bytes, int device);

/* ---- accounting (the reference's Profile::IncrementCounter(FLOP, Ns*Nt*FLOPS()), generic-kernel.txx:188) ---- */
/* Process-wide counters, updated atomically by every eval / kernel_matrix call. */
void sctl_amd_counters(int64_t* pair_interactions, int64_t* sctl_flops);
void sctl_amd_reset_counters(void);
/* Frees the device scratch memory the library keeps per (device, stream) between calls (partial sums, the sort buffers
 * of the tile-centred path: up to ~1 GB per stream at 2^20 points) and the operators sctl_amd_eval_host_multi keeps between
 * calls (streams, device copies of the last coordinates, pinned staging; at most 8).  Waits for the devices.  Optional. */
void sctl_amd_trim(void);

/* Debugging switches (a bit mask; returns the previous mask).  SCTL_AMD_DEBUG_POISON_SCRATCH: every evaluation first fills the
 * device scratch it is about to use (partial sums, sort buffers) with NaN bit patterns, so that a read of scratch the call did not
 * write shows up as NaN in the result instead of as the previous call's numbers.  Costs one memset per call; off by default. */
#define SCTL_AMD_DEBUG_POISON_SCRATCH 1
int sctl_amd_set_debug(int flags);

/* Launch geometry chosen for a problem (for benchmarks and DESIGN.md; no side effects):
 * targets per lane, source splits, workgroups, and bytes of the partial-sum workspace.
 * Nt_whole: as in sctl_amd_eval_device_slab; 0 (or Nt) for a whole target set. */
int sctl_amd_eval_plan(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, int digits, int* trg_per_lane,
                       int* src_splits, int64_t* workgroups, int64_t* workspace_bytes);

/* Which device algorithm sctl_amd_eval_device/_host will use for a problem at the DEFAULT accuracy: 0 = the exact all-pairs kernel
 * (d = x_t - x_s per pair, as generic-kernel.txx:83), 1 = the tile-centred path (targets Morton-sorted on the device, far sources through
 * r2 = |x_t'|^2 + |x_s'|^2 - 2 x_t'.x_s', near sources exact): Laplace3D-FxU/-DxU (f64, f32), Laplace3D-FxdU and
 * Stokes3D-FxUP (f64), Stokes3D-FxU/-FSxU/-FxUP/-DxU/-FxT and Laplace3D-FxdU/-FDxUdU (f32, at the seed's accuracy only: sctl_amd_eval_pipe answers for a given `digits`).
 * Negative = error code.  Setting SCTL_AMD_CENTERED=0 in the environment forces 0. */
int sctl_amd_eval_path(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole);

/* Which execution units the far pairs of that problem run on at `digits` (for roofline labels; no side effects): 0 = the vector pipe, exact kernel;
 * 1 = the vector pipe, tile-centred path; 2 = tile-centred path with r2 (and the double layer's / the Stokeslet's dot product) as split-bf16 contractions on
 * the MATRIX cores (v_mfma_f32_32x32x16_bf16) and v_rsq_f32 + the accumulation on the vector pipe — fp32 Laplace3D-FxU/-DxU/-FxdU/-FDxUdU and five fp32 Stokes kernels at
 * the seed's accuracy (digits < 8); SCTL_AMD_MFMA_F32=0 in the environment keeps Laplace3D-FxU/-DxU on 1 and the others on 0.  Negative = error
 * code.  (The reference has one pipe, the host's SIMD units: vec.hpp.) */
int sctl_amd_eval_pipe(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, int digits);

#ifdef __cplusplus
}
#endif
#endif /* SCTL_AMD_H_ */
