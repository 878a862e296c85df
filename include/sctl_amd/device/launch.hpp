// Launch tables: one KernelEntry per micro-kernel, filled in its own translation unit (inst_*.hip) so the
// ~200 kernel instantiations compile in parallel.  capi.hip only sees function pointers.
#pragma once
#include "eval_kernel.hpp"
#include "eval_transpose_kernel.hpp"
#include "eval_grad_kernel.hpp"
#include "lists_kernel.hpp"
#include "lists_transpose_kernel.hpp"

namespace sctl_amd {

constexpr int kNumT = 3;                       // targets per lane: 1, 2, 4
constexpr int kTvalues[kNumT] = {1, 2, 4};
constexpr int kNumMode = 3;                    // rsqrt refinement: seed, Newton, Halley (ukernels.hpp)
constexpr int kNumTT = 2;                      // sources per lane of the transposed evaluator: 1, 2
constexpr int kTTvalues[kNumTT] = {1, 2};

template <class R> using EvalLaunch = void (*)(const EvalArgs<R>&, dim3 grid, hipStream_t);
template <class R> using EvalTLaunch = void (*)(const EvalTArgs<R>&, dim3 grid, hipStream_t);
template <class R> using EvalGLaunch = void (*)(const EvalGArgs<R>&, dim3 grid, hipStream_t);
template <class R> using MatrixBatchLaunch = void (*)(const MatTile* tiles, int64_t ntiles, const R* xt, const R* xs, const R* xn, R* M, R scale, const KerCtx&, hipStream_t);
template <class R> using ListsLaunch = void (*)(const ListArgs<R>&, int64_t nblocks, hipStream_t);
template <class R> using ListsTLaunch = void (*)(const ListTArgs<R>&, int64_t nblocks, hipStream_t);
template <class R> using MatrixLaunch = void (*)(int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, R* M, R scale, const KerCtx&, dim3 grid, hipStream_t);

struct KernelEntry {
  const char* name;
  int id, k0, k1, nd, flops, nrec, ctx_bytes;
  double scale;
  double acc_factor[kNumMode];   // pair() of mode m accumulates acc_factor[m] x the kernel value: the launch scale is scale / acc_factor[m]
  EvalLaunch<double> eval_f64[kNumMode][kNumT];
  EvalLaunch<float> eval_f32[kNumMode][kNumT];     // modes 0 and 1 only (mode 2 aliases mode 1)
  MatrixLaunch<double> matrix_f64[kNumMode];
  MatrixLaunch<float> matrix_f32[kNumMode];
  MatrixBatchLaunch<double> matrix_batch_f64[kNumMode];
  MatrixBatchLaunch<float> matrix_batch_f32[kNumMode];
  ListsLaunch<double> lists_f64[kNumMode];          // lists_kernel.hpp
  ListsLaunch<float> lists_f32[kNumMode];
  // the transposed evaluator (eval_transpose_kernel.hpp): all null, and nrec_t 0, for a functor without pair_t
  int nrec_t;
  EvalTLaunch<double> eval_t_f64[kNumMode][kNumTT];
  EvalTLaunch<float> eval_t_f32[kNumMode][kNumTT];  // modes 0 and 1 only (mode 2 aliases mode 1)
  // the gradient evaluator (eval_grad_kernel.hpp), side 0 target-owned, side 1 source-owned: all null, and grad_t 0, for a functor without pair_g
  int grad_t[2];                                    // owners per lane of each side (GradOwnersOf)
  double grad_factor[kNumMode];                     // pair_g() of mode m accumulates grad_factor[m] x the derivative (GradFactorOf)
  EvalGLaunch<double> eval_g_f64[kNumMode][2];
  EvalGLaunch<float> eval_g_f32[kNumMode][2];       // modes 0 and 1 only (mode 2 aliases mode 1)
  // the transposed list evaluator (lists_transpose_kernel.hpp): null for a functor without pair_t.  At the END of the entry: registration refuses a
  // plugin built against a shorter entry by entry_bytes, so SCTL_AMD_DEVICE_ABI stays as it is
  ListsTLaunch<double> lists_t_f64[kNumMode];
  ListsTLaunch<float> lists_t_f32[kNumMode];        // modes 0 and 1 only (mode 2 aliases mode 1)
};

// Owners per lane of the gradient evaluator, per kernel and side.  One everywhere: a gradient pair is two to four times the forward pair's arithmetic, so
// the LDS reads a second owner would share are a small part of it, and every form then keeps ScratchSize 0 and at least two waves per SIMD with room
// to spare (two owners per lane have not been timed).
template <class Ker, int SIDE> struct GradOwnersOf { static constexpr int value = 1; };

template <class Ker, class R, int MODE, int T> void launch_eval(const EvalArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_kernel<Ker, R, MODE, T>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, class R, int MODE, int T> void launch_eval_t(const EvalTArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_transpose_kernel<Ker, R, MODE, T>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, class R, int MODE, int SIDE> void launch_eval_g(const EvalGArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_grad_kernel<Ker, R, MODE, SIDE, GradOwnersOf<Ker, SIDE>::value>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, class R, int MODE> void launch_matrix(int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, R* M, R scale,
                                                           const KerCtx& ctx, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((matrix_kernel<Ker, R, MODE>), grid, dim3(kBlock), 0, st, Nt, Ns, xt, xs, xn, M, scale, ctx);
}

template <class Ker, class R, int MODE> void launch_matrix_batch(const MatTile* tiles, int64_t ntiles, const R* xt, const R* xs, const R* xn, R* M, R scale,
                                                                 const KerCtx& ctx, hipStream_t st) {
  hipLaunchKernelGGL((matrix_batch_kernel<Ker, R, MODE>), dim3((unsigned)ntiles), dim3(kBlock), 0, st, tiles, xt, xs, xn, M, scale, ctx);
}

template <class Ker, class R, int MODE> void launch_lists(const ListArgs<R>& a, int64_t nblocks, hipStream_t st) {
  hipLaunchKernelGGL((lists_kernel<Ker, R, MODE>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}

template <class Ker, class R, int MODE> void launch_lists_t(const ListTArgs<R>& a, int64_t nblocks, hipStream_t st) {
  hipLaunchKernelGGL((lists_transpose_kernel<Ker, R, MODE>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}

template <class Ker> KernelEntry make_entry(int ctx_bytes) {
  KernelEntry e{};
  e.name = Ker::NAME; e.id = Ker::ID; e.k0 = Ker::K0; e.k1 = Ker::K1; e.nd = Ker::ND; e.flops = Ker::FLOPS; e.nrec = Ker::NREC;
  e.ctx_bytes = ctx_bytes; e.scale = Ker::scale();
  for (int m = 0; m < kNumMode; m++) e.acc_factor[m] = Ker::acc_factor(m);
#define SCTL_AMD_ROW(R, arr, M, MM) \
  arr[M][0] = launch_eval<Ker, R, MM, 1>; arr[M][1] = launch_eval<Ker, R, MM, 2>; arr[M][2] = launch_eval<Ker, R, MM, 4>;
  SCTL_AMD_ROW(double, e.eval_f64, 0, 0) SCTL_AMD_ROW(double, e.eval_f64, 1, 1) SCTL_AMD_ROW(double, e.eval_f64, 2, 2)
  SCTL_AMD_ROW(float, e.eval_f32, 0, 0) SCTL_AMD_ROW(float, e.eval_f32, 1, 1) SCTL_AMD_ROW(float, e.eval_f32, 2, 1)
#undef SCTL_AMD_ROW
  e.matrix_f64[0] = launch_matrix<Ker, double, 0>; e.matrix_f64[1] = launch_matrix<Ker, double, 1>; e.matrix_f64[2] = launch_matrix<Ker, double, 2>;
  e.matrix_f32[0] = launch_matrix<Ker, float, 0>; e.matrix_f32[1] = launch_matrix<Ker, float, 1>; e.matrix_f32[2] = launch_matrix<Ker, float, 1>;
  e.matrix_batch_f64[0] = launch_matrix_batch<Ker, double, 0>; e.matrix_batch_f64[1] = launch_matrix_batch<Ker, double, 1>;
  e.matrix_batch_f64[2] = launch_matrix_batch<Ker, double, 2>;
  e.matrix_batch_f32[0] = launch_matrix_batch<Ker, float, 0>; e.matrix_batch_f32[1] = launch_matrix_batch<Ker, float, 1>;
  e.matrix_batch_f32[2] = launch_matrix_batch<Ker, float, 1>;
  e.lists_f64[0] = launch_lists<Ker, double, 0>; e.lists_f64[1] = launch_lists<Ker, double, 1>; e.lists_f64[2] = launch_lists<Ker, double, 2>;
  e.lists_f32[0] = launch_lists<Ker, float, 0>; e.lists_f32[1] = launch_lists<Ker, float, 1>; e.lists_f32[2] = launch_lists<Ker, float, 1>;
  if constexpr (HasPairT<Ker>::value) {
    e.nrec_t = Ker::NREC_T;
#define SCTL_AMD_ROW_T(R, arr, M, MM) arr[M][0] = launch_eval_t<Ker, R, MM, 1>; arr[M][1] = launch_eval_t<Ker, R, MM, 2>;
    SCTL_AMD_ROW_T(double, e.eval_t_f64, 0, 0) SCTL_AMD_ROW_T(double, e.eval_t_f64, 1, 1) SCTL_AMD_ROW_T(double, e.eval_t_f64, 2, 2)
    SCTL_AMD_ROW_T(float, e.eval_t_f32, 0, 0) SCTL_AMD_ROW_T(float, e.eval_t_f32, 1, 1) SCTL_AMD_ROW_T(float, e.eval_t_f32, 2, 1)
#undef SCTL_AMD_ROW_T
    e.lists_t_f64[0] = launch_lists_t<Ker, double, 0>; e.lists_t_f64[1] = launch_lists_t<Ker, double, 1>; e.lists_t_f64[2] = launch_lists_t<Ker, double, 2>;
    e.lists_t_f32[0] = launch_lists_t<Ker, float, 0>; e.lists_t_f32[1] = launch_lists_t<Ker, float, 1>; e.lists_t_f32[2] = launch_lists_t<Ker, float, 1>;
  }
  if constexpr (HasPairG<Ker>::value) {
    e.grad_t[0] = GradOwnersOf<Ker, 0>::value; e.grad_t[1] = GradOwnersOf<Ker, 1>::value;
    for (int m = 0; m < kNumMode; m++) e.grad_factor[m] = GradFactorOf<Ker>::value(m);
#define SCTL_AMD_ROW_G(R, arr, M, MM) arr[M][0] = launch_eval_g<Ker, R, MM, 0>; arr[M][1] = launch_eval_g<Ker, R, MM, 1>;
    SCTL_AMD_ROW_G(double, e.eval_g_f64, 0, 0) SCTL_AMD_ROW_G(double, e.eval_g_f64, 1, 1) SCTL_AMD_ROW_G(double, e.eval_g_f64, 2, 2)
    SCTL_AMD_ROW_G(float, e.eval_g_f32, 0, 0) SCTL_AMD_ROW_G(float, e.eval_g_f32, 1, 1) SCTL_AMD_ROW_G(float, e.eval_g_f32, 2, 1)
#undef SCTL_AMD_ROW_G
  }
  return e;
}

// The transposed launchers of the ten built-in functors are compiled in units of their own (inst_t_*.hip): make_entry, in inst_*.hip, only takes
// their addresses.  A plugin's functor is instantiated where its make_entry is.
#define SCTL_AMD_EVAL_T_INSTANCES(PREFIX, Ker)                                                              \
  PREFIX template void launch_eval_t<Ker, double, 0, 1>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, double, 0, 2>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, double, 1, 1>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, double, 1, 2>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, double, 2, 1>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, double, 2, 2>(const EvalTArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_t<Ker, float, 0, 1>(const EvalTArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_t<Ker, float, 0, 2>(const EvalTArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_t<Ker, float, 1, 1>(const EvalTArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_t<Ker, float, 1, 2>(const EvalTArgs<float>&, dim3, hipStream_t);
SCTL_AMD_EVAL_T_INSTANCES(extern, Laplace3D_FxU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Laplace3D_DxU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Laplace3D_FxdU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Stokes3D_FxU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Stokes3D_DxU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Stokes3D_FxT)
SCTL_AMD_EVAL_T_INSTANCES(extern, Stokes3D_FSxU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Stokes3D_FxUP)
SCTL_AMD_EVAL_T_INSTANCES(extern, Laplace3D_FDxUdU)
SCTL_AMD_EVAL_T_INSTANCES(extern, Helmholtz3D_FxU)

// ... and the gradient launchers in inst_g_*.hip
#define SCTL_AMD_EVAL_G_INSTANCES(PREFIX, Ker)                                                              \
  PREFIX template void launch_eval_g<Ker, double, 0, 0>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, double, 0, 1>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, double, 1, 0>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, double, 1, 1>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, double, 2, 0>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, double, 2, 1>(const EvalGArgs<double>&, dim3, hipStream_t);       \
  PREFIX template void launch_eval_g<Ker, float, 0, 0>(const EvalGArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_g<Ker, float, 0, 1>(const EvalGArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_g<Ker, float, 1, 0>(const EvalGArgs<float>&, dim3, hipStream_t);         \
  PREFIX template void launch_eval_g<Ker, float, 1, 1>(const EvalGArgs<float>&, dim3, hipStream_t);
SCTL_AMD_EVAL_G_INSTANCES(extern, Laplace3D_FxU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Laplace3D_DxU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Laplace3D_FxdU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Stokes3D_FxU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Stokes3D_DxU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Stokes3D_FxT)
SCTL_AMD_EVAL_G_INSTANCES(extern, Stokes3D_FSxU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Stokes3D_FxUP)
SCTL_AMD_EVAL_G_INSTANCES(extern, Laplace3D_FDxUdU)
SCTL_AMD_EVAL_G_INSTANCES(extern, Helmholtz3D_FxU)

// ... the transposed list launchers in inst_lt_*.hip
#define SCTL_AMD_LISTS_T_INSTANCES(PREFIX, Ker)                                                             \
  PREFIX template void launch_lists_t<Ker, double, 0>(const ListTArgs<double>&, int64_t, hipStream_t);      \
  PREFIX template void launch_lists_t<Ker, double, 1>(const ListTArgs<double>&, int64_t, hipStream_t);      \
  PREFIX template void launch_lists_t<Ker, double, 2>(const ListTArgs<double>&, int64_t, hipStream_t);      \
  PREFIX template void launch_lists_t<Ker, float, 0>(const ListTArgs<float>&, int64_t, hipStream_t);        \
  PREFIX template void launch_lists_t<Ker, float, 1>(const ListTArgs<float>&, int64_t, hipStream_t);
SCTL_AMD_LISTS_T_INSTANCES(extern, Laplace3D_FxU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Laplace3D_DxU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Laplace3D_FxdU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Stokes3D_FxU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Stokes3D_DxU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Stokes3D_FxT)
SCTL_AMD_LISTS_T_INSTANCES(extern, Stokes3D_FSxU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Stokes3D_FxUP)
SCTL_AMD_LISTS_T_INSTANCES(extern, Laplace3D_FDxUdU)
SCTL_AMD_LISTS_T_INSTANCES(extern, Helmholtz3D_FxU)

// defined in inst_*.hip
const KernelEntry& entry_Laplace3D_FxU();
const KernelEntry& entry_Laplace3D_DxU();
const KernelEntry& entry_Laplace3D_FxdU();
const KernelEntry& entry_Stokes3D_FxU();
const KernelEntry& entry_Stokes3D_DxU();
const KernelEntry& entry_Stokes3D_FxT();
const KernelEntry& entry_Stokes3D_FSxU();
const KernelEntry& entry_Stokes3D_FxUP();
const KernelEntry& entry_Laplace3D_FDxUdU();
const KernelEntry& entry_Helmholtz3D_FxU();

}  // namespace sctl_amd
