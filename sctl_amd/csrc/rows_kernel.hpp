// Several rows through the all-pairs kernel sum in a single pass, both directions from ONE body:
//   forward     (eval_multi_kernel)            v[m][t*K1 + k1] += scale * sum_s sum_k0 U(x_t - x_s, n_s)[k0][k1] * f[m][s*K0 + k0]
//   transposed  (eval_multi_transpose_kernel)  g[m][s*K0 + k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t*K1 + k1]
// for m = 0 .. nd-1.  These are the all-pairs evaluators of include/sctl_amd/device/eval_kernel.hpp and eval_transpose_kernel.hpp with M rows (densities, weight
// vectors) per streamed record (ukernels.hpp: NREC_M / pack_m / pair_m and NREC_TM / pack_tm / pair_tm).  Everything a pair costs that does not depend on the row
// (distance, reciprocal square root and its refinement, d.n, Helmholtz's e^{ikr}) is computed once per pair and contracted with each of the M rows.
//
// Same scheme as the single-row kernels: 256-lane workgroups whose lanes OWN T points each (a target forward; a source with its normal transposed), LDS tiles of
// the STREAMED points read by wave broadcast, splits of the streamed range with the XCD-owned mapping, partial sums reduced in a fixed order (no atomics), unmasked
// speculation with per-tile repair.  What differs from the single-row kernels:
//   * accumulators are T x M x KOUT per lane (and as many per-tile sums), so T is fixed per (direction, kernel, M) in the launch tables (multi_*.hip, tmulti_*.hip);
//   * rows are row-major: row m of streamed point q is in[m * in_stride + q * KIN + k], its result for owner o is out[m * out_stride + o * KOUT + k];
//   * the last pass of a call may use fewer rows than the form's M (nact): the others are packed as 0 and never stored;
//   * partial sums are [M][splits][n_own * KOUT], so that reduce_splits_kernel adds one row's splits as it adds a single-row call's.
// fp32 runs this exact vector-pipe pair at every accuracy (there is no matrix-core form): full fp32 accuracy, also at digits <= 7.
//
// The two directions differ only in the policy `Dir` (RowsFwd, RowsTrans of rows_dir.hpp): which of K0 / K1 is the output width, the record, who carries the normal
// and the sign of d.  Everything else — the body, its arguments, the launch table — exists once.
#pragma once
#include <sctl_amd/device/launch.hpp>
#include "rows_dir.hpp"

namespace sctl_amd {

template <class R> struct RowsArgs {
  int64_t n_own, n_str;   // owners of this launch, streamed points
  const R* x_own;         // [n_own*3], this launch's owners
  const R* x_str;         // [n_str*3]
  const R* nrm;           // [sources*ND] or null: the normals of the sources, which are streamed forward and (this launch's) owners transposed
  const R* in;            // row-major: row m at in + m * in_stride
  int64_t in_stride;
  R* out;                 // row-major: row m at out + m * out_stride (accumulated into when gridDim.y == 1)
  int64_t out_stride;
  R* partial;             // [M][gridDim.y][n_own*KOUT] unscaled partial sums when gridDim.y > 1
  int64_t chunk;          // streamed points per split, a multiple of kTile
  int nact;               // rows in use, 1 <= nact <= M
  R scale;
  KerCtx ctx;
};

template <class Dir, class Ker, class R, int MODE, int T, int M> __device__ __forceinline__ void rows_body(const RowsArgs<R> a) {
  constexpr int KIN = Dir::template KIN<Ker>, KOUT = Dir::template KOUT<Ker>, ND = Ker::ND, NREC = Dir::template NREC<Ker, M>;
  constexpr int OWN_N = Dir::template OWN_N<Ker>, STR_N = Dir::template STR_N<Ker>, NN = OWN_N ? OWN_N : 1;
  using V = typename VecOf<R>::type;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  __shared__ V tile[kTile * NV];

  const int tid = threadIdx.x;
  unsigned tile_x = blockIdx.x, split_y = blockIdx.y;   // the XCD-owned split mapping of eval_kernel
  if (gridDim.y >= 8 && (gridDim.y & 7) == 0) {
    const unsigned b = blockIdx.x + gridDim.x * blockIdx.y, i = b >> 3;
    tile_x = i % gridDim.x;
    split_y = (b & 7) * (gridDim.y >> 3) + i / gridDim.x;
  }
  const int64_t obase = (int64_t)tile_x * (kBlock * T);
  using KC = typename Ker::template Consts<R>;
  constexpr int SCRATCH = AllPairsScratch<KC>::value;
  __shared__ double kscratch[SCRATCH > 0 ? SCRATCH : 1];
  const KC K = make_consts<KC>(kscratch, SCRATCH, a.ctx, MODE);

  R xo[T][3], no[T][NN], acc[T][M][KOUT];   // (no: a dummy where the owner holds no normal; the forward pair ignores it)
#pragma unroll
  for (int j = 0; j < T; j++) {
    int64_t o = obase + j * kBlock + tid;
    if (o >= a.n_own) o = a.n_own - 1;   // tail lanes recompute the last owner; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) xo[j][k] = a.x_own[o * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) no[j][k] = OWN_N ? a.nrm[o * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < KOUT; k++) acc[j][m][k] = 0;
  }

  const int64_t q_begin = (int64_t)split_y * a.chunk;
  const int64_t q_end = (q_begin + a.chunk < a.n_str) ? q_begin + a.chunk : a.n_str;
  const int64_t len = (q_end > q_begin) ? q_end - q_begin : 0;   // (a split past the streamed points, which rounds the splits up to eights, has none)
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  for (int it = 0; it < ntile; it++) {
    const int nq = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (tid < nq) {
      const int64_t q = q_begin + (int64_t)it * kTile + tid;
      R px[3], pn[3] = {0, 0, 0}, pr[M][KIN];
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.x_str[q * 3 + k];
#pragma unroll
      for (int k = 0; k < STR_N; k++) pn[k] = a.nrm[q * STR_N + k];
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < KIN; k++) pr[m][k] = (m < a.nact) ? a.in[m * a.in_stride + q * KIN + k] : R(0);
      R rec[NRECP] = {};
      Dir::template pack<Ker, R, M>(rec, px, pn, pr);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V w;
#pragma unroll
        for (int e = 0; e < VN; e++) w[e] = rec[v * VN + e];
        tile[tid * NV + v] = w;
      }
    }
    __syncthreads();

    R tacc[T][M][KOUT];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < KOUT; k++) tacc[j][m][k] = 0;
      auto one_point = [&](int s) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V w = tile[s * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = w[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) Dir::template pair<Ker, R, MODE, MASKED, M, VARIANT>(tacc[j], xo[j], no[j], rec, a.ctx, K);
      };
      if (nq == kTile) {
#pragma unroll UnrollOf<T, M * KOUT>::value
        for (int s = 0; s < kTile; s++) one_point(s);
      } else {
        for (int s = 0; s < nq; s++) one_point(s);
      }
    };
    auto run_tile = [&](auto masked_tag) {
      if constexpr (KC::HAS_VARIANT) {
        const int v = (int)K.variant(a.ctx);
        if constexpr (NumVariants<KC>::value > 2) {
          if (v == 3) run_tile_v(masked_tag, std::integral_constant<int, 3>());
          else if (v == 2) run_tile_v(masked_tag, std::integral_constant<int, 2>());
          else if (v == 1) run_tile_v(masked_tag, std::integral_constant<int, 1>());
          else run_tile_v(masked_tag, std::integral_constant<int, 0>());
        } else {
          if (v) run_tile_v(masked_tag, std::integral_constant<int, 1>());
          else run_tile_v(masked_tag, std::integral_constant<int, 0>());
        }
      } else {
        run_tile_v(masked_tag, std::integral_constant<int, 0>());
      }
    };
    bool repaired = true;
    if (!always_masked) {
      run_tile(std::false_type());
      bool bad = K.tile_bad(a.ctx);
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < KOUT; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < KOUT; k++) acc[j][m][k] += tacc[j][m][k];
  }

#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t o = obase + j * kBlock + tid;
    if (o >= a.n_own) continue;
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      Dir::template finish<Ker, R, MODE>(acc[j][m]);
      if (gridDim.y == 1) {
        R* v = a.out + m * a.out_stride + o * KOUT;
#pragma unroll
        for (int k = 0; k < KOUT; k++) v[k] += acc[j][m][k] * a.scale;
      } else {
        R* p = a.partial + (((int64_t)m * gridDim.y + split_y) * a.n_own + o) * KOUT;
#pragma unroll
        for (int k = 0; k < KOUT; k++) p[k] = acc[j][m][k];
      }
    }
  }
}

template <class Ker, class R, int MODE, int T, int M> __global__ void __launch_bounds__(kBlock, 2) eval_multi_kernel(const RowsArgs<R> a) {
  rows_body<RowsFwd, Ker, R, MODE, T, M>(a);
}
template <class Ker, class R, int MODE, int T, int M> __global__ void __launch_bounds__(kBlock, 2) eval_multi_transpose_kernel(const RowsArgs<R> a) {
  rows_body<RowsTrans, Ker, R, MODE, T, M>(a);
}

// ---- launch table: one per direction and built-in kernel (multi_<Kernel>.hip, tmulti_<Kernel>.hip), none for plugin kernels ------------------------------
constexpr int kNumRowsM = 3;                         // forms of 2, 4 and 8 rows
constexpr int kRowsM[kNumRowsM] = {2, 4, 8};
template <class R> using RowsLaunch = void (*)(const RowsArgs<R>&, dim3 grid, hipStream_t);
template <class Dir> struct RowsEntry {
  int m_max;                                         // widest form: 4 or 8
  int t[kNumRowsM];                                  // owners per lane of each form (0: no such form)
  RowsLaunch<double> f64[kNumMode][kNumRowsM];
  RowsLaunch<float> f32[kNumMode][kNumRowsM];        // modes 0 and 1 (mode 2 aliases 1)
};
using MultiEntry = RowsEntry<RowsFwd>;
using MultiTEntry = RowsEntry<RowsTrans>;

template <class Dir, class Ker, class R, int MODE, int T, int M> void launch_rows(const RowsArgs<R>& a, dim3 grid, hipStream_t st) {
  if constexpr (std::is_same<Dir, RowsFwd>::value) hipLaunchKernelGGL((eval_multi_kernel<Ker, R, MODE, T, M>), grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL((eval_multi_transpose_kernel<Ker, R, MODE, T, M>), grid, dim3(kBlock), 0, st, a);
}
template <class Dir, class Ker, int T, int M> void fill_rows(RowsEntry<Dir>& e, int i) {
  e.t[i] = T;
  e.f64[0][i] = launch_rows<Dir, Ker, double, 0, T, M>; e.f64[1][i] = launch_rows<Dir, Ker, double, 1, T, M>; e.f64[2][i] = launch_rows<Dir, Ker, double, 2, T, M>;
  e.f32[0][i] = launch_rows<Dir, Ker, float, 0, T, M>; e.f32[1][i] = launch_rows<Dir, Ker, float, 1, T, M>; e.f32[2][i] = e.f32[1][i];
}
// T2, T4, T8: owners per lane of the forms of 2, 4 and 8 rows; T8 = 0: the kernel's widest form has 4
template <class Dir, class Ker, int T2, int T4, int T8> RowsEntry<Dir> make_rows_entry() {
  RowsEntry<Dir> e{};
  fill_rows<Dir, Ker, T2, 2>(e, 0);
  fill_rows<Dir, Ker, T4, 4>(e, 1);
  if constexpr (T8 > 0) fill_rows<Dir, Ker, T8, 8>(e, 2);
  e.m_max = T8 > 0 ? 8 : 4;
  return e;
}

// defined in multi_*.hip
const MultiEntry& multi_Laplace3D_FxU();
const MultiEntry& multi_Laplace3D_DxU();
const MultiEntry& multi_Laplace3D_FxdU();
const MultiEntry& multi_Stokes3D_FxU();
const MultiEntry& multi_Stokes3D_DxU();
const MultiEntry& multi_Stokes3D_FxT();
const MultiEntry& multi_Stokes3D_FSxU();
const MultiEntry& multi_Stokes3D_FxUP();
const MultiEntry& multi_Laplace3D_FDxUdU();
const MultiEntry& multi_Helmholtz3D_FxU();
// defined in tmulti_*.hip
const MultiTEntry& multi_t_Laplace3D_FxU();
const MultiTEntry& multi_t_Laplace3D_DxU();
const MultiTEntry& multi_t_Laplace3D_FxdU();
const MultiTEntry& multi_t_Stokes3D_FxU();
const MultiTEntry& multi_t_Stokes3D_DxU();
const MultiTEntry& multi_t_Stokes3D_FxT();
const MultiTEntry& multi_t_Stokes3D_FSxU();
const MultiTEntry& multi_t_Stokes3D_FxUP();
const MultiTEntry& multi_t_Laplace3D_FDxUdU();
const MultiTEntry& multi_t_Helmholtz3D_FxU();

}  // namespace sctl_amd
