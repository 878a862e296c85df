// Several weight vectors through the transposed sum in a single pass: the transposed all-pairs evaluator of include/sctl_amd/device/eval_transpose_kernel.hpp
// with M weight vectors per streamed target record (ukernels.hpp: NREC_TM / pack_tm / pair_tm),
//     g[m][s*K0 + k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t*K1 + k1],   m = 0 .. nd-1.
// Everything a pair costs that does not depend on the weights (distance, reciprocal square root and its refinement, d.n, Helmholtz's e^{ikr}) is
// computed once per pair and contracted with each of the M weight vectors.
//
// Same scheme as eval_transpose_kernel: 256-lane workgroups whose lanes OWN T sources each (coordinates, normal, sums), LDS target tiles read by wave
// broadcast, target splits with the XCD-owned mapping, partial sums reduced in a fixed order (no atomics), unmasked speculation with per-tile repair.
// What differs, as multi_kernel.hpp differs from eval_kernel.hpp:
//   * accumulators are T x M x K0 per lane (and as many per-tile sums), so T is fixed per (kernel, M) in the launch table below;
//   * rows are density-major: weights m of target t are w[m * w_stride + t * K1 + k], their result g_src[m * g_stride + s * K0 + k];
//   * the last pass of a call may use fewer rows than the form's M (nact): the others are packed as 0 and never stored;
//   * partial sums are [M][splits][Ns * K0], so that reduce_splits_kernel adds one row's splits as it adds a single call's.
// fp32 runs this exact vector-pipe pair at every accuracy, as the single transposed kernel does.
#pragma once
#include <sctl_amd/device/eval_transpose_kernel.hpp>
#include <sctl_amd/device/launch.hpp>

namespace sctl_amd {

template <class R> struct MultiTArgs {
  int64_t Nt, Ns;   // targets, sources (owners) of this launch
  const R* xt;      // [Nt*3]   streamed
  const R* xs;      // [Ns*3], this launch's owners
  const R* xn;      // [Ns*ND] or null
  const R* w;       // row-major: row m at w + m * w_stride
  int64_t w_stride;
  R* g_src;         // row-major: row m at g_src + m * g_stride (accumulated into when gridDim.y == 1)
  int64_t g_stride;
  R* partial;       // [M][gridDim.y][Ns*K0] unscaled partial sums when gridDim.y > 1
  int64_t chunk;    // targets per split, a multiple of kTile
  int nact;         // rows in use, 1 <= nact <= M
  R scale;
  KerCtx ctx;
};

template <class Ker, class R, int MODE, int T, int M>
__global__ void __launch_bounds__(kBlock, 2) eval_multi_transpose_kernel(const MultiTArgs<R> a) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_TM<M>, NN = ND ? 3 : 1;
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
  const int64_t sbase = (int64_t)tile_x * (kBlock * T);
  using KC = typename Ker::template Consts<R>;
  constexpr int SCRATCH = AllPairsScratch<KC>::value;
  __shared__ double kscratch[SCRATCH > 0 ? SCRATCH : 1];
  const KC K = make_consts<KC>(kscratch, SCRATCH, a.ctx, MODE);

  R xs[T][3], xn[T][NN], acc[T][M][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int64_t s = sbase + j * kBlock + tid;
    if (s >= a.Ns) s = a.Ns - 1;   // tail lanes recompute the last source; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.xn[s * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][m][k] = 0;
  }

  const int64_t t_begin = (int64_t)split_y * a.chunk;
  const int64_t t_end = (t_begin + a.chunk < a.Nt) ? t_begin + a.chunk : a.Nt;
  const int64_t len = (t_end > t_begin) ? t_end - t_begin : 0;   // (a split past the targets, which rounds the splits up to eights, has none)
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  for (int it = 0; it < ntile; it++) {
    const int nt = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (tid < nt) {
      const int64_t t = t_begin + (int64_t)it * kTile + tid;
      R px[3], pw[M][K1];
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.xt[t * 3 + k];
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) pw[m][k] = (m < a.nact) ? a.w[m * a.w_stride + t * K1 + k] : R(0);
      R rec[NRECP] = {};
      Ker::template pack_tm<R, M>(rec, px, pw);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V q;
#pragma unroll
        for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
        tile[tid * NV + v] = q;
      }
    }
    __syncthreads();

    R tacc[T][M][K0];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < K0; k++) tacc[j][m][k] = 0;
      auto one_target = [&](int t) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V q = tile[t * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = q[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
          const R d[3] = {rec[0] - xs[j][0], rec[1] - xs[j][1], rec[2] - xs[j][2]};
          if constexpr (KC::HAS_VARIANT) Ker::template pair_tm<R, MODE, MASKED, M, VARIANT>(tacc[j], d, xn[j], rec, a.ctx, K);
          else Ker::template pair_tm<R, MODE, MASKED, M>(tacc[j], d, xn[j], rec, a.ctx, K);
        }
      };
      if (nt == kTile) {
#pragma unroll UnrollOf<T, M * K0>::value
        for (int t = 0; t < kTile; t++) one_target(t);
      } else {
        for (int t = 0; t < nt; t++) one_target(t);
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
          for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) acc[j][m][k] += tacc[j][m][k];
  }

#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t s = sbase + j * kBlock + tid;
    if (s >= a.Ns) continue;
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_t_acc<Ker, R, MODE>(acc[j][m]);
      if (gridDim.y == 1) {
        R* g = a.g_src + m * a.g_stride + s * K0;
#pragma unroll
        for (int k = 0; k < K0; k++) g[k] += acc[j][m][k] * a.scale;
      } else {
        R* p = a.partial + (((int64_t)m * gridDim.y + split_y) * a.Ns + s) * K0;
#pragma unroll
        for (int k = 0; k < K0; k++) p[k] = acc[j][m][k];
      }
    }
  }
}

// ---- launch table: one per built-in kernel (tmulti_<Kernel>.hip), none for plugin kernels ------------------------------------------------
constexpr int kNumMultiTM = 3;                       // forms of 2, 4 and 8 weight vectors
constexpr int kMultiTM[kNumMultiTM] = {2, 4, 8};
template <class R> using MultiTLaunch = void (*)(const MultiTArgs<R>&, dim3 grid, hipStream_t);
struct MultiTEntry {
  int m_max;                                         // widest form: 4 or 8
  int t[kNumMultiTM];                                // sources per lane of each form (0: no such form)
  MultiTLaunch<double> f64[kNumMode][kNumMultiTM];
  MultiTLaunch<float> f32[kNumMode][kNumMultiTM];    // modes 0 and 1 (mode 2 aliases 1)
};

template <class Ker, class R, int MODE, int T, int M> void launch_multi_t(const MultiTArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_multi_transpose_kernel<Ker, R, MODE, T, M>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, int T, int M> void fill_multi_t(MultiTEntry& e, int i) {
  e.t[i] = T;
  e.f64[0][i] = launch_multi_t<Ker, double, 0, T, M>; e.f64[1][i] = launch_multi_t<Ker, double, 1, T, M>; e.f64[2][i] = launch_multi_t<Ker, double, 2, T, M>;
  e.f32[0][i] = launch_multi_t<Ker, float, 0, T, M>; e.f32[1][i] = launch_multi_t<Ker, float, 1, T, M>; e.f32[2][i] = e.f32[1][i];
}
// T2, T4, T8: sources per lane of the forms of 2, 4 and 8 weight vectors; T8 = 0: the kernel's widest form has 4
template <class Ker, int T2, int T4, int T8> MultiTEntry make_multi_t_entry() {
  MultiTEntry e{};
  fill_multi_t<Ker, T2, 2>(e, 0);
  fill_multi_t<Ker, T4, 4>(e, 1);
  if constexpr (T8 > 0) fill_multi_t<Ker, T8, 8>(e, 2);
  e.m_max = T8 > 0 ? 8 : 4;
  return e;
}

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
