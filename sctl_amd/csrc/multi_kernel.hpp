// Many densities against one geometry in a single pass: the all-pairs evaluator of include/sctl_amd/device/eval_kernel.hpp with M densities
// per source record (ukernels.hpp: NREC_M / pack_m / pair_m).  Everything a pair costs that does not depend on the density (distance,
// reciprocal square root and its refinement, Helmholtz's e^{ikr}) is computed once per pair and contracted with each of the M densities.
//
// Same scheme as eval_kernel: 256-lane workgroups with T targets per lane, LDS source tiles read by wave broadcast, source splits with the
// XCD-owned mapping, partial sums reduced in a fixed order (no atomics), unmasked speculation with per-tile repair.  What differs:
//   * accumulators are T x M x K1 per lane (and as many per-tile sums), so T is fixed per (kernel, M) in the launch table below;
//   * densities are density-major: density m of source s is f[m * f_stride + s * K0 + k], its result v_trg[m * v_stride + t * K1 + k];
//   * the last pass of a call may use fewer densities than the form's M (nact): the others are packed as 0 and never stored;
//   * partial sums are [M][splits][Nt * K1], so that reduce_splits_kernel adds one density's splits as it adds a single-density call's.
// fp32 runs this exact vector-pipe pair at every accuracy (there is no matrix-core form): full fp32 accuracy, also at digits <= 7.
#pragma once
#include <sctl_amd/device/eval_kernel.hpp>
#include <sctl_amd/device/launch.hpp>

namespace sctl_amd {

template <class R> struct MultiArgs {
  int64_t Nt, Ns;   // targets of this launch, sources
  const R* xt;      // [Nt*3], this launch's targets
  const R* xs;      // [Ns*3]
  const R* xn;      // [Ns*ND] or null
  const R* f;       // density-major: density m at f + m * f_stride
  int64_t f_stride;
  R* v_trg;         // density-major: density m at v_trg + m * v_stride (accumulated into when gridDim.y == 1)
  int64_t v_stride;
  R* partial;       // [M][gridDim.y][Nt*K1] unscaled partial sums when gridDim.y > 1
  int64_t chunk;    // sources per split, a multiple of kTile
  int nact;         // densities in use, 1 <= nact <= M
  R scale;
  KerCtx ctx;
};

template <class Ker, class R, int MODE, int T, int M>
__global__ void __launch_bounds__(kBlock, 2) eval_multi_kernel(const MultiArgs<R> a) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_M<M>;
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
  const int64_t tbase = (int64_t)tile_x * (kBlock * T);
  using KC = typename Ker::template Consts<R>;
  constexpr int SCRATCH = AllPairsScratch<KC>::value;
  __shared__ double kscratch[SCRATCH > 0 ? SCRATCH : 1];
  const KC K = make_consts<KC>(kscratch, SCRATCH, a.ctx, MODE);

  R xt[T][3], acc[T][M][K1];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int64_t t = tbase + j * kBlock + tid;
    if (t >= a.Nt) t = a.Nt - 1;   // tail lanes recompute the last target; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) xt[j][k] = a.xt[t * 3 + k];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K1; k++) acc[j][m][k] = 0;
  }

  const int64_t s_begin = (int64_t)split_y * a.chunk;
  const int64_t s_end = (s_begin + a.chunk < a.Ns) ? s_begin + a.chunk : a.Ns;
  const int64_t len = (s_end > s_begin) ? s_end - s_begin : 0;   // (a split past the sources, which rounds the splits up to eights, has none)
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);
  int repairs = 0;

  for (int it = 0; it < ntile; it++) {
    const int ns = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (tid < ns) {
      const int64_t s = s_begin + (int64_t)it * kTile + tid;
      R px[3], pn[3] = {0, 0, 0}, pf[M][K0];
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.xs[s * 3 + k];
#pragma unroll
      for (int k = 0; k < ND; k++) pn[k] = a.xn[s * ND + k];
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) pf[m][k] = (m < a.nact) ? a.f[m * a.f_stride + s * K0 + k] : R(0);
      R rec[NRECP] = {};
      Ker::template pack_m<R, M>(rec, px, pn, pf);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V w;
#pragma unroll
        for (int e = 0; e < VN; e++) w[e] = rec[v * VN + e];
        tile[tid * NV + v] = w;
      }
    }
    __syncthreads();

    R tacc[T][M][K1];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < K1; k++) tacc[j][m][k] = 0;
      auto one_source = [&](int s) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V w = tile[s * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = w[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
          const R d[3] = {xt[j][0] - rec[0], xt[j][1] - rec[1], xt[j][2] - rec[2]};
          if constexpr (KC::HAS_VARIANT) Ker::template pair_m<R, MODE, MASKED, M, VARIANT>(tacc[j], d, rec, a.ctx, K);
          else Ker::template pair_m<R, MODE, MASKED, M>(tacc[j], d, rec, a.ctx, K);
        }
      };
      if (ns == kTile) {
#pragma unroll UnrollOf<T, M * K1>::value
        for (int s = 0; s < kTile; s++) one_source(s);
      } else {
        for (int s = 0; s < ns; s++) one_source(s);
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
          for (int k = 0; k < K1; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) acc[j][m][k] += tacc[j][m][k];
  }

#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t t = tbase + j * kBlock + tid;
    if (t >= a.Nt) continue;
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_acc<Ker, R, MODE>(acc[j][m]);
      if (gridDim.y == 1) {
        R* v = a.v_trg + m * a.v_stride + t * K1;
#pragma unroll
        for (int k = 0; k < K1; k++) v[k] += acc[j][m][k] * a.scale;
      } else {
        R* p = a.partial + (((int64_t)m * gridDim.y + split_y) * a.Nt + t) * K1;
#pragma unroll
        for (int k = 0; k < K1; k++) p[k] = acc[j][m][k];
      }
    }
  }
}

// ---- launch table: one per built-in kernel (multi_<Kernel>.hip), none for plugin kernels ------------------------------------------------
constexpr int kNumMultiM = 3;                        // forms of 2, 4 and 8 densities
constexpr int kMultiM[kNumMultiM] = {2, 4, 8};
template <class R> using MultiLaunch = void (*)(const MultiArgs<R>&, dim3 grid, hipStream_t);
struct MultiEntry {
  int m_max;                                         // widest form: 4 or 8
  int t[kNumMultiM];                                 // targets per lane of each form (0: no such form)
  MultiLaunch<double> f64[kNumMode][kNumMultiM];
  MultiLaunch<float> f32[kNumMode][kNumMultiM];      // modes 0 and 1 (mode 2 aliases 1)
};

template <class Ker, class R, int MODE, int T, int M> void launch_multi(const MultiArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_multi_kernel<Ker, R, MODE, T, M>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, int T, int M> void fill_multi(MultiEntry& e, int i) {
  e.t[i] = T;
  e.f64[0][i] = launch_multi<Ker, double, 0, T, M>; e.f64[1][i] = launch_multi<Ker, double, 1, T, M>; e.f64[2][i] = launch_multi<Ker, double, 2, T, M>;
  e.f32[0][i] = launch_multi<Ker, float, 0, T, M>; e.f32[1][i] = launch_multi<Ker, float, 1, T, M>; e.f32[2][i] = e.f32[1][i];
}
// T2, T4, T8: targets per lane of the 2-, 4- and 8-density forms; T8 = 0: the kernel's widest form has 4 densities
template <class Ker, int T2, int T4, int T8> MultiEntry make_multi_entry() {
  MultiEntry e{};
  fill_multi<Ker, T2, 2>(e, 0);
  fill_multi<Ker, T4, 4>(e, 1);
  if constexpr (T8 > 0) fill_multi<Ker, T8, 8>(e, 2);
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

}  // namespace sctl_amd
