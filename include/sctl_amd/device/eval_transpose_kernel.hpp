// Transposed all-pairs evaluation for gfx950 (MI355X): the adjoint of eval_kernel's sum,
//     g[s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[t,k1],
// i.e. KernelMatrix (generic-kernel.txx:191-307, (Ns*K0) x (Nt*K1)) applied to a vector of target weights without ever forming it.
//
// The scheme is eval_kernel's with the roles of the two point sets exchanged:
//   * a workgroup is 256 lanes; each lane OWNS T sources in registers: coordinates, the normal where ND > 0, and K0 accumulators;
//   * grid.x tiles the sources (256*T per workgroup), grid.y splits the TARGET range; each split writes unscaled partial sums
//     [splits][Ns*K0] and reduce_splits_kernel adds them in split order (no atomics: bit-reproducible) — with one split the kernel
//     accumulates into g directly;
//   * targets stream through LDS in tiles of 256 packed records (ukernels.hpp: pack_t()), read back at one address by the whole wave;
//   * a tile runs unmasked into per-tile sums first; one compare per tile finds a coincident pair (inf/NaN) and the tile is re-run masked.
// The pair keeps d = x_trg - x_src, the forward pair's sign, so the odd kernels need no sign flip.
#pragma once
#include "eval_kernel.hpp"

namespace sctl_amd {

template <class R> struct EvalTArgs {
  int64_t Nt, Ns;
  const R* xt;      // [Nt*3]   streamed
  const R* xs;      // [Ns*3]   owners
  const R* xn;      // [Ns*ND] or null
  const R* w;       // [Nt*K1]  target weights
  R* g_src;         // [Ns*K0], accumulated into (only touched by the main kernel when gridDim.y == 1)
  R* partial;       // [gridDim.y][Ns*K0] unscaled partial sums when gridDim.y > 1
  int64_t chunk;    // targets per split, a multiple of kTile
  R scale;
  KerCtx ctx;
};

template <class Ker, class R, int MODE, int T>
__global__ void __launch_bounds__(kBlock) eval_transpose_kernel(const EvalTArgs<R> a) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::NREC_T, NN = ND ? 3 : 1;
  using V = typename VecOf<R>::type;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;     // 16-byte LDS words per record
  constexpr int NRECP = NV * VN;
  __shared__ V tile[kTile * NV];

  const int tid = threadIdx.x;
  // (source tile, target split) of this workgroup; XCD k owns the splits [k S/8, (k+1) S/8) one at a time when they come in eights (eval_kernel.hpp)
  unsigned tile_x = blockIdx.x, split_y = blockIdx.y;
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

  R xs[T][3], xn[T][NN], acc[T][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int64_t s = sbase + j * kBlock + tid;
    if (s >= a.Ns) s = a.Ns - 1;   // tail lanes recompute the last source; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.xn[s * ND + k] : R(0);
#pragma unroll
    for (int k = 0; k < K0; k++) acc[j][k] = 0;
  }

  const int64_t t_begin = (int64_t)split_y * a.chunk;
  const int64_t t_end = (t_begin + a.chunk < a.Nt) ? t_begin + a.chunk : a.Nt;
  const int64_t len = (t_end > t_begin) ? t_end - t_begin : 0;
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  constexpr bool PREFETCH = (T == 1);   // as eval_kernel: one owner per lane is what small owner counts run
  R px[3] = {0, 0, 0}, pw[K1];
#pragma unroll
  for (int k = 0; k < K1; k++) pw[k] = 0;
  auto fetch_target = [&](int it) {
    const int64_t t = t_begin + (int64_t)it * kTile + tid;
    if (t < t_end) {
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.xt[t * 3 + k];
#pragma unroll
      for (int k = 0; k < K1; k++) pw[k] = a.w[t * K1 + k];
    }
  };
  if (PREFETCH && ntile > 0) fetch_target(0);

  for (int it = 0; it < ntile; it++) {
    const int nt = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (!PREFETCH) fetch_target(it);
    if (tid < nt) {
      R rec[NRECP] = {};
      pack_t_record<Ker, R, MODE>(rec, px, pw);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V q;
#pragma unroll
        for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
        tile[tid * NV + v] = q;
      }
    }
    if (PREFETCH && it + 1 < ntile) fetch_target(it + 1);
    __syncthreads();

    R tacc[T][K0];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int k = 0; k < K0; k++) tacc[j][k] = 0;
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
          if constexpr (KC::HAS_VARIANT) Ker::template pair_t<R, MODE, MASKED, VARIANT>(tacc[j], d, xn[j], rec, a.ctx, K);
          else Ker::template pair_t<R, MODE, MASKED>(tacc[j], d, xn[j], rec, a.ctx, K);
        }
      };
      if (nt == kTile) {
#pragma unroll UnrollOf<T, Ker::K0>::value
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
        for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][k] += tacc[j][k];
  }

#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t s = sbase + j * kBlock + tid;
    finish_t_acc<Ker, R, MODE>(acc[j]);
    if (s < a.Ns) {
      if (gridDim.y == 1) {
#pragma unroll
        for (int k = 0; k < K0; k++) a.g_src[s * K0 + k] += acc[j][k] * a.scale;
      } else {
        R* p = a.partial + ((int64_t)split_y * a.Ns + s) * K0;
#pragma unroll
        for (int k = 0; k < K0; k++) p[k] = acc[j][k];
      }
    }
  }
}

}  // namespace sctl_amd
