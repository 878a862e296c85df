// Coordinate and normal gradients of an all-pairs kernel sum for gfx950 (MI355X).  With target weights w, L = sum_t sum_k1 w[t,k1] u[t,k1] and the pair's
// scalar phi_ts = sum_k0 sum_k1 w[t,k1] U(x_t - x_s, n_s)[k0][k1] f[s,k0] (ukernels.hpp: pair_g),
//     g_trg[t,j] +=  scale * sum_s d phi_ts / d d_j          SIDE 0: the TARGETS own the output, the sources stream
//     g_src[s,j] += -scale * sum_t d phi_ts / d d_j          SIDE 1: the SOURCES own the outputs, the targets stream
//     g_nrm[s,j] +=  scale * sum_t d phi_ts / d n_j          SIDE 1, kernels with a normal, out of the same pass
//
// The scheme is eval_kernel's and eval_transpose_kernel's, one template with the side as a parameter:
//   * a workgroup is 256 lanes; each lane OWNS T points in registers: coordinates, w[K1] (SIDE 0) or the normal and f[K0] (SIDE 1), and 3 (+3) sums;
//   * grid.x tiles the owners (256*T per workgroup), grid.y splits the streamed range; each split writes unscaled partial sums and
//     reduce_splits_kernel adds them in split order (no atomics: bit-reproducible) — with one split the kernel accumulates into the outputs directly;
//   * the other set streams through LDS in tiles of 256 plain records, {x_s, n_s, f_s} (SIDE 0) or {x_t, w_t} (SIDE 1), read back at one address
//     by the whole wave;
//   * a tile's pairs go round-robin to 2 (fp64) or 8 (fp32) independent chains of sums, added pairwise at the end of the tile;
//   * a tile runs unmasked into per-tile sums first; one compare per tile finds a coincident pair (inf/NaN) and the tile is re-run masked.
// Both sides call the same pair_g with the same d = x_trg - x_src; SIDE 1 changes the sign of the coordinate sums once, when they leave the registers.
#pragma once
#include "eval_kernel.hpp"

namespace sctl_amd {

template <class R> struct EvalGArgs {
  int64_t No, Nst;  // owners, streamed points
  const R* xo;      // [No*3]   owners' coordinates
  const R* xst;     // [Nst*3]  streamed coordinates
  const R* xn;      // source normals or null: the streamed set's [Nst*ND] (SIDE 0), the owners' [No*ND] (SIDE 1)
  const R* f;       // source densities: [Nst*K0] (SIDE 0), [No*K0] (SIDE 1)
  const R* w;       // target weights:   [No*K1] (SIDE 0), [Nst*K1] (SIDE 1)
  R* g;             // [No*3] coordinate gradient, accumulated into; null: not stored (only touched by the main kernel when gridDim.y == 1)
  R* gn;            // [No*3] normal gradient (SIDE 1, ND > 0), likewise
  R* partial;       // gridDim.y > 1: [gridDim.y][No*3] unscaled coordinate sums, then, SIDE 1 with a normal, [gridDim.y][No*3] normal sums
  int64_t chunk;    // streamed points per split, a multiple of kTile
  R scale;
  KerCtx ctx;
};

template <class Ker, class R, int MODE, int SIDE, int T>
__global__ void __launch_bounds__(kBlock) eval_grad_kernel(const EvalGArgs<R> a) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NN = ND ? 3 : 1;
  constexpr bool WANT_N = (SIDE == 1 && ND > 0);
  constexpr int NPAY = (SIDE == 0) ? ND + K0 : K1;   // what a streamed record holds after its coordinates
  constexpr int NREC = 3 + NPAY;
  using V = typename VecOf<R>::type;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;     // 16-byte LDS words per record
  constexpr int NRECP = NV * VN;
  constexpr int NCH = (sizeof(R) == 4) ? 8 : 2;   // independent chains of sums per tile, a power of two (below)
  __shared__ V tile[kTile * NV];

  const int tid = threadIdx.x;
  // (owner tile, streamed split) of this workgroup; XCD k owns the splits [k S/8, (k+1) S/8) one at a time when they come in eights (eval_kernel.hpp)
  unsigned tile_x = blockIdx.x, split_y = blockIdx.y;
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

  // the owners: w (SIDE 0) or n and f (SIDE 1); the arrays of the other side are placeholders of one element
  R xo[T][3], own_n[T][NN], own_f[T][SIDE == 1 ? K0 : 1], own_w[T][SIDE == 0 ? K1 : 1], accG[T][3], accN[T][NN];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int64_t o = obase + j * kBlock + tid;
    if (o >= a.No) o = a.No - 1;   // tail lanes recompute the last owner; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) { xo[j][k] = a.xo[o * 3 + k]; accG[j][k] = 0; }
#pragma unroll
    for (int k = 0; k < NN; k++) { own_n[j][k] = (SIDE == 1 && ND) ? a.xn[o * ND + k] : R(0); accN[j][k] = 0; }
    if constexpr (SIDE == 1) {
#pragma unroll
      for (int k = 0; k < K0; k++) own_f[j][k] = a.f[o * K0 + k];
      own_w[j][0] = 0;
    } else {
#pragma unroll
      for (int k = 0; k < K1; k++) own_w[j][k] = a.w[o * K1 + k];
      own_f[j][0] = 0;
    }
  }

  const int64_t p_begin = (int64_t)split_y * a.chunk;
  const int64_t p_end = (p_begin + a.chunk < a.Nst) ? p_begin + a.chunk : a.Nst;
  const int64_t len = (p_end > p_begin) ? p_end - p_begin : 0;
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  constexpr bool PREFETCH = (T == 1);   // as eval_kernel
  R px[3] = {0, 0, 0}, pp[NPAY];
#pragma unroll
  for (int k = 0; k < NPAY; k++) pp[k] = 0;
  auto fetch_point = [&](int it) {
    const int64_t p = p_begin + (int64_t)it * kTile + tid;
    if (p < p_end) {
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.xst[p * 3 + k];
      if constexpr (SIDE == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++) pp[k] = a.xn[p * ND + k];
#pragma unroll
        for (int k = 0; k < K0; k++) pp[ND + k] = a.f[p * K0 + k];
      } else {
#pragma unroll
        for (int k = 0; k < K1; k++) pp[k] = a.w[p * K1 + k];
      }
    }
  };
  if (PREFETCH && ntile > 0) fetch_point(0);

  for (int it = 0; it < ntile; it++) {
    const int np = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (!PREFETCH) fetch_point(it);
    if (tid < np) {
      R rec[NRECP] = {};
      rec[0] = px[0]; rec[1] = px[1]; rec[2] = px[2];
#pragma unroll
      for (int k = 0; k < NPAY; k++) rec[3 + k] = pp[k];
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V q;
#pragma unroll
        for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
        tile[tid * NV + v] = q;
      }
    }
    if (PREFETCH && it + 1 < ntile) fetch_point(it + 1);
    __syncthreads();

    // A tile's pairs are dealt round-robin to NCH independent chains of sums, added pairwise when the tile is done: NCH pairs in flight per lane, and
    // a chain adds up 256 / NCH terms, not 256 — in fp32 the rounding of one long chain was the largest error of the whole sum.
    R tG[T][3], tN[T][NN];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
      R cG[NCH][T][3], cN[NCH][T][NN];
#pragma unroll
      for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int j = 0; j < T; j++) {
#pragma unroll
          for (int k = 0; k < 3; k++) cG[c][j][k] = 0;
#pragma unroll
          for (int k = 0; k < NN; k++) cN[c][j][k] = 0;
        }
      auto one_point = [&](int p, R (&G)[T][3], R (&N)[T][NN]) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V q = tile[p * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = q[e];
        }
        // the streamed point's share of the pair's inputs
        R st_n[NN], st_f[SIDE == 0 ? K0 : 1], st_w[SIDE == 1 ? K1 : 1];
        st_n[0] = 0; st_f[0] = 0; st_w[0] = 0;
        if constexpr (SIDE == 0) {
#pragma unroll
          for (int k = 0; k < ND; k++) st_n[k] = rec[3 + k];
#pragma unroll
          for (int k = 0; k < K0; k++) st_f[k] = rec[3 + ND + k];
        } else {
#pragma unroll
          for (int k = 0; k < K1; k++) st_w[k] = rec[3 + k];
        }
        auto pair = [&](R (&Gj)[3], R (&Nj)[NN], const R (&d)[3], const R (&n)[NN], const R (&f)[K0], const R (&w)[K1]) {
          if constexpr (KC::HAS_VARIANT) Ker::template pair_g<R, MODE, MASKED, VARIANT, WANT_N>(Gj, Nj, d, n, f, w, a.ctx, K);
          else Ker::template pair_g<R, MODE, MASKED, WANT_N>(Gj, Nj, d, n, f, w, a.ctx, K);
        };
#pragma unroll
        for (int j = 0; j < T; j++) {
          if constexpr (SIDE == 0) {   // d = x_trg - x_src on both sides
            const R d[3] = {xo[j][0] - rec[0], xo[j][1] - rec[1], xo[j][2] - rec[2]};
            pair(G[j], N[j], d, st_n, st_f, own_w[j]);
          } else {
            const R d[3] = {rec[0] - xo[j][0], rec[1] - xo[j][1], rec[2] - xo[j][2]};
            pair(G[j], N[j], d, own_n[j], own_f[j], st_w);
          }
        }
      };
      const int whole = np & ~(NCH - 1);     // np == kTile for every tile but possibly the last
      for (int p = 0; p < whole; p += NCH) {
#pragma unroll
        for (int c = 0; c < NCH; c++) one_point(p + c, cG[c], cN[c]);
      }
      for (int p = whole; p < np; p++) one_point(p, cG[0], cN[0]);   // the ragged rest of a last tile
#pragma unroll
      for (int h = NCH / 2; h >= 1; h /= 2)
#pragma unroll
        for (int c = 0; c < h; c++)
#pragma unroll
          for (int j = 0; j < T; j++) {
#pragma unroll
            for (int k = 0; k < 3; k++) cG[c][j][k] += cG[c + h][j][k];
#pragma unroll
            for (int k = 0; k < NN; k++) cN[c][j][k] += cN[c + h][j][k];
          }
#pragma unroll
      for (int j = 0; j < T; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) tG[j][k] = cG[0][j][k];
#pragma unroll
        for (int k = 0; k < NN; k++) tN[j][k] = cN[0][j][k];
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
      for (int j = 0; j < T; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) bad |= !(fabs_(tG[j][k]) <= max_finite<R>());
        if constexpr (WANT_N) {
#pragma unroll
          for (int k = 0; k < 3; k++) bad |= !(fabs_(tN[j][k]) <= max_finite<R>());
        }
      }
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++) {
#pragma unroll
      for (int k = 0; k < 3; k++) accG[j][k] += tG[j][k];
      if constexpr (WANT_N) {
#pragma unroll
        for (int k = 0; k < 3; k++) accN[j][k] += tN[j][k];
      }
    }
  }

#pragma unroll
  for (int j = 0; j < T; j++) {
    const int64_t o = obase + j * kBlock + tid;
    if (o < a.No) {
      R G[3];
#pragma unroll
      for (int k = 0; k < 3; k++) G[k] = (SIDE == 1) ? -accG[j][k] : accG[j][k];   // d d / d x_src = -1
      if (gridDim.y == 1) {
        if (a.g) {
#pragma unroll
          for (int k = 0; k < 3; k++) a.g[o * 3 + k] += G[k] * a.scale;
        }
        if constexpr (WANT_N) {
          if (a.gn) {
#pragma unroll
            for (int k = 0; k < 3; k++) a.gn[o * 3 + k] += accN[j][k] * a.scale;
          }
        }
      } else {
        R* p = a.partial + ((int64_t)split_y * a.No + o) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] = G[k];
        if constexpr (WANT_N) {
          R* pn = a.partial + (((int64_t)gridDim.y + split_y) * a.No + o) * 3;
#pragma unroll
          for (int k = 0; k < 3; k++) pn[k] = accN[j][k];
        }
      }
    }
  }
}

}  // namespace sctl_amd
