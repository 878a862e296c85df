// Geometry gradients for several density / weight rows in a single pass: the gradient evaluator of include/sctl_amd/device/eval_grad_kernel.hpp with M rows
// per point (ukernels.hpp: pair_gm).  With L = sum_m <w[m], A f[m]> and the pair's scalar phi_ts = sum_m phi(f[m][s], w[m][t]),
//     g_trg[t,j] +=  scale * sum_s d phi_ts / d d_j          SIDE 0: the TARGETS own the output, the sources stream
//     g_src[s,j] += -scale * sum_t d phi_ts / d d_j          SIDE 1: the SOURCES own the outputs, the targets stream
//     g_nrm[s,j] +=  scale * sum_t d phi_ts / d n_j          SIDE 1, kernels with a normal, out of the same pass
// The outputs are sums over the rows: a lane keeps 3 (+3) sums whatever M is, only its inputs widen.  Everything a pair costs that does not depend on the rows
// (distance, reciprocal square root and its refinement, the powers of y, d.n, Helmholtz's e^{ikr}) is computed once per pair.
//
// Same scheme as eval_grad_kernel: 256-lane workgroups, one owner per lane, LDS tiles of 256 plain records read by wave broadcast,
// splits of the streamed range with the XCD-owned mapping, partial sums reduced in split order (no atomics), 2 (fp64) or 8 (fp32) chains of sums per tile,
// unmasked speculation with per-tile repair.  What differs:
//   * a SIDE 0 lane holds w[M][K1] and a streamed record is {x_s, n_s, f[M][K0]}; a SIDE 1 lane holds n and f[M][K0] and a record is {x_t, w[M][K1]};
//   * rows are density-major: row m of f is f + m * f_stride, of w is w + m * w_stride;
//   * the last pass of a call may use fewer rows than the form's M (nact): the others are loaded and packed as 0 and add exactly 0;
//   * a tile's record is loaded when it is staged (no register prefetch: a record has up to 3 + 9 M reals).
#pragma once
#include <sctl_amd/device/eval_grad_kernel.hpp>
#include <sctl_amd/device/launch.hpp>

namespace sctl_amd {

template <class R> struct MultiGArgs {
  int64_t No, Nst;   // owners, streamed points of this launch
  const R* xo;       // [No*3]   owners' coordinates
  const R* xst;      // [Nst*3]  streamed coordinates
  const R* xn;       // source normals or null: the streamed set's [Nst*ND] (SIDE 0), the owners' [No*ND] (SIDE 1)
  const R* f;        // source densities, row m at f + m * f_stride: the streamed set's (SIDE 0), this launch's owners' (SIDE 1)
  const R* w;        // target weights, row m at w + m * w_stride: this launch's owners' (SIDE 0), the streamed set's (SIDE 1)
  int64_t f_stride, w_stride;
  R* g;              // [No*3] coordinate gradient, accumulated into; null: not stored (only touched by the main kernel when gridDim.y == 1)
  R* gn;             // [No*3] normal gradient (SIDE 1, ND > 0), likewise
  R* partial;        // gridDim.y > 1: [gridDim.y][No*3] unscaled coordinate sums, then, SIDE 1 with a normal, [gridDim.y][No*3] normal sums
  int64_t chunk;     // streamed points per split, a multiple of kTile
  int nact;          // rows in use, 1 <= nact <= M
  R scale;
  KerCtx ctx;
};

template <class Ker, class R, int MODE, int SIDE, int T, int M>
__global__ void __launch_bounds__(kBlock, 2) eval_multi_grad_kernel(const MultiGArgs<R> a) {
  static_assert(T == 1, "one owner per lane");
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NN = ND ? 3 : 1;
  constexpr bool WANT_N = (SIDE == 1 && ND > 0);
  constexpr int NPAY = (SIDE == 0) ? ND + M * K0 : M * K1;   // what a streamed record holds after its coordinates
  constexpr int NREC = 3 + NPAY;
  using V = typename VecOf<R>::type;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;     // 16-byte LDS words per record
  constexpr int NRECP = NV * VN;
  constexpr int NCH = (sizeof(R) == 4) ? 8 : 2;   // independent chains of sums per tile, a power of two
  __shared__ V tile[kTile * NV];

  const int tid = threadIdx.x;
  unsigned tile_x = blockIdx.x, split_y = blockIdx.y;   // the XCD-owned split mapping of eval_kernel
  if (gridDim.y >= 8 && (gridDim.y & 7) == 0) {
    const unsigned b = blockIdx.x + gridDim.x * blockIdx.y, i = b >> 3;
    tile_x = i % gridDim.x;
    split_y = (b & 7) * (gridDim.y >> 3) + i / gridDim.x;
  }
  const int64_t obase = (int64_t)tile_x * kBlock;
  using KC = typename Ker::template Consts<R>;
  constexpr int SCRATCH = AllPairsScratch<KC>::value;
  __shared__ double kscratch[SCRATCH > 0 ? SCRATCH : 1];
  const KC K = make_consts<KC>(kscratch, SCRATCH, a.ctx, MODE);

  // the owner: w rows (SIDE 0) or n and f rows (SIDE 1); the arrays of the other side are placeholders
  R xo[3], own_n[NN], own_f[SIDE == 1 ? M : 1][K0], own_w[SIDE == 0 ? M : 1][K1], accG[3], accN[NN];
  {
    int64_t o = obase + tid;
    if (o >= a.No) o = a.No - 1;   // tail lanes recompute the last owner; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) { xo[k] = a.xo[o * 3 + k]; accG[k] = 0; }
#pragma unroll
    for (int k = 0; k < NN; k++) { own_n[k] = (SIDE == 1 && ND) ? a.xn[o * ND + k] : R(0); accN[k] = 0; }
    if constexpr (SIDE == 1) {
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) own_f[m][k] = (m < a.nact) ? a.f[m * a.f_stride + o * K0 + k] : R(0);
#pragma unroll
      for (int k = 0; k < K1; k++) own_w[0][k] = 0;
    } else {
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) own_w[m][k] = (m < a.nact) ? a.w[m * a.w_stride + o * K1 + k] : R(0);
#pragma unroll
      for (int k = 0; k < K0; k++) own_f[0][k] = 0;
    }
  }

  const int64_t p_begin = (int64_t)split_y * a.chunk;
  const int64_t p_end = (p_begin + a.chunk < a.Nst) ? p_begin + a.chunk : a.Nst;
  const int64_t len = (p_end > p_begin) ? p_end - p_begin : 0;   // (a split past the streamed set, which rounds the splits up to eights, has none)
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  for (int it = 0; it < ntile; it++) {
    const int np = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
    if (tid < np) {
      const int64_t p = p_begin + (int64_t)it * kTile + tid;
      R rec[NRECP] = {};
#pragma unroll
      for (int k = 0; k < 3; k++) rec[k] = a.xst[p * 3 + k];
      if constexpr (SIDE == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++) rec[3 + k] = a.xn[p * ND + k];
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < K0; k++) rec[3 + ND + m * K0 + k] = (m < a.nact) ? a.f[m * a.f_stride + p * K0 + k] : R(0);
      } else {
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < K1; k++) rec[3 + m * K1 + k] = (m < a.nact) ? a.w[m * a.w_stride + p * K1 + k] : R(0);
      }
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V q;
#pragma unroll
        for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
        tile[tid * NV + v] = q;
      }
    }
    __syncthreads();

    // A tile's pairs are dealt round-robin to NCH independent chains of sums, added pairwise when the tile is done (eval_grad_kernel.hpp)
    R tG[3], tN[NN];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
      R cG[NCH][3], cN[NCH][NN];
#pragma unroll
      for (int c = 0; c < NCH; c++) {
#pragma unroll
        for (int k = 0; k < 3; k++) cG[c][k] = 0;
#pragma unroll
        for (int k = 0; k < NN; k++) cN[c][k] = 0;
      }
      auto pair = [&](R (&Gj)[3], R (&Nj)[NN], const R (&d)[3], const R (&n)[NN], const R (&f)[M][K0], const R (&w)[M][K1]) {
        if constexpr (KC::HAS_VARIANT) Ker::template pair_gm<R, MODE, MASKED, VARIANT, WANT_N, M>(Gj, Nj, d, n, f, w, a.ctx, K);
        else Ker::template pair_gm<R, MODE, MASKED, WANT_N, M>(Gj, Nj, d, n, f, w, a.ctx, K);
      };
      auto one_point = [&](int p, R (&G)[3], R (&N)[NN]) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V q = tile[p * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = q[e];
        }
        if constexpr (SIDE == 0) {   // d = x_trg - x_src on both sides
          R st_n[NN], st_f[M][K0];
          st_n[0] = 0;
#pragma unroll
          for (int k = 0; k < ND; k++) st_n[k] = rec[3 + k];
#pragma unroll
          for (int m = 0; m < M; m++)
#pragma unroll
            for (int k = 0; k < K0; k++) st_f[m][k] = rec[3 + ND + m * K0 + k];
          const R d[3] = {xo[0] - rec[0], xo[1] - rec[1], xo[2] - rec[2]};
          pair(G, N, d, st_n, st_f, own_w);
        } else {
          R st_w[M][K1];
#pragma unroll
          for (int m = 0; m < M; m++)
#pragma unroll
            for (int k = 0; k < K1; k++) st_w[m][k] = rec[3 + m * K1 + k];
          const R d[3] = {rec[0] - xo[0], rec[1] - xo[1], rec[2] - xo[2]};
          pair(G, N, d, own_n, own_f, st_w);
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
        for (int c = 0; c < h; c++) {
#pragma unroll
          for (int k = 0; k < 3; k++) cG[c][k] += cG[c + h][k];
#pragma unroll
          for (int k = 0; k < NN; k++) cN[c][k] += cN[c + h][k];
        }
#pragma unroll
      for (int k = 0; k < 3; k++) tG[k] = cG[0][k];
#pragma unroll
      for (int k = 0; k < NN; k++) tN[k] = cN[0][k];
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
      for (int k = 0; k < 3; k++) bad |= !(fabs_(tG[k]) <= max_finite<R>());
      if constexpr (WANT_N) {
#pragma unroll
        for (int k = 0; k < 3; k++) bad |= !(fabs_(tN[k]) <= max_finite<R>());
      }
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int k = 0; k < 3; k++) accG[k] += tG[k];
    if constexpr (WANT_N) {
#pragma unroll
      for (int k = 0; k < 3; k++) accN[k] += tN[k];
    }
  }

  const int64_t o = obase + tid;
  if (o < a.No) {
    R G[3];
#pragma unroll
    for (int k = 0; k < 3; k++) G[k] = (SIDE == 1) ? -accG[k] : accG[k];   // d d / d x_src = -1
    if (gridDim.y == 1) {
      if (a.g) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.g[o * 3 + k] += G[k] * a.scale;
      }
      if constexpr (WANT_N) {
        if (a.gn) {
#pragma unroll
          for (int k = 0; k < 3; k++) a.gn[o * 3 + k] += accN[k] * a.scale;
        }
      }
    } else {
      R* p = a.partial + ((int64_t)split_y * a.No + o) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) p[k] = G[k];
      if constexpr (WANT_N) {
        R* pn = a.partial + (((int64_t)gridDim.y + split_y) * a.No + o) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) pn[k] = accN[k];
      }
    }
  }
}

// ---- launch table: one per built-in kernel (gmulti_<Kernel>.hip), none for plugin kernels ------------------------------------------------
constexpr int kNumMultiGM = 3;                       // forms of 2, 4 and 8 rows
constexpr int kMultiGM[kNumMultiGM] = {2, 4, 8};
template <class R> using MultiGLaunch = void (*)(const MultiGArgs<R>&, dim3 grid, hipStream_t);
struct MultiGEntry {
  int m_max;                                            // widest form: 2, 4 or 8 (both sides of a pass run the same form)
  MultiGLaunch<double> f64[kNumMode][2][kNumMultiGM];   // [mode][side][form]; null: no such form
  MultiGLaunch<float> f32[kNumMode][2][kNumMultiGM];    // modes 0 and 1 (mode 2 aliases 1)
};

template <class Ker, class R, int MODE, int SIDE, int M> void launch_multi_g(const MultiGArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_multi_grad_kernel<Ker, R, MODE, SIDE, 1, M>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker, int SIDE, int M> void fill_multi_g(MultiGEntry& e, int i) {
  e.f64[0][SIDE][i] = launch_multi_g<Ker, double, 0, SIDE, M>; e.f64[1][SIDE][i] = launch_multi_g<Ker, double, 1, SIDE, M>;
  e.f64[2][SIDE][i] = launch_multi_g<Ker, double, 2, SIDE, M>;
  e.f32[0][SIDE][i] = launch_multi_g<Ker, float, 0, SIDE, M>; e.f32[1][SIDE][i] = launch_multi_g<Ker, float, 1, SIDE, M>; e.f32[2][SIDE][i] = e.f32[1][SIDE][i];
}
// M_MAX: the kernel's widest form, 2, 4 or 8
template <class Ker, int M_MAX> MultiGEntry make_multi_g_entry() {
  static_assert(HasPairGM<Ker>::value, "the functor supplies no pair_gm");
  MultiGEntry e{};
  fill_multi_g<Ker, 0, 2>(e, 0); fill_multi_g<Ker, 1, 2>(e, 0);
  if constexpr (M_MAX >= 4) { fill_multi_g<Ker, 0, 4>(e, 1); fill_multi_g<Ker, 1, 4>(e, 1); }
  if constexpr (M_MAX >= 8) { fill_multi_g<Ker, 0, 8>(e, 2); fill_multi_g<Ker, 1, 8>(e, 2); }
  e.m_max = M_MAX;
  return e;
}

// defined in gmulti_*.hip
const MultiGEntry& multi_g_Laplace3D_FxU();
const MultiGEntry& multi_g_Laplace3D_DxU();
const MultiGEntry& multi_g_Laplace3D_FxdU();
const MultiGEntry& multi_g_Stokes3D_FxU();
const MultiGEntry& multi_g_Stokes3D_DxU();
const MultiGEntry& multi_g_Stokes3D_FxT();
const MultiGEntry& multi_g_Stokes3D_FSxU();
const MultiGEntry& multi_g_Stokes3D_FxUP();
const MultiGEntry& multi_g_Laplace3D_FDxUdU();
const MultiGEntry& multi_g_Helmholtz3D_FxU();

}  // namespace sctl_amd
