// Directional derivative (forward-mode tangent) of an all-pairs kernel sum for gfx950 (MI355X).  With u = A(x_trg, x_src, n_src) v_src and a perturbation
// (dx_trg, dx_src, dn_src) of the geometry, the densities held fixed,
//     du[t,k1] += scale * sum_s sum_k0 [(e.grad_d) U(d, n_s) + (dn_s.grad_n) U(d, n_s)][k0][k1] f[s,k0],    d = x_t - x_s,  e = dx_t - dx_s
// (ukernels.hpp: pair_j).  The scheme is eval_grad_kernel's SIDE 0:
//   * a workgroup is 256 lanes; each lane OWNS one target in registers: x_t, dx_t and K1 sums;
//   * grid.x tiles the targets, grid.y splits the sources with the XCD-owned mapping; each split writes unscaled partial sums and reduce_splits_kernel adds
//     them in split order (no atomics: bit-reproducible) — with one split the kernel accumulates into the output directly;
//   * the sources stream through LDS in tiles of 256 plain records {x_s, dx_s, n_s, dn_s, f_s}, 3 + 3 + 2 ND + K0 reals (at most 15), read back at one address
//     by the whole wave;
//   * a tile's pairs go round-robin to JvpChainsOf independent chains of sums, added pairwise at the end of the tile;
//   * a tile runs unmasked into per-tile sums first; one compare per tile finds a coincident pair (inf/NaN) and the tile is re-run masked.
// A null tangent array is a field of zeros: the zeros go into the lane's registers (dx_trg) or into the staged record (dx_src, dn_src) under a launch-uniform
// branch, and the pairs run the same instructions either way — a null tangent and an array of zeros give the same bits.
#pragma once
#include <sctl_amd/device/eval_grad_kernel.hpp>
#include <sctl_amd/device/launch.hpp>

namespace sctl_amd {

template <class R> struct EvalJArgs {
  int64_t Nt, Ns;   // targets of this launch, sources
  const R* xt;      // [Nt*3]
  const R* dxt;     // [Nt*3] or null (zeros)
  const R* xs;      // [Ns*3]
  const R* dxs;     // [Ns*3] or null (zeros)
  const R* xn;      // [Ns*ND] or null (ND == 0)
  const R* dxn;     // [Ns*ND] or null (zeros)
  const R* f;       // [Ns*K0]
  R* dv;            // [Nt*K1], accumulated into (only touched by the main kernel when gridDim.y == 1)
  R* partial;       // gridDim.y > 1: [gridDim.y][Nt*K1] unscaled sums
  int64_t chunk;    // sources per split, a multiple of kTile
  R scale;
  KerCtx ctx;
};

// Targets per lane.  One: a tangent pair is 1.3 to 2.4 times the forward pair's arithmetic, so the LDS reads a second target would share are a
// small part of it; two targets per lane have not been timed
template <class Ker> struct JvpOwnersOf { static constexpr int value = 1; };
// Independent chains of sums per tile, a power of two: 2 (fp64) or 8 (fp32), as the gradient kernels
template <class Ker, class R> struct JvpChainsOf { static constexpr int value = (sizeof(R) == 4) ? 8 : 2; };

template <class Ker, class R, int MODE, int T>
__global__ void __launch_bounds__(kBlock) eval_jvp_kernel(const EvalJArgs<R> a) {
  static_assert(T == 1, "one target per lane");
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NN = ND ? 3 : 1;
  constexpr int NPAY = 3 + 2 * ND + K0;        // what a streamed record holds after its coordinates: dx_s, n_s, dn_s, f_s
  constexpr int NREC = 3 + NPAY;
  using V = typename VecOf<R>::type;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;     // 16-byte LDS words per record
  constexpr int NRECP = NV * VN;
  constexpr int NCH = JvpChainsOf<Ker, R>::value;
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

  R xo[3], eo[3], acc[K1];
  {
    int64_t o = obase + tid;
    if (o >= a.Nt) o = a.Nt - 1;   // tail lanes recompute the last target; never stored
#pragma unroll
    for (int k = 0; k < 3; k++) { xo[k] = a.xt[o * 3 + k]; eo[k] = 0; }
    if (a.dxt) {                   // launch-uniform; null: zeros
#pragma unroll
      for (int k = 0; k < 3; k++) eo[k] = a.dxt[o * 3 + k];
    }
#pragma unroll
    for (int k = 0; k < K1; k++) acc[k] = 0;
  }

  const int64_t p_begin = (int64_t)split_y * a.chunk;
  const int64_t p_end = (p_begin + a.chunk < a.Ns) ? p_begin + a.chunk : a.Ns;
  const int64_t len = (p_end > p_begin) ? p_end - p_begin : 0;
  const int ntile = (int)((len + kTile - 1) / kTile);
  bool always_masked = (ntile < 4);   // few tiles: speculation cannot pay for a repair
  int repairs = 0;

  R px[3] = {0, 0, 0}, pp[NPAY];
#pragma unroll
  for (int k = 0; k < NPAY; k++) pp[k] = 0;
  auto fetch_point = [&](int it) {
    const int64_t p = p_begin + (int64_t)it * kTile + tid;
    if (p < p_end) {
#pragma unroll
      for (int k = 0; k < 3; k++) px[k] = a.xs[p * 3 + k];
      if (a.dxs) {                 // launch-uniform; null: the zeros pp starts with
#pragma unroll
        for (int k = 0; k < 3; k++) pp[k] = a.dxs[p * 3 + k];
      }
#pragma unroll
      for (int k = 0; k < ND; k++) pp[3 + k] = a.xn[p * ND + k];
      if (ND > 0 && a.dxn) {
#pragma unroll
        for (int k = 0; k < ND; k++) pp[3 + ND + k] = a.dxn[p * ND + k];
      }
#pragma unroll
      for (int k = 0; k < K0; k++) pp[3 + 2 * ND + k] = a.f[p * K0 + k];
    }
  };
  if (ntile > 0) fetch_point(0);

  for (int it = 0; it < ntile; it++) {
    const int np = (it == ntile - 1) ? (int)(len - (int64_t)it * kTile) : kTile;   // wave-uniform
    __syncthreads();   // previous tile fully consumed
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
    if (it + 1 < ntile) fetch_point(it + 1);
    __syncthreads();

    // A tile's pairs are dealt round-robin to NCH independent chains of sums, added pairwise when the tile is done (eval_grad_kernel.hpp)
    R tS[K1];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
      R cS[NCH][K1];
#pragma unroll
      for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int k = 0; k < K1; k++) cS[c][k] = 0;
      auto one_point = [&](int p, R (&S)[K1]) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V q = tile[p * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = q[e];
        }
        R st_n[NN], st_m[NN], st_f[K0];
        st_n[0] = 0; st_m[0] = 0;
#pragma unroll
        for (int k = 0; k < ND; k++) { st_n[k] = rec[6 + k]; st_m[k] = rec[6 + ND + k]; }
#pragma unroll
        for (int k = 0; k < K0; k++) st_f[k] = rec[6 + 2 * ND + k];
        const R d[3] = {xo[0] - rec[0], xo[1] - rec[1], xo[2] - rec[2]};
        const R e[3] = {eo[0] - rec[3], eo[1] - rec[4], eo[2] - rec[5]};
        if constexpr (KC::HAS_VARIANT) Ker::template pair_j<R, MODE, MASKED, VARIANT>(S, d, e, st_n, st_m, st_f, a.ctx, K);
        else Ker::template pair_j<R, MODE, MASKED>(S, d, e, st_n, st_m, st_f, a.ctx, K);
      };
      const int whole = np & ~(NCH - 1);     // np == kTile for every tile but possibly the last
      for (int p = 0; p < whole; p += NCH) {
#pragma unroll
        for (int c = 0; c < NCH; c++) one_point(p + c, cS[c]);
      }
      for (int p = whole; p < np; p++) one_point(p, cS[0]);   // the ragged rest of a last tile
#pragma unroll
      for (int h = NCH / 2; h >= 1; h /= 2)
#pragma unroll
        for (int c = 0; c < h; c++)
#pragma unroll
          for (int k = 0; k < K1; k++) cS[c][k] += cS[c + h][k];
#pragma unroll
      for (int k = 0; k < K1; k++) tS[k] = cS[0][k];
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
      for (int k = 0; k < K1; k++) bad |= !(fabs_(tS[k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 8 > ntile) always_masked = true;
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int k = 0; k < K1; k++) acc[k] += tS[k];
  }

  const int64_t o = obase + tid;
  if (o < a.Nt) {
    if (gridDim.y == 1) {
#pragma unroll
      for (int k = 0; k < K1; k++) a.dv[o * K1 + k] += acc[k] * a.scale;
    } else {
      R* p = a.partial + ((int64_t)split_y * a.Nt + o) * K1;
#pragma unroll
      for (int k = 0; k < K1; k++) p[k] = acc[k];
    }
  }
}

// ---- launch table: one per built-in kernel (inst_j_<Kernel>.hip), none for plugin kernels --------------------------------------------------
template <class R> using EvalJLaunch = void (*)(const EvalJArgs<R>&, dim3 grid, hipStream_t);
struct JvpEntry {
  int t;                            // targets per lane (JvpOwnersOf)
  EvalJLaunch<double> f64[kNumMode];
  EvalJLaunch<float> f32[kNumMode];   // modes 0 and 1 (mode 2 aliases 1)
};
template <class Ker, class R, int MODE> void launch_eval_j(const EvalJArgs<R>& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((eval_jvp_kernel<Ker, R, MODE, JvpOwnersOf<Ker>::value>), grid, dim3(kBlock), 0, st, a);
}
template <class Ker> JvpEntry make_jvp_entry() {
  JvpEntry e{};
  e.t = JvpOwnersOf<Ker>::value;
  e.f64[0] = launch_eval_j<Ker, double, 0>; e.f64[1] = launch_eval_j<Ker, double, 1>; e.f64[2] = launch_eval_j<Ker, double, 2>;
  e.f32[0] = launch_eval_j<Ker, float, 0>; e.f32[1] = launch_eval_j<Ker, float, 1>; e.f32[2] = e.f32[1];
  return e;
}

// defined in inst_j_*.hip
const JvpEntry& jvp_Laplace3D_FxU();
const JvpEntry& jvp_Laplace3D_DxU();
const JvpEntry& jvp_Laplace3D_FxdU();
const JvpEntry& jvp_Stokes3D_FxU();
const JvpEntry& jvp_Stokes3D_DxU();
const JvpEntry& jvp_Stokes3D_FxT();
const JvpEntry& jvp_Stokes3D_FSxU();
const JvpEntry& jvp_Stokes3D_FxUP();
const JvpEntry& jvp_Laplace3D_FDxUdU();
const JvpEntry& jvp_Helmholtz3D_FxU();

}  // namespace sctl_amd
