// BoundaryIntegralOp::ComputeNearInterac on the device: the precomputed per-element near-field
// operator matrices stay resident in HBM; one application is a batch of small row-major GEMVs U_ = F_ . K_near_
// (boundary_integral.txx:1092-1102), the permutation by near_scatter_index (:1129) and the per-target accumulation
// (:1131-1140).  HBM-bound: every byte of K_near is read exactly once per application and nothing else is of that order.
#include <sctl_amd.h>
#include "staging.hpp"
#include "workspace.hpp"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace sctl_amd {
int set_error(int code, const std::string& msg);   // capi.hip (internal.hpp): records the message for sctl_amd_last_error()

namespace {

#define NEAR_TRY(expr)                                                                                              \
  do {                                                                                                              \
    hipError_t e_ = (expr);                                                                                         \
    if (e_ != hipSuccess) return set_error(SCTL_AMD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

constexpr int kCols = 64;     // columns (target dofs) of an operator block handled by one workgroup: one per lane of a wave
constexpr int kRowGroups = 4; // the four waves of a workgroup take rows s = g, g + 4, ...
constexpr int kNearBlock = kCols * kRowGroups;

struct NearWork {   // one workgroup: columns [t0, t0 + 64) (narrow) or [t0, t0 + 256) (wide) of one element's block
  int64_t k_off;    // first entry of the block in K_near
  int64_t f_off;    // first density value of the element
  int64_t u_off;    // first entry of the element's run in U_near
  int32_t src_dof, trg_dof, t0, wide;
};

// rows s0, s0 + step, ... of one column: UNR row loads in flight per lane.  K_near is read exactly once per application:
// non-temporal loads keep it from displacing F and U_near in L2.
template <class R, int UNR>
__device__ __forceinline__ R near_column_sum(const R* __restrict__ Kc, const R* __restrict__ Fe, int64_t ld, int s0, int step, int src_dof) {
  R acc[UNR];
#pragma unroll
  for (int u = 0; u < UNR; u++) acc[u] = 0;
  for (int s = s0; s < src_dof; s += UNR * step) {
    R kv[UNR], fv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; u++) {
      const int r = s + u * step;              // wave-uniform
      const bool ok = r < src_dof;
      kv[u] = ok ? __builtin_nontemporal_load(Kc + (int64_t)r * ld) : R(0);
      fv[u] = ok ? Fe[r] : R(0);
    }
#pragma unroll
    for (int u = 0; u < UNR; u++) acc[u] += fv[u] * kv[u];
  }
  static_assert(UNR == 8, "pairwise reduction below is written for 8 partial sums");
  return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// U_near[u_off + t] = sum_s F[f_off + s] * K[k_off + s * trg_dof + t], lanes along t, every lane walks all rows of its
// column (no reduction across lanes: deterministic).
//   wide   (blocks at least 256 columns wide): one work item per workgroup, whose 256 lanes read 2 KB of a row at a time;
//   narrow : one work item (64 columns) per WAVE; the four waves of a workgroup take four consecutive items.
// A workgroup walks the work list with the stride of the grid, so small blocks do not pay a workgroup launch each.
template <class R>
__global__ void __launch_bounds__(kNearBlock) near_gemv_kernel(const NearWork* __restrict__ wide_work, int64_t n_wide, const NearWork* __restrict__ narrow_work,
                                                               int64_t n_narrow, const R* __restrict__ K, const R* __restrict__ F, R* __restrict__ U_near) {
  for (int64_t wi = blockIdx.x; wi < n_wide; wi += gridDim.x) {
    const NearWork w = wide_work[wi];
    const int t = w.t0 + (int)threadIdx.x;
    if (t < w.trg_dof) U_near[w.u_off + t] = near_column_sum<R, 8>(K + w.k_off + t, F + w.f_off, w.trg_dof, 0, 1, w.src_dof);
  }
  const int lane = threadIdx.x & (kCols - 1), wave = threadIdx.x / kCols;
  for (int64_t wi = (int64_t)blockIdx.x * kRowGroups + wave; wi < n_narrow; wi += (int64_t)gridDim.x * kRowGroups) {
    const NearWork w = narrow_work[wi];
    const int t = w.t0 + lane;
    if (t < w.trg_dof) U_near[w.u_off + t] = near_column_sum<R, 8>(K + w.k_off + t, F + w.f_off, w.trg_dof, 0, 1, w.src_dof);
  }
}

// U[i*k1 + k] += sum over the target's near entries, in the order of the scattered array (boundary_integral.txx:1129-1140)
template <class R>
__global__ void __launch_bounds__(256) near_accumulate_kernel(int64_t ntrg, int k1, const int64_t* __restrict__ scatter, const int64_t* __restrict__ trg_cnt,
                                                              const int64_t* __restrict__ trg_dsp, const R* __restrict__ U_near, R* __restrict__ U) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntrg * k1) return;
  const int64_t i = idx / k1;
  const int k = (int)(idx - i * k1);
  const int64_t p0 = trg_dsp[i], p1 = p0 + trg_cnt[i];
  if (p1 == p0) return;
  R acc = U[idx];
  int64_t p = p0;
  for (; p + 4 <= p1; p += 4) {      // four independent index loads, then four independent gathers, added in list order
    const int64_t i0 = scatter[p], i1 = scatter[p + 1], i2 = scatter[p + 2], i3 = scatter[p + 3];
    const R v0 = U_near[i0 * k1 + k], v1 = U_near[i1 * k1 + k], v2 = U_near[i2 * k1 + k], v3 = U_near[i3 * k1 + k];
    acc = (((acc + v0) + v1) + v2) + v3;
  }
  for (; p < p1; p++) acc += U_near[scatter[p] * k1 + k];
  U[idx] = acc;
}

// ---- several densities against one operator (sctl_amd_near_apply_densities_*): U_[m] = F_[m] . K_near_, Matrix::GEMM(U_, F_, K_near_) with
// M rows in F_ (boundary_integral.txx:1092-1102), every operator entry read ONCE for the M densities ------------------------------------------
// Rows 0, 1, ... of one column for M densities: 8 row loads in flight per lane as in near_column_sum, each entry multiplied into M
// accumulators.  The densities of a row are wave-uniform (Fe and f_stride are: scalar loads, 8 consecutive rows of a density at a time);
// NP partial sums per density keep M * NP accumulators in registers (fp64, M = 8, NP = 2: 32 VGPRs), so the order in which a row's terms
// are added differs from the single-density kernel's.  Densities nact .. M-1 of a last, partly filled pass repeat density nact-1 and
// are not stored.
template <class R, int M, int NP>
__device__ __forceinline__ void near_column_sums(const R* __restrict__ Kc, const R* __restrict__ Fe, int64_t f_stride, int nact, int64_t ld, int src_dof,
                                                 R (&out)[M]) {
  static_assert(NP == 2 || NP == 4, "the reductions below are written for 2 or 4 partial sums");
  constexpr int UNR = 8;
  R acc[M][NP];
  const R* Fm[M];
#pragma unroll
  for (int m = 0; m < M; m++) {
    Fm[m] = Fe + (int64_t)(m < nact ? m : nact - 1) * f_stride;
#pragma unroll
    for (int p = 0; p < NP; p++) acc[m][p] = 0;
  }
  int s = 0;
  for (; s + UNR <= src_dof; s += UNR) {     // whole groups of 8 rows: no predicates
    R kv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; u++) kv[u] = __builtin_nontemporal_load(Kc + (int64_t)(s + u) * ld);
#pragma unroll
    for (int u = 0; u < UNR; u++)
#pragma unroll
      for (int m = 0; m < M; m++) acc[m][u % NP] += Fm[m][s + u] * kv[u];
  }
  if (s < src_dof) {                         // the last 1 .. 7 rows
    R kv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; u++) kv[u] = (s + u < src_dof) ? __builtin_nontemporal_load(Kc + (int64_t)(s + u) * ld) : R(0);
#pragma unroll
    for (int u = 0; u < UNR; u++)
#pragma unroll
      for (int m = 0; m < M; m++) acc[m][u % NP] += ((s + u < src_dof) ? Fm[m][s + u] : R(0)) * kv[u];
  }
#pragma unroll
  for (int m = 0; m < M; m++) out[m] = (NP == 2) ? acc[m][0] + acc[m][NP - 1] : (acc[m][0] + acc[m][1]) + (acc[m][NP - 2] + acc[m][NP - 1]);
}

// near_gemv_kernel's work list and lane mapping, M densities per pass: U_near[m * un_stride + u_off + t] = sum_s F[m * f_stride + f_off + s] *
// K[k_off + s * trg_dof + t].  The wave index of a narrow item goes through readfirstlane, so that the item and with it the density
// addresses are known to be wave-uniform.
template <class R, int M>
__global__ void __launch_bounds__(kNearBlock) near_gemm_kernel(const NearWork* __restrict__ wide_work, int64_t n_wide, const NearWork* __restrict__ narrow_work,
                                                               int64_t n_narrow, const R* __restrict__ K, const R* __restrict__ F, int64_t f_stride, int nact,
                                                               R* __restrict__ U_near, int64_t un_stride) {
  constexpr int NP = (M >= 8) ? 2 : 4;
  for (int64_t wi = blockIdx.x; wi < n_wide; wi += gridDim.x) {
    const NearWork w = wide_work[wi];
    const int t = w.t0 + (int)threadIdx.x;
    if (t < w.trg_dof) {
      R u[M];
      near_column_sums<R, M, NP>(K + w.k_off + t, F + w.f_off, f_stride, nact, w.trg_dof, w.src_dof, u);
#pragma unroll
      for (int m = 0; m < M; m++)
        if (m < nact) U_near[(int64_t)m * un_stride + w.u_off + t] = u[m];
    }
  }
  const int lane = threadIdx.x & (kCols - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kCols));
  for (int64_t wi = (int64_t)blockIdx.x * kRowGroups + wave; wi < n_narrow; wi += (int64_t)gridDim.x * kRowGroups) {
    const NearWork w = narrow_work[wi];
    const int t = w.t0 + lane;
    if (t < w.trg_dof) {
      R u[M];
      near_column_sums<R, M, NP>(K + w.k_off + t, F + w.f_off, f_stride, nact, w.trg_dof, w.src_dof, u);
#pragma unroll
      for (int m = 0; m < M; m++)
        if (m < nact) U_near[(int64_t)m * un_stride + w.u_off + t] = u[m];
    }
  }
}

// near_accumulate_kernel for M densities: a target's displacement, count and scatter indices are read once and used for every row;
// each row adds its entries in the order of the scattered array, as the single-density kernel does.
template <class R, int M>
__global__ void __launch_bounds__(256) near_accumulate_multi_kernel(int64_t ntrg, int k1, int nact, const int64_t* __restrict__ scatter,
                                                                    const int64_t* __restrict__ trg_cnt, const int64_t* __restrict__ trg_dsp,
                                                                    const R* __restrict__ U_near, int64_t un_stride, R* __restrict__ U, int64_t u_stride) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntrg * k1) return;
  const int64_t i = idx / k1;
  const int k = (int)(idx - i * k1);
  const int64_t p0 = trg_dsp[i], p1 = p0 + trg_cnt[i];
  if (p1 == p0) return;
  R acc[M];
#pragma unroll
  for (int m = 0; m < M; m++) acc[m] = (m < nact) ? U[(int64_t)m * u_stride + idx] : R(0);
  int64_t p = p0;
  for (; p + 2 <= p1; p += 2) {      // two index loads, then 2 M independent gathers
    const int64_t j0 = scatter[p] * k1 + k, j1 = scatter[p + 1] * k1 + k;
    R v0[M], v1[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
      const int64_t row = (int64_t)(m < nact ? m : nact - 1) * un_stride;
      v0[m] = U_near[row + j0];
      v1[m] = U_near[row + j1];
    }
#pragma unroll
    for (int m = 0; m < M; m++) acc[m] = (acc[m] + v0[m]) + v1[m];
  }
  if (p < p1) {
    const int64_t j0 = scatter[p] * k1 + k;
#pragma unroll
    for (int m = 0; m < M; m++) acc[m] += U_near[(int64_t)(m < nact ? m : nact - 1) * un_stride + j0];
  }
#pragma unroll
  for (int m = 0; m < M; m++)
    if (m < nact) U[(int64_t)m * u_stride + idx] = acc[m];
}

// ---- transposed application (sctl_amd_near_apply_transpose_*): G[f_off + s] += sum_t K[k_off + s * trg_dof + t] * Wn[u_off + t] -----------------
// A row of a block is contiguous, so lanes run along t and the sum goes ACROSS lanes.  One wave holds 8 loads per lane in flight: 8 / NC
// row steps times NC column chunks.  A row step is 64 / W rows, W = 2^lw lanes per row: W = 64 for blocks at least 64 columns wide, a
// narrower block packs several rows into the wave and the reduction stops at width W.  Each row's partial sums are added in a lane in
// the order of the column passes, then across the W lanes by an xor butterfly: a fixed tree, every lane of the row ends with the same bits.
struct NearWorkT {     // rows [r0, r1) of one element's block
  int64_t k_off, f_off, u_off;
  int32_t src_dof, trg_dof, r0, r1;
  int32_t lw;          // log2 of the lanes per row
  int32_t nc;          // column chunks of a row in flight: 1, 2, 4 or 8 (blocks with few rows fill the 8 loads along the row instead)
};

constexpr int kSplitCols = 1024;   // rows at least this long are cut over the four waves of a workgroup

// Wn[scatter[p] * k1 + k] = W[i * k1 + k] for the entries p of target i: the inverse of near_accumulate_kernel
template <class R>
__global__ void __launch_bounds__(256) near_gather_kernel(int64_t ntrg, int k1, const int64_t* __restrict__ scatter, const int64_t* __restrict__ trg_cnt,
                                                          const int64_t* __restrict__ trg_dsp, const R* __restrict__ W, R* __restrict__ Wn) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntrg * k1) return;
  const int64_t i = idx / k1;
  const int k = (int)(idx - i * k1);
  const int64_t p0 = trg_dsp[i], p1 = p0 + trg_cnt[i];
  if (p1 == p0) return;
  const R w = W[idx];
  for (int64_t p = p0; p < p1; p++) Wn[scatter[p] * k1 + k] = w;
}

// Rows rb + ru * (64 / W) + lane / W, ru = 0 .. 8 / NC - 1, against the columns [c0, c1): acc[ru] = the row's sum, in every lane of the row.
// rb, r1, c0, c1 and lw are wave-uniform.  K_near is read exactly once per application, with non-temporal loads as in near_column_sum.
template <class R, int NC>
__device__ __forceinline__ void near_t_batch(const R* __restrict__ Kb, const R* __restrict__ We, int ld, int rb, int r1, int c0, int c1, int lw, int lane,
                                             R (&acc)[8 / NC]) {
  constexpr int NR = 8 / NC;
  const int W = 1 << lw, step = 64 >> lw, row0 = rb + (lane >> lw), l = lane & (W - 1);
#pragma unroll
  for (int ru = 0; ru < NR; ru++) acc[ru] = 0;
  const bool rows_full = rb + NR * step <= r1;
  for (int cb = c0; cb < c1; cb += NC * W) {
    R kv[8], wv[NC];
    if (rows_full && cb + NC * W <= c1) {     // whole batch inside the block: no predicates
#pragma unroll
      for (int cu = 0; cu < NC; cu++) wv[cu] = We[cb + cu * W + l];
#pragma unroll
      for (int u = 0; u < 8; u++) kv[u] = __builtin_nontemporal_load(Kb + (int64_t)(row0 + (u / NC) * step) * ld + (cb + (u % NC) * W + l));
    } else {
#pragma unroll
      for (int cu = 0; cu < NC; cu++) {
        const int t = cb + cu * W + l;
        wv[cu] = (t < c1) ? We[t] : R(0);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int r = row0 + (u / NC) * step, t = cb + (u % NC) * W + l;
        kv[u] = (r < r1 && t < c1) ? __builtin_nontemporal_load(Kb + (int64_t)r * ld + t) : R(0);
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) acc[u / NC] += kv[u] * wv[u % NC];
  }
#pragma unroll
  for (int ru = 0; ru < NR; ru++)
    for (int o = W >> 1; o > 0; o >>= 1) acc[ru] += __shfl_xor(acc[ru], o);
}

// one wave, all rows of an item; lane 0 of a row adds the row's sum to its entry of G
template <class R, int NC>
__device__ __forceinline__ void near_t_item(const NearWorkT& w, const R* __restrict__ K, const R* __restrict__ Wn, R* __restrict__ G, int lane) {
  constexpr int NR = 8 / NC;
  const int step = 64 >> w.lw;
  for (int rb = w.r0; rb < w.r1; rb += NR * step) {
    R acc[NR];
    near_t_batch<R, NC>(K + w.k_off, Wn + w.u_off, w.trg_dof, rb, w.r1, 0, w.trg_dof, w.lw, lane, acc);
    const int row0 = rb + (lane >> w.lw);
#pragma unroll
    for (int ru = 0; ru < NR; ru++) {
      const int r = row0 + ru * step;
      if ((lane & ((1 << w.lw) - 1)) == 0 && r < w.r1) G[w.f_off + r] += acc[ru];
    }
  }
}

//   split items (rows of kSplitCols columns and more): one per workgroup, at most 8 rows (one or two rows where the block has fewer than 8,
//          which then have their 8 loads along the row: 8 chunks of one row, or 4 chunks of two where a wave's run has fewer than 8 chunks); the four waves take four runs of whole 64-column chunks, their sums meet in LDS and wave 0 adds
//          them in the order ((0 + 1) + (2 + 3));
//   wave items : one per WAVE, as the narrow items of near_gemv_kernel.
// No atomics: a row belongs to one item, its entry of G is written by one lane.
template <class R>
__global__ void __launch_bounds__(kNearBlock) near_gemv_t_kernel(const NearWorkT* __restrict__ split_work, int64_t n_split, const NearWorkT* __restrict__ wave_work,
                                                                 int64_t n_wave, const R* __restrict__ K, const R* __restrict__ Wn, R* __restrict__ G) {
  __shared__ R part[kRowGroups][8];
  const int lane = threadIdx.x & (kCols - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kCols));
  for (int64_t wi = blockIdx.x; wi < n_split; wi += gridDim.x) {
    const NearWorkT w = split_work[wi];
    const int per = ((w.trg_dof + kCols - 1) / kCols + kRowGroups - 1) / kRowGroups * kCols;   // columns per wave
    const int c0 = wave * per < w.trg_dof ? wave * per : w.trg_dof, c1 = c0 + per < w.trg_dof ? c0 + per : w.trg_dof;
    R acc[8];
    if (w.nc == 8) {
      R one[1];
      near_t_batch<R, 8>(K + w.k_off, Wn + w.u_off, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, one);
      acc[0] = one[0];
#pragma unroll
      for (int j = 1; j < 8; j++) acc[j] = 0;
    } else if (w.nc == 4) {   // two rows, four chunks each
      R two[2];
      near_t_batch<R, 4>(K + w.k_off, Wn + w.u_off, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, two);
      acc[0] = two[0];
      acc[1] = two[1];
#pragma unroll
      for (int j = 2; j < 8; j++) acc[j] = 0;
    } else {
      near_t_batch<R, 1>(K + w.k_off, Wn + w.u_off, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, acc);
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (lane == j) part[wave][j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 8 && w.r0 + (int)threadIdx.x < w.r1)
      G[w.f_off + w.r0 + threadIdx.x] += (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    __syncthreads();
  }
  for (int64_t wi = (int64_t)blockIdx.x * kRowGroups + wave; wi < n_wave; wi += (int64_t)gridDim.x * kRowGroups) {
    const NearWorkT w = wave_work[wi];
    if (w.nc == 1) near_t_item<R, 1>(w, K, Wn, G, lane);
    else if (w.nc == 2) near_t_item<R, 2>(w, K, Wn, G, lane);
    else if (w.nc == 4) near_t_item<R, 4>(w, K, Wn, G, lane);
    else near_t_item<R, 8>(w, K, Wn, G, lane);
  }
}

// ---- several weight vectors through the transposed application (sctl_amd_near_apply_transpose_densities_*): G[m][f_off + s] += sum_t K[k_off +
// s * trg_dof + t] * Wn[m][u_off + t], every operator entry read ONCE for the M vectors ----------------------------------------------------------
// The gathered weights are INTERLEAVED: Wn[(near entry * k1 + k) * wn_stride + m], wn_stride = the widest form the handle has used.  One scattered
// store of the gather and one weight load of a lane then cover the M values of an entry, which lie in one cache line.

// near_gather_kernel for M rows: a target's displacement, count and scatter indices are read once.  Rows nact .. M-1 of a partly filled pass are
// not read; their slots are written as zero.
template <class R, int M>
__global__ void __launch_bounds__(256) near_gather_multi_kernel(int64_t ntrg, int k1, int nact, const int64_t* __restrict__ scatter, const int64_t* __restrict__ trg_cnt,
                                                                const int64_t* __restrict__ trg_dsp, const R* __restrict__ W, int64_t w_stride, R* __restrict__ Wn,
                                                                int wn_stride) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntrg * k1) return;
  const int64_t i = idx / k1;
  const int k = (int)(idx - i * k1);
  const int64_t p0 = trg_dsp[i], p1 = p0 + trg_cnt[i];
  if (p1 == p0) return;
  R w[M];
#pragma unroll
  for (int m = 0; m < M; m++) w[m] = (m < nact) ? W[(int64_t)m * w_stride + idx] : R(0);
  for (int64_t p = p0; p < p1; p++) {
    R* dst = Wn + (scatter[p] * k1 + k) * wn_stride;
#pragma unroll
    for (int m = 0; m < M; m++) dst[m] = w[m];
  }
}

// near_t_batch for M vectors: the same rows, columns, loads and order of additions in a lane; acc[ru * M + m] is the partial sum of row ru and vector m.
// The sums then go through the SAME tree as near_t_batch's butterflies (offsets W/2 .. 1, own + partner at every level), but a level hands half of the
// live sums to the partner and keeps the other half: S - 1 exchanges for S = (8 / NC) * M sums over the first log2(S) levels instead of S per level.
// On return the lane l of a row group (l = lane & (W - 1)) holds in acc[0 .. n) the finished sums number first .. first + n - 1:
//   W >= S : n = 1, first = l / (W / S), the same bits in all W / S lanes of that run;       W < S : n = S / W, first = l * n.
template <class R, int NC, int M>
__device__ __forceinline__ void near_t_batch_m(const R* __restrict__ Kb, const R* __restrict__ We, int ws, int ld, int rb, int r1, int c0, int c1, int lw, int lane,
                                               R (&acc)[(8 / NC) * M]) {
  constexpr int NR = 8 / NC, S = NR * M;
  const int W = 1 << lw, step = 64 >> lw, row0 = rb + (lane >> lw), l = lane & (W - 1);
#pragma unroll
  for (int i = 0; i < S; i++) acc[i] = 0;
  const bool rows_full = rb + NR * step <= r1;
  for (int cb = c0; cb < c1; cb += NC * W) {
    R kv[8], wv[NC][M];
    if (rows_full && cb + NC * W <= c1) {     // whole batch inside the block: no predicates
#pragma unroll
      for (int cu = 0; cu < NC; cu++)
#pragma unroll
        for (int m = 0; m < M; m++) wv[cu][m] = We[(int64_t)(cb + cu * W + l) * ws + m];
#pragma unroll
      for (int u = 0; u < 8; u++) kv[u] = __builtin_nontemporal_load(Kb + (int64_t)(row0 + (u / NC) * step) * ld + (cb + (u % NC) * W + l));
      __asm__ volatile("" ::: "memory");     // (keeps the two paths' loads apart: none sinks below the join to serve both)
    } else {
#pragma unroll
      for (int cu = 0; cu < NC; cu++) {
        const int t = cb + cu * W + l;
#pragma unroll
        for (int m = 0; m < M; m++) wv[cu][m] = (t < c1) ? We[(int64_t)t * ws + m] : R(0);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int r = row0 + (u / NC) * step, t = cb + (u % NC) * W + l;
        kv[u] = (r < r1 && t < c1) ? __builtin_nontemporal_load(Kb + (int64_t)r * ld + t) : R(0);
      }
      __asm__ volatile("" ::: "memory");
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int m = 0; m < M; m++) acc[(u / NC) * M + m] += kv[u] * wv[u % NC][m];
  }
  int o = W >> 1;
#pragma unroll
  for (int j = 0; j < 6; j++) {               // level j: offset W >> (j + 1), S >> (j + 1) sums stay
    const int h = S >> (j + 1);
    if (o > 0) {                              // (wave-uniform)
      if (h >= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < (h >= 1 ? h : 1); i++) {
          const R keep = up ? acc[i + h] : acc[i], send = up ? acc[i] : acc[i + h];
          acc[i] = keep + __shfl_xor(send, o);
        }
      } else {
        acc[0] += __shfl_xor(acc[0], o);
      }
      o >>= 1;
    }
  }
}

// which finished sums of near_t_batch_m this lane owns, and whether it is the one lane that stores them
template <int S>
__device__ __forceinline__ void near_t_owned(int lw, int lane, int& first, int& n, bool& writer) {
  constexpr int LS = S == 1 ? 0 : S == 2 ? 1 : S == 4 ? 2 : S == 8 ? 3 : S == 16 ? 4 : S == 32 ? 5 : 6;
  static_assert((1 << LS) == S, "S is a power of two up to 64");
  const int l = lane & ((1 << lw) - 1);
  if (lw >= LS) { n = 1; first = l >> (lw - LS); writer = (l & ((1 << (lw - LS)) - 1)) == 0; }
  else { n = S >> lw; first = l << (LS - lw); writer = true; }
}

// one wave, all rows of an item; the owner lane of a sum adds it to its entry of G
template <class R, int NC, int M>
__device__ __forceinline__ void near_t_item_m(const NearWorkT& w, const R* __restrict__ K, const R* __restrict__ Wn, int ws, R* __restrict__ G, int64_t g_stride, int nact,
                                              int lane) {
  constexpr int NR = 8 / NC, S = NR * M;
  const int step = 64 >> w.lw;
  int first, n;
  bool writer;
  near_t_owned<S>(w.lw, lane, first, n, writer);
  for (int rb = w.r0; rb < w.r1; rb += NR * step) {
    R acc[S];
    near_t_batch_m<R, NC, M>(K + w.k_off, Wn + w.u_off * ws, ws, w.trg_dof, rb, w.r1, 0, w.trg_dof, w.lw, lane, acc);
    const int row0 = rb + (lane >> w.lw);
#pragma unroll
    for (int i = 0; i < S; i++) {
      const int id = first + i, m = id % M, r = row0 + (id / M) * step;
      if (i < n && writer && m < nact && r < w.r1) G[(int64_t)m * g_stride + w.f_off + r] += acc[i];
    }
  }
}

// near_gemv_t_kernel for M weight vectors per pass: its work list, lane mapping, loads and trees.  A split item leaves (8 / NC) * M sums per wave in LDS.
template <class R, int M>
__global__ void __launch_bounds__(kNearBlock) __attribute__((amdgpu_waves_per_eu(2, 8)))
near_gemm_t_kernel(const NearWorkT* __restrict__ split_work, int64_t n_split, const NearWorkT* __restrict__ wave_work, int64_t n_wave, const R* __restrict__ K,
                   const R* __restrict__ Wn, int ws, int nact, R* __restrict__ G, int64_t g_stride) {
  __shared__ R part[kRowGroups][8 * M];
  const int lane = threadIdx.x & (kCols - 1), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kCols));
  for (int64_t wi = blockIdx.x; wi < n_split; wi += gridDim.x) {
    const NearWorkT w = split_work[wi];
    const int per = ((w.trg_dof + kCols - 1) / kCols + kRowGroups - 1) / kRowGroups * kCols;   // columns per wave
    const int c0 = wave * per < w.trg_dof ? wave * per : w.trg_dof, c1 = c0 + per < w.trg_dof ? c0 + per : w.trg_dof;
    const R* We = Wn + w.u_off * ws;
    int S;                    // sums of this item: rows in flight x M, sum number = row * M + m
    if (w.nc == 8) {
      R a[M];
      near_t_batch_m<R, 8, M>(K + w.k_off, We, ws, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, a);
      S = M;
      if ((lane & (64 / M - 1)) == 0) part[wave][lane / (64 / M)] = a[0];
    } else if (w.nc == 4) {   // two rows, four chunks each
      R a[2 * M];
      near_t_batch_m<R, 4, M>(K + w.k_off, We, ws, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, a);
      S = 2 * M;
      if ((lane & (32 / M - 1)) == 0) part[wave][lane / (32 / M)] = a[0];
    } else {
      R a[8 * M];
      near_t_batch_m<R, 1, M>(K + w.k_off, We, ws, w.trg_dof, w.r0, w.r1, c0, c1, 6, lane, a);
      S = 8 * M;
      if ((lane & (8 / M - 1)) == 0) part[wave][lane / (8 / M)] = a[0];
    }
    __syncthreads();
    const int id = (int)threadIdx.x, m = id % M, r = w.r0 + id / M;
    if (id < S && m < nact && r < w.r1)
      G[(int64_t)m * g_stride + w.f_off + r] += (part[0][id] + part[1][id]) + (part[2][id] + part[3][id]);
    __syncthreads();
  }
  for (int64_t wi = (int64_t)blockIdx.x * kRowGroups + wave; wi < n_wave; wi += (int64_t)gridDim.x * kRowGroups) {
    const NearWorkT w = wave_work[wi];
    if (w.nc == 1) near_t_item_m<R, 1, M>(w, K, Wn, ws, G, g_stride, nact, lane);
    else if (w.nc == 2) near_t_item_m<R, 2, M>(w, K, Wn, ws, G, g_stride, nact, lane);
    else if (w.nc == 4) near_t_item_m<R, 4, M>(w, K, Wn, ws, G, g_stride, nact, lane);
    else near_t_item_m<R, 8, M>(w, K, Wn, ws, G, g_stride, nact, lane);
  }
}

struct DevMem {
  void* p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
  hipError_t realloc(size_t bytes) {   // (hipFree waits for the work that still uses the old block)
    if (p) { hipError_t e = hipFree(p); p = nullptr; if (e != hipSuccess) return e; }
    return alloc(bytes);
  }
};
struct PinMem {
  void* p = nullptr;
  ~PinMem() { if (p) (void)hipHostFree(p); }
  hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocPortable); }
  hipError_t realloc(size_t bytes) {
    if (p) { hipError_t e = hipHostFree(p); p = nullptr; if (e != hipSuccess) return e; }
    return alloc(bytes);
  }
};

}  // namespace
}  // namespace sctl_amd

using namespace sctl_amd;

struct sctl_amd_near {
  int real = 0, device = 0, k0 = 0, k1 = 0, cus = 256;
  int64_t nelem = 0, ntrg = 0, n_near = 0, f_len = 0, k_len = 0, nwork = 0;
  DevMem K, work, scatter, trg_cnt, trg_dsp, F, U_near, U;   // work: the wide items, then the narrow ones
  int64_t n_wide = 0, n_narrow = 0;
  PinMem stage;                 // F down, U up (host entry)
  // several densities: allocated on first use, never by sctl_amd_near_create
  DevMem U_near_m;              // [m_cap][n_near * k1], m_cap = the widest pass used so far; zero-filled when grown
  int m_cap = 0;
  DevMem F_m, U_m;              // [nd_cap] densities and potentials of the host entry
  PinMem stage_m;
  int nd_cap = 0;
  // transposed application: the element shapes are kept on the host, the work list and the gathered weights are made on the first
  // transposed call, never by sctl_amd_near_create
  std::vector<int64_t> e_nds, e_near, e_kcnt;
  DevMem work_t, Wn;            // work_t: the split items, then the wave items; Wn: W in near-list order, [n_near * k1]
  int64_t n_split = 0, n_wave_t = 0;
  bool t_ready = false;
  // several weight vectors: allocated on first use
  DevMem Wn_m;                  // [n_near * k1][mt_cap] (interleaved), mt_cap = the widest pass used so far; zero-filled when grown
  int mt_cap = 0;
  hipStream_t st = nullptr;
  ~sctl_amd_near() { if (st) (void)hipStreamDestroy(st); }
};

namespace {

template <class R>
int apply_on_stream(sctl_amd_near* h, const R* F, R* U, hipStream_t st) {
  (void)hipGetLastError();
  if (h->nwork > 0) {
    const int64_t resident = (int64_t)h->cus * 8;   // 8 workgroups of 4 waves fill a CU
    const int64_t groups = h->n_wide + (h->n_narrow + kRowGroups - 1) / kRowGroups;
    const unsigned grid = (unsigned)(groups < resident * 4 ? groups : resident * 4);
    const NearWork* wl = (const NearWork*)h->work.p;
    hipLaunchKernelGGL((near_gemv_kernel<R>), dim3(grid), dim3(kNearBlock), 0, st, wl, h->n_wide, wl + h->n_wide, h->n_narrow, (const R*)h->K.p, F,
                       (R*)h->U_near.p);
    NEAR_TRY(hipGetLastError());
  }
  if (h->n_near > 0 && h->ntrg > 0) {
    const int64_t n = h->ntrg * h->k1;
    hipLaunchKernelGGL((near_accumulate_kernel<R>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->ntrg, h->k1, (const int64_t*)h->scatter.p,
                       (const int64_t*)h->trg_cnt.p, (const int64_t*)h->trg_dsp.p, (const R*)h->U_near.p, U);
    NEAR_TRY(hipGetLastError());
  }
  return SCTL_AMD_OK;
}


// the pass for `left` densities still to do: the narrowest of 2 / 4 / 8 that takes them all, else the widest
inline int near_pass_width(int left) { return left <= 2 ? 2 : left <= 4 ? 4 : 8; }

template <class R, int M>
int near_pass(sctl_amd_near* h, int nact, const R* F, R* U, hipStream_t st) {
  const int64_t un_stride = h->n_near * h->k1;
  if (h->nwork > 0) {
    const int64_t resident = (int64_t)h->cus * 8;
    const int64_t groups = h->n_wide + (h->n_narrow + kRowGroups - 1) / kRowGroups;
    const unsigned grid = (unsigned)(groups < resident * 4 ? groups : resident * 4);
    const NearWork* wl = (const NearWork*)h->work.p;
    hipLaunchKernelGGL((near_gemm_kernel<R, M>), dim3(grid), dim3(kNearBlock), 0, st, wl, h->n_wide, wl + h->n_wide, h->n_narrow, (const R*)h->K.p, F, h->f_len, nact,
                       (R*)h->U_near_m.p, un_stride);
    NEAR_TRY(hipGetLastError());
  }
  const int64_t n = h->ntrg * h->k1;
  hipLaunchKernelGGL((near_accumulate_multi_kernel<R, M>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->ntrg, h->k1, nact, (const int64_t*)h->scatter.p,
                     (const int64_t*)h->trg_cnt.p, (const int64_t*)h->trg_dsp.p, (const R*)h->U_near_m.p, un_stride, U, n);
  NEAR_TRY(hipGetLastError());
  return SCTL_AMD_OK;
}

// nd >= 2 densities, density-major: passes of 8, the last pass on the narrowest form that takes what is left; a single density left over
// goes through the single-density kernels.
template <class R>
int apply_densities_on_stream(sctl_amd_near* h, int nd, const R* F, R* U, hipStream_t st) {
  (void)hipGetLastError();
  if (h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  const int widest = near_pass_width(nd);
  if (widest > h->m_cap) {   // U_near for the widest pass of this call; the runs of matrix-free elements are never written and stay zero
    const size_t bytes = (size_t)widest * h->n_near * h->k1 * sizeof(R);
    h->m_cap = 0;
    NEAR_TRY(h->U_near_m.realloc(bytes));
    NEAR_TRY(hipMemsetAsync(h->U_near_m.p, 0, bytes, st));
    h->m_cap = widest;
  }
  const int64_t u_len = h->ntrg * h->k1;
  for (int m0 = 0; m0 < nd;) {
    const int left = nd - m0;
    const R* Fp = F + (int64_t)m0 * h->f_len;
    R* Up = U + (int64_t)m0 * u_len;
    if (left == 1) return apply_on_stream<R>(h, Fp, Up, st);
    const int M = near_pass_width(left), nact = left < M ? left : M;
    const int rc = (M == 2) ? near_pass<R, 2>(h, nact, Fp, Up, st) : (M == 4) ? near_pass<R, 4>(h, nact, Fp, Up, st) : near_pass<R, 8>(h, nact, Fp, Up, st);
    if (rc) return rc;
    m0 += nact;
  }
  return SCTL_AMD_OK;
}

// The transposed work list.  Lanes per row: 64 from 64 columns on; below that the power of two (at least 8, or the first one that holds
// the row when it has fewer than 8 columns) that leaves the fewest idle lane slots over the row's passes, the widest of equals: 33 columns
// take 5 passes of 8 lanes (8 rows per wave and step), 63 take 2 passes of 32.
void build_transpose_work(const sctl_amd_near* h, std::vector<NearWorkT>& split, std::vector<NearWorkT>& wave) {
  int64_t f_len = 0, n_near = 0, k_len = 0;
  for (int64_t e = 0; e < h->nelem; e++) {
    const int64_t sd = h->e_nds[(size_t)e] * h->k0, td = h->e_near[(size_t)e] * h->k1, kc = h->e_kcnt[(size_t)e];
    if (kc != 0 && sd > 0 && td > 0) {
      NearWorkT w{k_len * h->k0 * h->k1, f_len, n_near * h->k1, (int32_t)sd, (int32_t)td, 0, 0, 6, 1};
      if (td >= kSplitCols) {
        // fewer than 8 rows: the loads go along the row, as many 64-column chunks in flight as a wave's run of columns fills (8, or 4 and then
        // two rows per item)
        const int64_t per = ((td + kCols - 1) / kCols + kRowGroups - 1) / kRowGroups;   // chunks per wave, as near_gemv_t_kernel cuts the row
        w.nc = sd >= 8 ? 1 : per >= 8 ? 8 : 4;                                          // (kSplitCols columns: at least 4 chunks per wave)
        const int64_t rows = 8 / w.nc;
        for (int64_t r = 0; r < sd; r += rows) { w.r0 = (int32_t)r; w.r1 = (int32_t)(r + rows < sd ? r + rows : sd); split.push_back(w); }
      } else {
        int lw = 6;
        if (td < 8) { lw = 0; while ((1 << lw) < td) lw++; }
        else if (td < kCols) {
          int64_t best = 0;
          for (int c = 3; c <= 5; c++) {
            const int64_t W = 1 << c, padded = (td + W - 1) / W * W;
            if (best == 0 || padded <= best) { best = padded; lw = c; }
          }
        }
        const int64_t W = 1 << lw, step = kCols / W, passes = (td + W - 1) / W;
        int nc = 1;
        while (nc < 8 && (8 / nc) * step > sd) nc *= 2;      // few rows: fill the 8 loads along the row
        while (nc > 1 && nc > passes) nc /= 2;
        const int64_t batch = (8 / nc) * step;                 // rows of one pass of the wave
        int64_t rows = batch * (4096 / (batch * td) > 1 ? 4096 / (batch * td) : 1);   // about 4096 entries per item
        w.lw = lw; w.nc = nc;
        for (int64_t r = 0; r < sd; r += rows) { w.r0 = (int32_t)r; w.r1 = (int32_t)(r + rows < sd ? r + rows : sd); wave.push_back(w); }
      }
    }
    f_len += sd;
    n_near += h->e_near[(size_t)e];
    k_len += kc;
  }
}

int prepare_transpose(sctl_amd_near* h, hipStream_t st) {
  if (h->t_ready) return SCTL_AMD_OK;
  std::vector<NearWorkT> work, wave;
  build_transpose_work(h, work, wave);
  h->n_split = (int64_t)work.size(); h->n_wave_t = (int64_t)wave.size();
  work.insert(work.end(), wave.begin(), wave.end());
  const size_t rs = real_size(h->real);
  NEAR_TRY(h->work_t.realloc(work.size() * sizeof(NearWorkT)));
  NEAR_TRY(h->Wn.realloc((size_t)h->n_near * h->k1 * rs));
  if (!work.empty()) NEAR_TRY(hipMemcpy(h->work_t.p, work.data(), work.size() * sizeof(NearWorkT), hipMemcpyHostToDevice));
  // (every entry of Wn is written by the gather when near_scatter_index is a permutation; zero otherwise.  On the caller's stream, as U_near_m)
  NEAR_TRY(hipMemsetAsync(h->Wn.p, 0, (size_t)h->n_near * h->k1 * rs, st));
  h->t_ready = true;
  return SCTL_AMD_OK;
}

template <class R>
int apply_transpose_on_stream(sctl_amd_near* h, const R* W, R* G, hipStream_t st) {
  (void)hipGetLastError();
  if (h->n_split + h->n_wave_t == 0) return SCTL_AMD_OK;
  const int64_t n = h->ntrg * h->k1;
  hipLaunchKernelGGL((near_gather_kernel<R>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->ntrg, h->k1, (const int64_t*)h->scatter.p,
                     (const int64_t*)h->trg_cnt.p, (const int64_t*)h->trg_dsp.p, W, (R*)h->Wn.p);
  NEAR_TRY(hipGetLastError());
  const int64_t resident = (int64_t)h->cus * 8;
  const int64_t groups = h->n_split + (h->n_wave_t + kRowGroups - 1) / kRowGroups;
  const unsigned grid = (unsigned)(groups < resident * 4 ? groups : resident * 4);
  const NearWorkT* wl = (const NearWorkT*)h->work_t.p;
  hipLaunchKernelGGL((near_gemv_t_kernel<R>), dim3(grid), dim3(kNearBlock), 0, st, wl, h->n_split, wl + h->n_split, h->n_wave_t, (const R*)h->K.p, (const R*)h->Wn.p, G);
  NEAR_TRY(hipGetLastError());
  return SCTL_AMD_OK;
}

// The transposed pass for `left` weight vectors still to do: near_pass_width's rule over the shipped forms, which are 2 and 4 in fp64 and 2 in fp32.
// Measured on the 2.8 GB operator: the fp32 form of 4 took 1.28 x the time of four single calls and is not built; a form of 8 does not
// fit 256 vector registers without scratch in either precision.
template <class R> constexpr int near_t_widest() { return sizeof(R) == 8 ? 4 : 2; }
template <class R> inline int near_t_pass_width(int left) { return left <= 2 ? 2 : near_t_widest<R>(); }

template <class R, int M>
int near_t_pass(sctl_amd_near* h, int nact, const R* W, R* G, hipStream_t st) {
  const int64_t n = h->ntrg * h->k1;
  hipLaunchKernelGGL((near_gather_multi_kernel<R, M>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->ntrg, h->k1, nact, (const int64_t*)h->scatter.p,
                     (const int64_t*)h->trg_cnt.p, (const int64_t*)h->trg_dsp.p, W, n, (R*)h->Wn_m.p, h->mt_cap);
  NEAR_TRY(hipGetLastError());
  const int64_t resident = (int64_t)h->cus * 8;
  const int64_t groups = h->n_split + (h->n_wave_t + kRowGroups - 1) / kRowGroups;
  const unsigned grid = (unsigned)(groups < resident * 4 ? groups : resident * 4);
  const NearWorkT* wl = (const NearWorkT*)h->work_t.p;
  hipLaunchKernelGGL((near_gemm_t_kernel<R, M>), dim3(grid), dim3(kNearBlock), 0, st, wl, h->n_split, wl + h->n_split, h->n_wave_t, (const R*)h->K.p,
                     (const R*)h->Wn_m.p, h->mt_cap, nact, G, h->f_len);
  NEAR_TRY(hipGetLastError());
  return SCTL_AMD_OK;
}

// nd >= 2 weight vectors, row-major: passes of the widest form, the last pass on the narrowest form that takes what is left; a single vector left over
// goes through the single-vector kernels.
template <class R>
int apply_transpose_densities_on_stream(sctl_amd_near* h, int nd, const R* W, R* G, hipStream_t st) {
  (void)hipGetLastError();
  if (h->n_split + h->n_wave_t == 0) return SCTL_AMD_OK;
  const int widest = near_t_pass_width<R>(nd);
  if (widest > h->mt_cap) {   // interleaved with the stride of the widest pass: an entry that the gather never writes (near_scatter_index no permutation) stays zero
    const size_t bytes = (size_t)widest * h->n_near * h->k1 * sizeof(R);
    h->mt_cap = 0;
    NEAR_TRY(h->Wn_m.realloc(bytes));
    NEAR_TRY(hipMemsetAsync(h->Wn_m.p, 0, bytes, st));
    h->mt_cap = widest;
  }
  const int64_t u_len = h->ntrg * h->k1;
  for (int m0 = 0; m0 < nd;) {
    const int left = nd - m0;
    const R* Wp = W + (int64_t)m0 * u_len;
    R* Gp = G + (int64_t)m0 * h->f_len;
    if (left == 1) return apply_transpose_on_stream<R>(h, Wp, Gp, st);
    const int M = near_t_pass_width<R>(left), nact = left < M ? left : M;
    const int rc = (M == 2) ? near_t_pass<R, 2>(h, nact, Wp, Gp, st) : near_t_pass<R, near_t_widest<R>()>(h, nact, Wp, Gp, st);
    if (rc) return rc;
    m0 += nact;
  }
  return SCTL_AMD_OK;
}

int check_apply_transpose(const sctl_amd_near* h, const void* W, const void* G) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if ((h->ntrg > 0 && !W) || (h->f_len > 0 && !G)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null weight or density-gradient array");
  return SCTL_AMD_OK;
}

int check_apply_transpose_densities(const sctl_amd_near* h, int nd, const void* W, const void* G) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of weight vectors");
  if (nd > 0 && ((h->ntrg > 0 && !W) || (h->f_len > 0 && !G))) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null weight or density-gradient array");
  return SCTL_AMD_OK;
}

int check_apply_densities(const sctl_amd_near* h, int nd, const void* F, const void* U) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  if (nd > 0 && ((h->f_len > 0 && !F) || (h->ntrg > 0 && !U))) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  return SCTL_AMD_OK;
}

}  // namespace

extern "C" {

int sctl_amd_near_create(int real, int device, int64_t Nelem, int src_dim, int trg_dim, const int64_t* elem_nds_cnt, const int64_t* near_elem_cnt,
                         const int64_t* K_near_cnt, const void* K_near, int64_t Ntrg, const int64_t* near_scatter_index, const int64_t* near_trg_cnt,
                         const int64_t* near_trg_dsp, sctl_amd_near** out) {
  if (!out) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null output handle");
  *out = nullptr;
  if (real != SCTL_AMD_F64 && real != SCTL_AMD_F32) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "real must be SCTL_AMD_F64 or SCTL_AMD_F32");
  if (Nelem < 0 || Ntrg < 0 || src_dim < 1 || trg_dim < 1) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative size or non-positive kernel dimension");
  if (Nelem > 0 && (!elem_nds_cnt || !near_elem_cnt)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null element count array");
  if (Ntrg > 0 && (!near_trg_cnt || !near_trg_dsp)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null target count array");

  // displacements (the reference's omp_par::scan, boundary_integral.txx:433,854) and the work list
  std::vector<NearWork> work, narrow;
  int64_t f_len = 0, n_near = 0, k_len = 0;
  for (int64_t e = 0; e < Nelem; e++) {
    const int64_t nds = elem_nds_cnt[e], nt = near_elem_cnt[e];
    if (nds < 0 || nt < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative element count");
    const int64_t kc = K_near_cnt ? K_near_cnt[e] : nds * nt;
    if (kc != 0 && kc != nds * nt) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "K_near_cnt[e] must be 0 or elem_nds_cnt[e] * near_elem_cnt[e] (boundary_integral.txx:1097)");
    const int64_t sd = nds * src_dim, td = nt * trg_dim;
    if (sd > INT32_MAX || td > INT32_MAX) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "operator block too large");
    if (kc != 0 && sd > 0 && td > 0) {
      const bool wide = td >= kNearBlock;   // a last wide chunk narrower than 64 columns would idle three waves: it goes narrow
      int64_t t0 = 0;
      for (; wide && t0 + kCols <= td && (td - t0 >= kNearBlock || (td - t0) > kNearBlock - kCols); t0 += kNearBlock)
        work.push_back(NearWork{k_len * src_dim * trg_dim, f_len, n_near * trg_dim, (int32_t)sd, (int32_t)td, (int32_t)t0, 1});
      for (; t0 < td; t0 += kCols) narrow.push_back(NearWork{k_len * src_dim * trg_dim, f_len, n_near * trg_dim, (int32_t)sd, (int32_t)td, (int32_t)t0, 0});
    }
    f_len += sd;
    n_near += nt;
    k_len += kc;
  }
  const int64_t n_wide = (int64_t)work.size(), n_narrow = (int64_t)narrow.size();
  work.insert(work.end(), narrow.begin(), narrow.end());
  if (k_len > 0 && !K_near) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null K_near");
  if (n_near > 0 && !near_scatter_index) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near_scatter_index");
  int64_t cnt_sum = 0;
  for (int64_t i = 0; i < Ntrg; i++) {
    if (near_trg_cnt[i] < 0 || near_trg_dsp[i] < 0 || near_trg_dsp[i] + near_trg_cnt[i] > n_near)
      return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "near_trg_dsp/cnt outside the near list");
    cnt_sum += near_trg_cnt[i];
  }
  if (cnt_sum != n_near) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "sum of near_trg_cnt differs from sum of near_elem_cnt");
  for (int64_t p = 0; p < n_near; p++)
    if (near_scatter_index[p] < 0 || near_scatter_index[p] >= n_near) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "near_scatter_index out of range");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) { (void)hipGetLastError(); ndev = 0; }
  if (ndev <= 0 || device < 0 || device >= ndev) return set_error(SCTL_AMD_ERR_NO_DEVICE, "no HIP device: libsctl_amd has no CPU fallback");

  const size_t rs = real_size(real);
  std::unique_ptr<sctl_amd_near> h(new sctl_amd_near);
  h->real = real; h->device = device; h->k0 = src_dim; h->k1 = trg_dim;
  h->nelem = Nelem; h->ntrg = Ntrg; h->n_near = n_near; h->f_len = f_len; h->k_len = k_len * src_dim * trg_dim; h->nwork = (int64_t)work.size(); h->n_wide = n_wide; h->n_narrow = n_narrow;
  if (Nelem > 0) {
    h->e_nds.assign(elem_nds_cnt, elem_nds_cnt + Nelem);
    h->e_near.assign(near_elem_cnt, near_elem_cnt + Nelem);
    h->e_kcnt.resize((size_t)Nelem);
    for (int64_t e = 0; e < Nelem; e++) h->e_kcnt[(size_t)e] = K_near_cnt ? K_near_cnt[e] : elem_nds_cnt[e] * near_elem_cnt[e];
  }
  DeviceScope dev_scope_1(device);
  NEAR_TRY(dev_scope_1.err);
  NEAR_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
  { int n = 0; if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) h->cus = n; }
  NEAR_TRY(h->K.alloc((size_t)h->k_len * rs));
  NEAR_TRY(h->work.alloc(work.size() * sizeof(NearWork)));
  NEAR_TRY(h->scatter.alloc((size_t)n_near * 8));
  NEAR_TRY(h->trg_cnt.alloc((size_t)Ntrg * 8));
  NEAR_TRY(h->trg_dsp.alloc((size_t)Ntrg * 8));
  NEAR_TRY(h->F.alloc((size_t)f_len * rs));
  NEAR_TRY(h->U_near.alloc((size_t)n_near * trg_dim * rs));
  NEAR_TRY(h->U.alloc((size_t)Ntrg * trg_dim * rs));
  NEAR_TRY(h->stage.alloc(((size_t)f_len + (size_t)Ntrg * trg_dim) * rs + 512));
  // one-time uploads: synchronous copies from the caller's arrays (read once, never rewritten in place by this library)
  if (h->k_len) NEAR_TRY(hipMemcpy(h->K.p, K_near, (size_t)h->k_len * rs, hipMemcpyHostToDevice));
  if (!work.empty()) NEAR_TRY(hipMemcpy(h->work.p, work.data(), work.size() * sizeof(NearWork), hipMemcpyHostToDevice));
  if (n_near) NEAR_TRY(hipMemcpy(h->scatter.p, near_scatter_index, (size_t)n_near * 8, hipMemcpyHostToDevice));
  if (Ntrg) {
    NEAR_TRY(hipMemcpy(h->trg_cnt.p, near_trg_cnt, (size_t)Ntrg * 8, hipMemcpyHostToDevice));
    NEAR_TRY(hipMemcpy(h->trg_dsp.p, near_trg_dsp, (size_t)Ntrg * 8, hipMemcpyHostToDevice));
  }
  NEAR_TRY(hipMemset(h->U_near.p, 0, (size_t)n_near * trg_dim * rs));   // runs of matrix-free elements stay zero (:1096)
  *out = h.release();
  return SCTL_AMD_OK;
}

int sctl_amd_near_apply_device(sctl_amd_near* h, const void* F, void* U, void* stream) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if ((h->f_len > 0 && !F) || (h->ntrg > 0 && !U)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  return with_real(h->real, [&](auto zero) { using R = decltype(zero); return apply_on_stream<R>(h, (const R*)F, (R*)U, (hipStream_t)stream); });
}

int sctl_amd_near_apply_host(sctl_amd_near* h, const void* F, void* U) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if ((h->f_len > 0 && !F) || (h->ntrg > 0 && !U)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  if (h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(h->real);
  const size_t bf = (size_t)h->f_len * rs, bu = (size_t)h->ntrg * h->k1 * rs;
  DeviceScope dev_scope_2(h->device);
  NEAR_TRY(dev_scope_2.err);
  char* sf = (char*)h->stage.p;
  char* su = sf + ((bf + 255) & ~(size_t)255);
  std::memcpy(sf, F, bf);                                  // pinned staging: see staging.hpp PinnedBufT
  NEAR_TRY(hipMemcpyAsync(h->F.p, sf, bf, hipMemcpyHostToDevice, h->st));
  NEAR_TRY(hipMemsetAsync(h->U.p, 0, bu, h->st));
  const int rc = sctl_amd_near_apply_device(h, h->F.p, h->U.p, h->st);
  if (rc != SCTL_AMD_OK) return rc;
  NEAR_TRY(hipMemcpyAsync(su, h->U.p, bu, hipMemcpyDeviceToHost, h->st));
  NEAR_TRY(hipStreamSynchronize(h->st));
  add_into(h->real, U, su, h->ntrg * h->k1);                       // U += near field (boundary_integral.txx:1131-1140)
  return SCTL_AMD_OK;
}

int sctl_amd_near_apply_densities_device(sctl_amd_near* h, int nd, const void* F, void* U, void* stream) {
  const int rc = check_apply_densities(h, nd, F, U);
  if (rc || nd == 0) return rc;
  if (nd == 1) return sctl_amd_near_apply_device(h, F, U, stream);
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  return with_real(h->real, [&](auto zero) { using R = decltype(zero); return apply_densities_on_stream<R>(h, nd, (const R*)F, (R*)U, (hipStream_t)stream); });
}

int sctl_amd_near_apply_densities_host(sctl_amd_near* h, int nd, const void* F, void* U) {
  const int rc0 = check_apply_densities(h, nd, F, U);
  if (rc0 || nd == 0) return rc0;
  if (nd == 1) return sctl_amd_near_apply_host(h, F, U);
  if (h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(h->real);
  const size_t bf = (size_t)nd * h->f_len * rs, bu = (size_t)nd * h->ntrg * h->k1 * rs;
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  if (nd > h->nd_cap) {
    h->nd_cap = 0;
    NEAR_TRY(h->F_m.realloc(bf));
    NEAR_TRY(h->U_m.realloc(bu));
    NEAR_TRY(h->stage_m.realloc(bf + bu + 512));
    h->nd_cap = nd;
  }
  char* sf = (char*)h->stage_m.p;
  char* su = sf + ((bf + 255) & ~(size_t)255);
  std::memcpy(sf, F, bf);
  NEAR_TRY(hipMemcpyAsync(h->F_m.p, sf, bf, hipMemcpyHostToDevice, h->st));
  NEAR_TRY(hipMemsetAsync(h->U_m.p, 0, bu, h->st));
  const int rc = sctl_amd_near_apply_densities_device(h, nd, h->F_m.p, h->U_m.p, h->st);
  if (rc != SCTL_AMD_OK) return rc;
  NEAR_TRY(hipMemcpyAsync(su, h->U_m.p, bu, hipMemcpyDeviceToHost, h->st));
  NEAR_TRY(hipStreamSynchronize(h->st));
  add_into(h->real, U, su, (int64_t)nd * h->ntrg * h->k1);         // every row: U += near field
  return SCTL_AMD_OK;
}

int sctl_amd_near_apply_transpose_device(sctl_amd_near* h, const void* W, void* G, void* stream) {
  const int rc0 = check_apply_transpose(h, W, G);
  if (rc0) return rc0;
  if (h->k_len == 0 || h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  const int rc = prepare_transpose(h, (hipStream_t)stream);
  if (rc) return rc;
  return with_real(h->real, [&](auto zero) { using R = decltype(zero); return apply_transpose_on_stream<R>(h, (const R*)W, (R*)G, (hipStream_t)stream); });
}

int sctl_amd_near_apply_transpose_host(sctl_amd_near* h, const void* W, void* G) {
  const int rc0 = check_apply_transpose(h, W, G);
  if (rc0) return rc0;
  if (h->k_len == 0 || h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(h->real);
  const size_t bf = (size_t)h->f_len * rs, bu = (size_t)h->ntrg * h->k1 * rs;
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  char* sf = (char*)h->stage.p;                            // the staging and the device arrays of the forward host entry, roles swapped
  char* su = sf + ((bf + 255) & ~(size_t)255);
  std::memcpy(su, W, bu);
  NEAR_TRY(hipMemcpyAsync(h->U.p, su, bu, hipMemcpyHostToDevice, h->st));
  NEAR_TRY(hipMemsetAsync(h->F.p, 0, bf, h->st));
  const int rc = sctl_amd_near_apply_transpose_device(h, h->U.p, h->F.p, h->st);
  if (rc != SCTL_AMD_OK) return rc;
  NEAR_TRY(hipMemcpyAsync(sf, h->F.p, bf, hipMemcpyDeviceToHost, h->st));
  NEAR_TRY(hipStreamSynchronize(h->st));
  // G += N^T W over the entries some block owns; the entries of elements without a matrix or without near targets keep their bits (a -0.0 too)
  int64_t f_off = 0;
  for (int64_t e = 0; e < h->nelem; e++) {
    const int64_t sd = h->e_nds[(size_t)e] * h->k0;
    if (h->e_kcnt[(size_t)e] != 0 && h->e_near[(size_t)e] > 0) {
      add_into(h->real, (char*)G + (size_t)f_off * rs, sf + (size_t)f_off * rs, sd);
    }
    f_off += sd;
  }
  return SCTL_AMD_OK;
}

// nd == 1 goes through the single-vector entry (bit-identical results); nd == 0 is a no-op after the argument checks.
int sctl_amd_near_apply_transpose_densities_device(sctl_amd_near* h, int nd, const void* W, void* G, void* stream) {
  const int rc0 = check_apply_transpose_densities(h, nd, W, G);
  if (rc0 || nd == 0) return rc0;
  if (nd == 1) return sctl_amd_near_apply_transpose_device(h, W, G, stream);
  if (h->k_len == 0 || h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  const int rc = prepare_transpose(h, (hipStream_t)stream);
  if (rc) return rc;
  return with_real(h->real, [&](auto zero) { using R = decltype(zero); return apply_transpose_densities_on_stream<R>(h, nd, (const R*)W, (R*)G, (hipStream_t)stream); });
}

int sctl_amd_near_apply_transpose_densities_host(sctl_amd_near* h, int nd, const void* W, void* G) {
  const int rc0 = check_apply_transpose_densities(h, nd, W, G);
  if (rc0 || nd == 0) return rc0;
  if (nd == 1) return sctl_amd_near_apply_transpose_host(h, W, G);
  if (h->k_len == 0 || h->n_near == 0 || h->ntrg == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(h->real);
  const size_t bf = (size_t)nd * h->f_len * rs, bu = (size_t)nd * h->ntrg * h->k1 * rs;
  DeviceScope dev_scope(h->device);
  NEAR_TRY(dev_scope.err);
  if (nd > h->nd_cap) {   // the staging and the device arrays of the forward several-densities host entry, roles swapped
    h->nd_cap = 0;
    NEAR_TRY(h->F_m.realloc(bf));
    NEAR_TRY(h->U_m.realloc(bu));
    NEAR_TRY(h->stage_m.realloc(bf + bu + 512));
    h->nd_cap = nd;
  }
  char* sf = (char*)h->stage_m.p;
  char* su = sf + ((bf + 255) & ~(size_t)255);
  std::memcpy(su, W, bu);
  NEAR_TRY(hipMemcpyAsync(h->U_m.p, su, bu, hipMemcpyHostToDevice, h->st));
  NEAR_TRY(hipMemsetAsync(h->F_m.p, 0, bf, h->st));
  const int rc = sctl_amd_near_apply_transpose_densities_device(h, nd, h->U_m.p, h->F_m.p, h->st);
  if (rc != SCTL_AMD_OK) return rc;
  NEAR_TRY(hipMemcpyAsync(sf, h->F_m.p, bf, hipMemcpyDeviceToHost, h->st));
  NEAR_TRY(hipStreamSynchronize(h->st));
  // every row: G += N^T W over the entries some block owns; the others keep their bits
  for (int m = 0; m < nd; m++) {
    int64_t f_off = (int64_t)m * h->f_len;
    for (int64_t e = 0; e < h->nelem; e++) {
      const int64_t sd = h->e_nds[(size_t)e] * h->k0;
      if (h->e_kcnt[(size_t)e] != 0 && h->e_near[(size_t)e] > 0) add_into(h->real, (char*)G + (size_t)f_off * rs, sf + (size_t)f_off * rs, sd);
      f_off += sd;
    }
  }
  return SCTL_AMD_OK;
}

int sctl_amd_near_info(const sctl_amd_near* h, int64_t* density_len, int64_t* potential_len, int64_t* near_entries, int64_t* operator_bytes,
                       int64_t* workgroups) {
  if (!h) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field handle");
  if (density_len) *density_len = h->f_len;
  if (potential_len) *potential_len = h->ntrg * h->k1;
  if (near_entries) *near_entries = h->n_near;
  if (operator_bytes) *operator_bytes = h->k_len * (int64_t)real_size(h->real);
  if (workgroups) *workgroups = h->nwork;
  return SCTL_AMD_OK;
}

void sctl_amd_near_destroy(sctl_amd_near* h) {
  if (!h) return;
  DeviceScope scope(h->device);
  delete h;
}

}  // extern "C"
