// Several rows over the P2P lists in one launch, both directions from ONE body:
//   forward     (lists_multi_kernel)            v[m][t,k1] += scale * sum_{l : t in target range l} sum_{s in source range l} sum_k0 U(x_t - x_s, n_s)[k0][k1] * f[m][s,k0]
//   transposed  (lists_multi_transpose_kernel)  g[m][s,k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t,k1]
// for m = 0 .. nd-1.  These are the list evaluators of include/sctl_amd/device/lists_kernel.hpp and lists_transpose_kernel.hpp with M rows (densities, weight
// vectors) per streamed record (ukernels.hpp: NREC_M / pack_m / pair_m and NREC_TM / pack_tm / pair_tm).  What a pair costs that does not depend on the row — and
// here also what a STREAMED point costs: its index, the gather of its coordinates, its place in the tile — is paid once for M rows.
//
// Same scheme as the single-row kernels: one wave64 per work item, XCD-owned shares (xcd_first), every OWNER point (a target forward, a source transposed) held by
// one lane, sums kept in registers in list order and written once, speculative unmasked tiles / steps with repair, the known_coincident shortcut of the packed
// items; no atomics, no workspace, deterministic.  The PLAN is the single-row plan of that direction: the kernel walks the same ListItem / ListRange / PackedGroup /
// flat-index arrays, all seven item shapes.  What differs from the single-row kernels:
//   * records are NREC<M> reals (pack), the pair adds into acc[M][KOUT]: a lane holds T x M x KOUT sums and as many per-tile sums;
//   * rows are row-major: row m of streamed point q is in[m * in_stride + q * KIN + k], its result for owner o is out[m * out_stride + o * KOUT + k];
//   * the last pass of a call may use fewer rows than the form's M (nact): the others are packed as 0 and never stored;
//   * an item the plan cut for two owners per lane (128 owners, packed classes 1 - 3) runs its owners in TWO HALVES over the same streamed sequence where the
//     registers do not hold two owners at width M (ListRowsForm::TWO): the item is not shrunk;
//   * where the packed tile of 128 records would cost the second wave per SIMD, the packed groups take one streamed point per lane and step instead of two
//     (ListRowsForm::SPL2): a tile of 64 records, as the one-range items use.
// fp32 runs this exact vector-pipe pair at every accuracy, as eval_multi_kernel and every transposed kernel do.
//
// The two directions differ only in the policy `Dir` (ListFwd, ListTrans below): which of K0 / K1 is the output width, the record, who carries the normal, the
// sign of d (rows_dir.hpp), and the names of the fields of ListArgs / ListTArgs (device/dir.hpp).  Everything else — the walker, the form, the dispatch, the launch table — exists once.
#pragma once
#include <sctl_amd/device/launch.hpp>
#include <sctl_amd/device/lists_kernel.hpp>
#include <sctl_amd/device/lists_transpose_kernel.hpp>
#include "rows_dir.hpp"

namespace sctl_amd {

// L: ListArgs<R> (forward) or ListTArgs<R> (transposed)
template <class L> struct ListRowsArgs {
  L l;                  // its input row (f / w) is row 0 of this pass, its output (v_trg / g_src) that row's result
  int64_t in_stride;    // input row m at + m * in_stride
  int64_t out_stride;   // its result at + m * out_stride, accumulated into
  int nact;             // rows in use, 1 <= nact <= M
};
template <class R> using ListMultiArgs = ListRowsArgs<ListArgs<R>>;
template <class R> using ListMultiTArgs = ListRowsArgs<ListTArgs<R>>;

// Everything about the direction is RowsFwd / RowsTrans of rows_dir.hpp, shared with the all-pairs kernels: the M-row record, pack and pair, and — inherited from
// the single-row policies of device/dir.hpp — the widths, the finish hook and the fields of ListArgs / ListTArgs.  Added here: the side and the argument type.
struct ListFwd : RowsFwd {            // the owners are the targets
  static constexpr int SIDE = 0;      // of sctl_amd_lists::side
  template <class R> using Args = ListMultiArgs<R>;
};
struct ListTrans : RowsTrans {        // the owners are the sources, each with its normal
  static constexpr int SIDE = 1;
  template <class R> using Args = ListMultiTArgs<R>;
};

// A workgroup is ONE wave: two waves per SIMD are eight workgroups per CU, so a form may use an eighth of the CU's 160 KB of LDS.
constexpr int kListRowsLdsBudget = 160 * 1024 / 8;

// Shape of the (direction, kernel, precision, M) form.  SPL2 / FITS follow from the LDS bytes alone; TWO is an estimate of the live registers (per owner:
// coordinates, normal, sums and per-tile sums; the record; the streamed points fetched ahead with their normal and M rows; in 32-bit registers, + 40 for
// addresses, constants and bookkeeping) against the 256 a wave may have at two waves per SIMD.  The launch tables (lmulti_*.hip, ltmulti_*.hip) name the
// widths that are built; what the compiler made of every one of them is in DESIGN.md §4.6 and §4.15 and held to ScratchSize 0 by
// tests/test_lists_densities_cpu.py and tests/test_lists_transpose_densities_cpu.py.
template <class Dir, class Ker, class R, int M> struct ListRowsForm {
  static constexpr int VN = VecOf<R>::N;
  static constexpr int NV = (Dir::template NREC<Ker, M> + VN - 1) / VN;
  static constexpr int SCRATCH = Ker::template Consts<R>::LDS_DOUBLES > 0 ? Ker::template Consts<R>::LDS_DOUBLES : 1;
  static constexpr bool SPL2 = kPackedTileWords(NV) * 16 + SCRATCH * 8 <= kListRowsLdsBudget;
  static constexpr int TILE_WORDS = SPL2 ? kPackedTileWords(NV) : kListTile * NV + 8;   // 8 groups x (8 or 16 records + 1 word)
  static constexpr bool FITS = TILE_WORDS * 16 + SCRATCH * 8 <= kListRowsLdsBudget;
  static constexpr int regs(int t, int spl) {
    return (int)(sizeof(R) / 4) * (t * (3 + Dir::template OWN_N<Ker> + 2 * M * Dir::template KOUT<Ker>) + NV * VN +
                                   spl * (3 + Dir::template STR_N<Ker> + M * Dir::template KIN<Ker>)) + 40;
  }
  static constexpr bool TWO = regs(2, SPL2 ? 2 : 1) <= 252;   // (256 by the estimate spilt: forward Stokes3D_DxU fp64, 4 densities)
};

// lists_item of the single-row kernels for M rows.  T owners per lane are held; slot j of the lane is owner (j0 + j) * 64 + lane of the item
// (j0 = 1: the second half of a 128-owner item run in halves).
template <class Dir, class Ker, class R, int MODE, int M, int T, bool SPLIT, class A, class KC, class V>
__device__ __forceinline__ void lists_rows_item(const A& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  static_assert(!SPLIT || T == 1, "replicas are for small one-owner-per-lane items");
  constexpr int KIN = Dir::template KIN<Ker>, KOUT = Dir::template KOUT<Ker>, ND = Ker::ND, NREC = Dir::template NREC<Ker, M>;
  constexpr int OWN_N = Dir::template OWN_N<Ker>, STR_N = Dir::template STR_N<Ker>, NN = OWN_N ? OWN_N : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  const int lane = threadIdx.x;
  const ListRange* const rg = a.l.ranges + it.first_range;

  int P = kListWave;                       // lanes per replica
  if (SPLIT) { P = 8; while (P < it.nt) P <<= 1; }
  const int nrep = kListWave / P, rep = lane / P;

  R xo[T][3], no[T][NN], acc[T][M][KOUT];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int ol = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    if (ol >= it.nt) ol = it.nt - 1;      // idle lanes repeat the last owner; never stored
    const int64_t oi = it.t0 + ol;
#pragma unroll
    for (int k = 0; k < 3; k++) xo[j][k] = Dir::own_x(a.l)[oi * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) no[j][k] = OWN_N ? Dir::own_n(a.l)[oi * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < KOUT; k++) acc[j][m][k] = 0;
  }

  // cursor into the concatenated streamed sequence (wave-uniform): range r, offset o inside it
  int r = 0;
  int64_t o = 0;
  R sx[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sr[M][KIN];
#pragma unroll
  for (int m = 0; m < M; m++)
#pragma unroll
    for (int k = 0; k < KIN; k++) sr[m][k] = 0;
  // fetch the next (up to) 64 points of the sequence into registers, lane i the i-th of them, with their M rows; returns how many
  auto fetch = [&]() -> int {
    int fill = 0;
    int64_t mine = -1;
    while (fill < kListTile && r < it.nranges) {
      const int64_t left = rg[r].ns - o;
      const int take = (left < (int64_t)(kListTile - fill)) ? (int)left : (kListTile - fill);
      if (lane >= fill && lane < fill + take) mine = rg[r].s0 + o + (lane - fill);
      fill += take;
      o += take;
      if (o >= rg[r].ns) { r++; o = 0; }
    }
    if (mine >= 0) {
#pragma unroll
      for (int k = 0; k < 3; k++) sx[k] = Dir::str_x(a.l)[mine * 3 + k];
#pragma unroll
      for (int k = 0; k < STR_N; k++) sn[k] = Dir::str_n(a.l)[mine * STR_N + k];
#pragma unroll
      for (int m = 0; m < M; m++) {
        if (m < a.nact) {                  // (wave-uniform; the rows past nact stay 0)
          const R* const pr = Dir::in(a.l) + m * a.in_stride + mine * KIN;
#pragma unroll
          for (int k = 0; k < KIN; k++) sr[m][k] = pr[k];
        }
      }
    }
    return fill;
  };

  int repairs = 0, tiles = 0;
  bool always_masked = false;
  int ns = fetch();
  while (ns > 0) {
    __syncthreads();   // previous tile fully consumed
    if (lane < ns) {
      R rec[NRECP] = {};
      Dir::template pack<Ker, R, M>(rec, sx, sn, sr);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V w;
#pragma unroll
        for (int e = 0; e < VN; e++) w[e] = rec[v * VN + e];
        tile[lane * NV + v] = w;
      }
    }
    const int ns_cur = ns;
    ns = fetch();      // loads for the next tile are in flight during this tile's arithmetic
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
        for (int j = 0; j < T; j++) Dir::template pair<Ker, R, MODE, MASKED, M, VARIANT>(tacc[j], xo[j], no[j], rec, a.l.ctx, K);
      };
      if (SPLIT) {                         // replica `rep` takes points rep, rep + nrep, ... of the tile
        const int cnt = (ns_cur + nrep - 1) / nrep;   // wave-uniform trip count; the tail of a short tile is predicated
        for (int i = 0; i < cnt; i++) {
          const int s = i * nrep + rep;
          if (s < ns_cur) one_point(s);
        }
      } else if (ns_cur == kListTile) {
#pragma unroll UnrollOf<T, M * KOUT>::value
        for (int s = 0; s < kListTile; s++) one_point(s);
      } else {
        for (int s = 0; s < ns_cur; s++) one_point(s);
      }
    };
    auto run_tile = [&](auto masked_tag) {   // (one-wave work items: the small tables, variants 0 / 1 only, as in the single-row kernels)
      if constexpr (KC::HAS_VARIANT) {
        if (K.variant(a.l.ctx) & 1) run_tile_v(masked_tag, std::integral_constant<int, 1>());
        else run_tile_v(masked_tag, std::integral_constant<int, 0>());
      } else {
        run_tile_v(masked_tag, std::integral_constant<int, 0>());
      }
    };
    bool repaired = true;
    tiles++;
    if (!always_masked) {
      run_tile(std::false_type());
      bool bad = K.tile_bad(a.l.ctx);
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < KOUT; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 4 > tiles + 4) always_masked = true;   // mostly coincident points (tiny boxes): stop speculating
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < KOUT; k++) acc[j][m][k] += tacc[j][m][k];
  }

  if (SPLIT) {                             // add the replicas' sums: lanes l, l ^ P, l ^ 2P, ... hold the same owner
    for (int off = P; off < kListWave; off <<= 1)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < KOUT; k++) acc[0][m][k] += __shfl_xor(acc[0][m][k], off);
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int ol = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    const bool store = ol < it.nt && (!SPLIT || rep == 0);
    const int64_t oi = it.t0 + (store ? ol : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      Dir::template finish<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const v = Dir::out(a.l) + m * a.out_stride + oi * KOUT;
#pragma unroll
        for (int k = 0; k < KOUT; k++) v[k] += acc[j][m][k] * a.l.scale;   // generic-kernel.txx:184
      }
    }
  }
}

// lists_packed_item of the single-row kernels for M rows.  T owners per lane are held; slot j of a lane is owner (j0 + j) * P + i of its
// group (j0 = 1: the second half of a two-owners-per-lane class run in halves; a wave whose groups all fit the first half skips it).
template <class Dir, class Ker, class R, int MODE, int M, int P, int T, int SPL, class A, class KC, class V>
__device__ __forceinline__ void lists_rows_packed_item(const A& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  constexpr int KIN = Dir::template KIN<Ker>, KOUT = Dir::template KOUT<Ker>, ND = Ker::ND, NREC = Dir::template NREC<Ker, M>;
  constexpr int OWN_N = Dir::template OWN_N<Ker>, STR_N = Dir::template STR_N<Ker>, NN = OWN_N ? OWN_N : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  constexpr int G = kListWave / P, S = P * SPL, SLICE = S * NV + 1;   // S points per group and step (SPL per lane); 16-byte words per group slice (+ 1: bank spread)
  static_assert(G * SLICE <= ListRowsForm<Dir, Ker, R, M>::TILE_WORDS, "the packed slices fit the form's LDS tile");
  const int lane = threadIdx.x, g = lane / P, i = lane % P;
  const bool live = g < it.nt;                              // (it.nt = groups of this item)
  const PackedGroup pg = a.l.groups[it.t0 + (live ? g : 0)];
  if (j0 > 0 && !__any(live && pg.nt > j0 * P)) return;    // wave-uniform: no group of this wave reaches into the second half
  const int nstr = live ? pg.nsrc : 0;                      // streamed points of the group
  const bool self = (const void*)a.l.xs == (const void*)a.l.xt;

  R xo[T][3], no[T][NN], acc[T][M][KOUT];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int ol = (j0 + j) * P + i;
    if (ol >= pg.nt) ol = pg.nt - 1;                        // idle slots repeat the last owner; never stored
    const int64_t oi = pg.t0 + ol;
#pragma unroll
    for (int k = 0; k < 3; k++) xo[j][k] = Dir::own_x(a.l)[oi * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) no[j][k] = OWN_N ? Dir::own_n(a.l)[oi * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < KOUT; k++) acc[j][m][k] = 0;
  }
  int nmax = nstr;                                          // the longest sequence of the wave decides the trip count
  for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(nmax, o); nmax = (w > nmax) ? w : nmax; }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  const int nsteps = (nmax + S - 1) / S;

  R sx[SPL][3], sn[SPL][3], sr[SPL][M][KIN];
#pragma unroll
  for (int u = 0; u < SPL; u++) {
#pragma unroll
    for (int k = 0; k < 3; k++) { sx[u][k] = 0; sn[u][k] = 0; }
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < KIN; k++) sr[u][m][k] = 0;
  }
  // Points one step ahead, their indices two steps ahead, 32-bit byte offsets from scalar bases: as in the single-row packed items.  The M rows are M scalar
  // bases (in + m * in_stride) with the same lane offset.
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t own_lo = (uint32_t)pg.t0, own_n = self ? (uint32_t)pg.nt : 0u;   // (own points exist only when the sources ARE the targets)
  const uint32_t* const flat_g = a.l.flat + pg.flat_off;
  bool own = false;    // a point this lane holds for the coming step is one of its group's owners
  uint32_t idx_next[SPL];
  auto load_idx = [&](int step) {
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      const int q = step * S + u * P + i;
      idx_next[u] = (q < nstr) ? flat_g[q] : kNone;
    }
  };
  if (nsteps > 0) load_idx(0);
  auto at = [](const R* base, uint32_t byte_off) -> const R* { return (const R*)((const char*)base + byte_off); };
  auto fetch = [&](int step) {
    uint32_t str[SPL];
#pragma unroll
    for (int u = 0; u < SPL; u++) str[u] = idx_next[u];
    if (step + 1 < nsteps) load_idx(step + 1);
    own = false;
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (str[u] != kNone) {
        own = own || (str[u] - own_lo < own_n);
        const R* const px = at(Dir::str_x(a.l), str[u] * (uint32_t)(3 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < 3; k++) sx[u][k] = px[k];
        if (STR_N > 0) {
          const R* const pn = at(Dir::str_n(a.l), str[u] * (uint32_t)(STR_N * sizeof(R)));
#pragma unroll
          for (int k = 0; k < STR_N; k++) sn[u][k] = pn[k];
        }
#pragma unroll
        for (int m = 0; m < M; m++) {
          if (m < a.nact) {                                 // (wave-uniform; the rows past nact stay 0)
            const R* const pr = at(Dir::in(a.l) + m * a.in_stride, str[u] * (uint32_t)(KIN * sizeof(R)));
#pragma unroll
            for (int k = 0; k < KIN; k++) sr[u][m][k] = pr[k];
          }
        }
      }
    }
  };
  V* const slice = tile + g * SLICE;
  if (nsteps > 0) fetch(0);
  for (int step = 0; step < nsteps; step++) {
    __syncthreads();   // previous slices fully consumed
    const int cnt = nstr - step * S;                        // points of this group in this step: >= S (full), 1 .. S - 1 (its last), <= 0 (done)
    const bool known_coincident = __any(own);               // (of the step being staged now: `own` belongs to the points fetched for it)
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (u * P + i < cnt) {
        R rec[NRECP] = {};
        Dir::template pack<Ker, R, M>(rec, sx[u], sn[u], sr[u]);
#pragma unroll
        for (int v = 0; v < NV; v++) {
          V w;
#pragma unroll
          for (int e = 0; e < VN; e++) w[e] = rec[v * VN + e];
          slice[(u * P + i) * NV + v] = w;
        }
      }
    }
    if (step + 1 < nsteps) fetch(step + 1);
    __syncthreads();

    R tacc[T][M][KOUT];
    const bool full = __all(cnt >= S);                      // wave-uniform: every group has a whole slice (all steps but the groups' last ones)
    auto run_step_v = [&](auto masked_tag, auto variant_tag) {
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
          const V w = slice[s * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = w[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) Dir::template pair<Ker, R, MODE, MASKED, M, VARIANT>(tacc[j], xo[j], no[j], rec, a.l.ctx, K);
      };
      if (full) {
#pragma unroll UnrollOf<T, M * KOUT>::value
        for (int s = 0; s < S; s++) one_point(s);
      } else {                                              // a group's last step: its remaining points, the other groups' lanes idle
        int cmax = cnt;
        for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(cmax, o); cmax = (w > cmax) ? w : cmax; }
        cmax = __builtin_amdgcn_readfirstlane(cmax < S ? cmax : S);
        for (int s = 0; s < cmax; s++)
          if (s < cnt) one_point(s);
      }
    };
    auto run_step = [&](auto masked_tag) {
      if constexpr (KC::HAS_VARIANT) {
        if (K.variant(a.l.ctx) & 1) run_step_v(masked_tag, std::integral_constant<int, 1>());
        else run_step_v(masked_tag, std::integral_constant<int, 0>());
      } else {
        run_step_v(masked_tag, std::integral_constant<int, 0>());
      }
    };
    bool repaired = true;
    if (!known_coincident) {
      run_step(std::false_type());
      bool bad = K.tile_bad(a.l.ctx);
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int m = 0; m < M; m++)
#pragma unroll
          for (int k = 0; k < KOUT; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);
    }
    if (repaired) run_step(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < KOUT; k++) acc[j][m][k] += tacc[j][m][k];
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int ol = (j0 + j) * P + i;
    const bool store = live && ol < pg.nt;
    const int64_t oi = pg.t0 + (store ? ol : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      Dir::template finish<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const v = Dir::out(a.l) + m * a.out_stride + oi * KOUT;
#pragma unroll
        for (int k = 0; k < KOUT; k++) v[k] += acc[j][m][k] * a.l.scale;   // generic-kernel.txx:184
      }
    }
  }
}

// The dispatch of the single-row kernels over the plan's seven item shapes.  An item cut for two owners per lane holds both (TWO) or runs twice.
template <class Dir, class Ker, class R, int MODE, int M, class A> __device__ __forceinline__ void lists_rows_dispatch(const A& a) {
  using V = typename VecOf<R>::type;
  using F = ListRowsForm<Dir, Ker, R, M>;
  static_assert(F::FITS, "this form's LDS tile leaves less than two waves per SIMD: it is not built (lmulti_*.hip, ltmulti_*.hip)");
  constexpr bool TWO = F::TWO;
  constexpr int SPL = F::SPL2 ? 2 : 1;
  __shared__ V tile[F::TILE_WORDS];
  using KC = typename Ker::template Consts<R>;
  __shared__ double kscratch[F::SCRATCH];
  const KC K = make_consts<KC>(kscratch, a.l.ctx, MODE);
  const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;      // XCD x walks its share of the item list (as the single-row kernels do)
  if (j >= a.l.xcd_first[xcd + 1] - a.l.xcd_first[xcd]) return;
  const ListItem it = a.l.items[a.l.xcd_first[xcd] + j];
  if (it.nranges < 0) {      // packed small owner ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) {
      lists_rows_packed_item<Dir, Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, 0);
    } else if (cls == 1) {
      if constexpr (TWO) lists_rows_packed_item<Dir, Ker, R, MODE, M, 8, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_rows_packed_item<Dir, Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, h);
      }
    } else if (cls == 2) {
      if constexpr (TWO) lists_rows_packed_item<Dir, Ker, R, MODE, M, 16, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_rows_packed_item<Dir, Ker, R, MODE, M, 16, 1, SPL>(a, it, tile, K, h);
      }
    } else {
      if constexpr (TWO) lists_rows_packed_item<Dir, Ker, R, MODE, M, 32, 2, 1>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_rows_packed_item<Dir, Ker, R, MODE, M, 32, 1, 1>(a, it, tile, K, h);
      }
    }
    return;
  }
  if (it.nt > kListWave) {
    if constexpr (TWO) lists_rows_item<Dir, Ker, R, MODE, M, 2, false>(a, it, tile, K, 0);
    else {
#pragma unroll 1
      for (int h = 0; h < 2; h++) lists_rows_item<Dir, Ker, R, MODE, M, 1, false>(a, it, tile, K, h);
    }
  } else if (it.nt > kListWave / 2) {
    lists_rows_item<Dir, Ker, R, MODE, M, 1, false>(a, it, tile, K, 0);
  } else {
    lists_rows_item<Dir, Ker, R, MODE, M, 1, true>(a, it, tile, K, 0);
  }
}

template <class Ker, class R, int MODE, int M> __global__ void __launch_bounds__(kListWave, 2) lists_multi_kernel(const ListMultiArgs<R> a) {
  lists_rows_dispatch<ListFwd, Ker, R, MODE, M>(a);
}
template <class Ker, class R, int MODE, int M> __global__ void __launch_bounds__(kListWave, 2) lists_multi_transpose_kernel(const ListMultiTArgs<R> a) {
  lists_rows_dispatch<ListTrans, Ker, R, MODE, M>(a);
}

// ---- launch table: one per direction and built-in kernel (lmulti_<Kernel>.hip, ltmulti_<Kernel>.hip), none for plugin kernels ----------
constexpr int kNumListRowsM = 3;                     // forms of 2, 4 and 8 rows
constexpr int kListRowsM[kNumListRowsM] = {2, 4, 8};
template <class Dir, class R> using ListsRowsLaunch = void (*)(const typename Dir::template Args<R>&, int64_t nblocks, hipStream_t);
template <class Dir> struct ListsRowsEntry {
  ListsRowsLaunch<Dir, double> f64[kNumMode][kNumListRowsM];   // null: no such form
  ListsRowsLaunch<Dir, float> f32[kNumMode][kNumListRowsM];    // modes 0 and 1 (mode 2 aliases 1)
};
using ListsMultiEntry = ListsRowsEntry<ListFwd>;
using ListsMultiTEntry = ListsRowsEntry<ListTrans>;

template <class Dir, class Ker, class R, int MODE, int M> void launch_lists_rows(const typename Dir::template Args<R>& a, int64_t nblocks, hipStream_t st) {
  if constexpr (Dir::SIDE == 0) hipLaunchKernelGGL((lists_multi_kernel<Ker, R, MODE, M>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
  else hipLaunchKernelGGL((lists_multi_transpose_kernel<Ker, R, MODE, M>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}
template <class Dir, class Ker, int M, bool D, bool F> void fill_lists_rows(ListsRowsEntry<Dir>& e, int i) {
  if constexpr (D) {
    e.f64[0][i] = launch_lists_rows<Dir, Ker, double, 0, M>; e.f64[1][i] = launch_lists_rows<Dir, Ker, double, 1, M>; e.f64[2][i] = launch_lists_rows<Dir, Ker, double, 2, M>;
  }
  if constexpr (F) {
    e.f32[0][i] = launch_lists_rows<Dir, Ker, float, 0, M>; e.f32[1][i] = launch_lists_rows<Dir, Ker, float, 1, M>; e.f32[2][i] = e.f32[1][i];
  }
}
// MD, MF: the widest form built in fp64 and in fp32 (2, 4 or 8; the narrower ones are built with it)
template <class Dir, class Ker, int MD, int MF> ListsRowsEntry<Dir> make_lists_rows_entry() {
  ListsRowsEntry<Dir> e{};
  fill_lists_rows<Dir, Ker, 2, (MD >= 2), (MF >= 2)>(e, 0);
  fill_lists_rows<Dir, Ker, 4, (MD >= 4), (MF >= 4)>(e, 1);
  fill_lists_rows<Dir, Ker, 8, (MD >= 8), (MF >= 8)>(e, 2);
  return e;
}

// defined in lmulti_*.hip
const ListsMultiEntry& lmulti_Laplace3D_FxU();
const ListsMultiEntry& lmulti_Laplace3D_DxU();
const ListsMultiEntry& lmulti_Laplace3D_FxdU();
const ListsMultiEntry& lmulti_Stokes3D_FxU();
const ListsMultiEntry& lmulti_Stokes3D_DxU();
const ListsMultiEntry& lmulti_Stokes3D_FxT();
const ListsMultiEntry& lmulti_Stokes3D_FSxU();
const ListsMultiEntry& lmulti_Stokes3D_FxUP();
const ListsMultiEntry& lmulti_Laplace3D_FDxUdU();
const ListsMultiEntry& lmulti_Helmholtz3D_FxU();
// defined in ltmulti_*.hip
const ListsMultiTEntry& ltmulti_Laplace3D_FxU();
const ListsMultiTEntry& ltmulti_Laplace3D_DxU();
const ListsMultiTEntry& ltmulti_Laplace3D_FxdU();
const ListsMultiTEntry& ltmulti_Stokes3D_FxU();
const ListsMultiTEntry& ltmulti_Stokes3D_DxU();
const ListsMultiTEntry& ltmulti_Stokes3D_FxT();
const ListsMultiTEntry& ltmulti_Stokes3D_FSxU();
const ListsMultiTEntry& ltmulti_Stokes3D_FxUP();
const ListsMultiTEntry& ltmulti_Laplace3D_FDxUdU();
const ListsMultiTEntry& ltmulti_Helmholtz3D_FxU();

}  // namespace sctl_amd
