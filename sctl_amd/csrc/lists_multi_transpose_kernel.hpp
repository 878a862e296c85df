// Several weight vectors through the transposed sum over the P2P lists in one launch: the transposed list evaluator of
// include/sctl_amd/device/lists_transpose_kernel.hpp with M weight vectors per streamed target record (ukernels.hpp: NREC_TM / pack_tm / pair_tm),
//     g[m][s,k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t,k1],   m = 0 .. nd-1.
// It relates to lists_transpose_kernel.hpp as lists_multi_kernel.hpp relates to lists_kernel.hpp.  What a pair costs that does not depend on the weights
// — and here also what a streamed TARGET costs: its index, the gather of its coordinates, its place in the tile — is paid once for M weight vectors.
//
// Same scheme as lists_transpose_kernel: one wave64 per work item, XCD-owned shares (xcd_first), every source owned by one lane, sums kept in registers
// in list order and written once, speculative unmasked tiles / steps with repair, the known_coincident shortcut of the packed items; no atomics, no
// workspace, deterministic.  The PLAN is the single-vector transposed plan: the kernel walks the same ListItem / ListRange / PackedGroup / flat-index
// arrays, all seven item shapes.  What differs:
//   * records are NREC_TM<M> reals (pack_tm), the pair is pair_tm into acc[M][K0]: a lane holds T x M x K0 sums and as many per-tile sums;
//   * rows are row-major: weights m of target t are w[m * w_stride + t * K1 + k], their result g_src[m * g_stride + s * K0 + k];
//   * the last pass of a call may use fewer rows than the form's M (nact): the others are packed as 0 and never stored;
//   * an item the plan cut for two owners per lane (128 sources, packed classes 1 - 3) runs its owners in TWO HALVES over the same target sequence
//     where the registers do not hold two owners at width M (ListMultiTForm::TWO): the item is not shrunk;
//   * where the packed tile of 128 records would cost the second wave per SIMD, the packed groups take one target per lane and step instead of two
//     (ListMultiTForm::SPL2): a tile of 64 records, as the one-range items use.
// fp32 runs this exact vector-pipe pair at every accuracy, as every transposed kernel does.
#pragma once
#include <sctl_amd/device/launch.hpp>
#include <sctl_amd/device/lists_transpose_kernel.hpp>

namespace sctl_amd {

template <class R> struct ListMultiTArgs {
  ListTArgs<R> l;     // w: row 0 of this pass, g_src: its result
  int64_t w_stride;   // weights m at l.w + m * w_stride
  int64_t g_stride;   // their result at l.g_src + m * g_stride, accumulated into
  int nact;           // rows in use, 1 <= nact <= M
};

// A workgroup is ONE wave: two waves per SIMD are eight workgroups per CU, so a form may use an eighth of the CU's 160 KB of LDS.
constexpr int kListMultiTLdsBudget = 160 * 1024 / 8;

// Shape of the (kernel, precision, M) form.  SPL2 / FITS follow from the LDS bytes alone; TWO is an estimate of the live registers (per owner:
// coordinates, normal, sums and per-tile sums; the record; the targets fetched ahead with their M weights; in 32-bit registers, + 40 for addresses,
// constants and bookkeeping) against the 256 a wave may have at two waves per SIMD.  The launch tables (ltmulti_*.hip) name the widths that are built;
// what the compiler made of every one of them is in DESIGN.md §4.15 and held to ScratchSize 0 by tests/test_lists_transpose_densities_cpu.py.
template <class Ker, class R, int M> struct ListMultiTForm {
  static constexpr int VN = VecOf<R>::N;
  static constexpr int NV = (Ker::template NREC_TM<M> + VN - 1) / VN;
  static constexpr int SCRATCH = Ker::template Consts<R>::LDS_DOUBLES > 0 ? Ker::template Consts<R>::LDS_DOUBLES : 1;
  static constexpr bool SPL2 = kPackedTileWords(NV) * 16 + SCRATCH * 8 <= kListMultiTLdsBudget;
  static constexpr int TILE_WORDS = SPL2 ? kPackedTileWords(NV) : kListTile * NV + 8;   // 8 groups x (8 or 16 records + 1 word)
  static constexpr bool FITS = TILE_WORDS * 16 + SCRATCH * 8 <= kListMultiTLdsBudget;
  static constexpr int regs(int t, int spl) {
    return (int)(sizeof(R) / 4) * (t * (3 + (Ker::ND ? 3 : 0) + 2 * M * Ker::K0) + NV * VN + spl * (3 + M * Ker::K1)) + 40;
  }
  static constexpr bool TWO = regs(2, SPL2 ? 2 : 1) <= 252;
};

// lists_t_item of lists_transpose_kernel.hpp for M weight vectors.  T owners per lane are held; slot j of the lane is source (j0 + j) * 64 + lane of
// the item (j0 = 1: the second half of a 128-source item run in halves).
template <class Ker, class R, int MODE, int M, int T, bool SPLIT, class KC, class V>
__device__ __forceinline__ void lists_multi_t_item(const ListMultiTArgs<R>& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  static_assert(!SPLIT || T == 1, "replicas are for small one-owner-per-lane items");
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_TM<M>, NN = ND ? 3 : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  const int lane = threadIdx.x;
  const ListRange* const rg = a.l.ranges + it.first_range;

  int P = kListWave;                       // lanes per replica
  if (SPLIT) { P = 8; while (P < it.nt) P <<= 1; }
  const int nrep = kListWave / P, rep = lane / P;

  R xs[T][3], xn[T][NN], acc[T][M][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int sl = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    if (sl >= it.nt) sl = it.nt - 1;      // idle lanes repeat the last owner; never stored
    const int64_t s = it.t0 + sl;
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.l.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.l.xn[s * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][m][k] = 0;
  }

  // cursor into the concatenated target sequence (wave-uniform): range r, offset o inside it
  int r = 0;
  int64_t o = 0;
  R px[3] = {0, 0, 0}, pw[M][K1];
#pragma unroll
  for (int m = 0; m < M; m++)
#pragma unroll
    for (int k = 0; k < K1; k++) pw[m][k] = 0;
  // fetch the next (up to) 64 targets of the sequence into registers, lane i the i-th of them, with their M weights; returns how many
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
      for (int k = 0; k < 3; k++) px[k] = a.l.xt[mine * 3 + k];
#pragma unroll
      for (int m = 0; m < M; m++) {
        if (m < a.nact) {                  // (wave-uniform; the rows past nact stay 0)
          const R* const qw = a.l.w + m * a.w_stride + mine * K1;
#pragma unroll
          for (int k = 0; k < K1; k++) pw[m][k] = qw[k];
        }
      }
    }
    return fill;
  };

  int repairs = 0, tiles = 0;
  bool always_masked = false;
  int nt = fetch();
  while (nt > 0) {
    __syncthreads();   // previous tile fully consumed
    if (lane < nt) {
      R rec[NRECP] = {};
      Ker::template pack_tm<R, M>(rec, px, pw);
#pragma unroll
      for (int v = 0; v < NV; v++) {
        V q;
#pragma unroll
        for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
        tile[lane * NV + v] = q;
      }
    }
    const int nt_cur = nt;
    nt = fetch();      // loads for the next tile are in flight during this tile's arithmetic
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
          if constexpr (KC::HAS_VARIANT) Ker::template pair_tm<R, MODE, MASKED, M, VARIANT>(tacc[j], d, xn[j], rec, a.l.ctx, K);
          else Ker::template pair_tm<R, MODE, MASKED, M>(tacc[j], d, xn[j], rec, a.l.ctx, K);
        }
      };
      if (SPLIT) {                         // replica `rep` takes targets rep, rep + nrep, ... of the tile
        const int cnt = (nt_cur + nrep - 1) / nrep;   // wave-uniform trip count; the tail of a short tile is predicated
        for (int i = 0; i < cnt; i++) {
          const int t = i * nrep + rep;
          if (t < nt_cur) one_target(t);
        }
      } else if (nt_cur == kListTile) {
#pragma unroll UnrollOf<T, M * Ker::K0>::value
        for (int t = 0; t < kListTile; t++) one_target(t);
      } else {
        for (int t = 0; t < nt_cur; t++) one_target(t);
      }
    };
    auto run_tile = [&](auto masked_tag) {   // (one-wave work items: the small tables, variants 0 / 1 only, as in lists_transpose_kernel)
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
          for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 4 > tiles + 4) always_masked = true;   // mostly coincident points (tiny boxes): stop speculating
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) acc[j][m][k] += tacc[j][m][k];
  }

  if (SPLIT) {                             // add the replicas' sums: lanes l, l ^ P, l ^ 2P, ... hold the same owner
    for (int off = P; off < kListWave; off <<= 1)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) acc[0][m][k] += __shfl_xor(acc[0][m][k], off);
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int sl = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    const bool store = sl < it.nt && (!SPLIT || rep == 0);
    const int64_t s = it.t0 + (store ? sl : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_t_acc<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const g = a.l.g_src + m * a.g_stride + s * K0;
#pragma unroll
        for (int k = 0; k < K0; k++) g[k] += acc[j][m][k] * a.l.scale;
      }
    }
  }
}

// lists_t_packed_item of lists_transpose_kernel.hpp for M weight vectors.  T owners per lane are held; slot j of a lane is source (j0 + j) * P + i of
// its group (j0 = 1: the second half of a two-owners-per-lane class run in halves; a wave whose groups all fit the first half skips it).
template <class Ker, class R, int MODE, int M, int P, int T, int SPL, class KC, class V>
__device__ __forceinline__ void lists_multi_t_packed_item(const ListMultiTArgs<R>& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_TM<M>, NN = ND ? 3 : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  constexpr int G = kListWave / P, S = P * SPL, SLICE = S * NV + 1;   // S targets per group and step (SPL per lane); 16-byte words per group slice (+ 1: bank spread)
  static_assert(G * SLICE <= ListMultiTForm<Ker, R, M>::TILE_WORDS, "the packed slices fit the form's LDS tile");
  const int lane = threadIdx.x, g = lane / P, i = lane % P;
  const bool live = g < it.nt;                              // (it.nt = groups of this item)
  const PackedGroup pg = a.l.groups[it.t0 + (live ? g : 0)];
  if (j0 > 0 && !__any(live && pg.nt > j0 * P)) return;    // wave-uniform: no group of this wave reaches into the second half
  const int ntrg = live ? pg.nsrc : 0;                      // streamed targets of the group
  const bool self = (const void*)a.l.xs == (const void*)a.l.xt;

  R xs[T][3], xn[T][NN], acc[T][M][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int sl = (j0 + j) * P + i;
    if (sl >= pg.nt) sl = pg.nt - 1;                        // idle slots repeat the last owner; never stored
    const int64_t s = pg.t0 + sl;
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.l.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.l.xn[s * ND + k] : R(0);
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][m][k] = 0;
  }
  int nmax = ntrg;                                          // the longest sequence of the wave decides the trip count
  for (int o = 32; o > 0; o >>= 1) { const int q = __shfl_xor(nmax, o); nmax = (q > nmax) ? q : nmax; }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  const int nsteps = (nmax + S - 1) / S;

  R px[SPL][3], pw[SPL][M][K1];
#pragma unroll
  for (int u = 0; u < SPL; u++) {
#pragma unroll
    for (int k = 0; k < 3; k++) px[u][k] = 0;
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K1; k++) pw[u][m][k] = 0;
  }
  // Targets one step ahead, their indices two steps ahead, 32-bit byte offsets from scalar bases: as in lists_t_packed_item.  The M weight rows are
  // M scalar bases (w + m * w_stride) with the same lane offset.
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t own_lo = (uint32_t)pg.t0, own_n = self ? (uint32_t)pg.nt : 0u;   // (own points exist only when the sources ARE the targets)
  const uint32_t* const flat_g = a.l.flat + pg.flat_off;
  bool own = false;    // a target this lane holds for the coming step is one of its group's owners
  uint32_t idx_next[SPL];
  auto load_idx = [&](int step) {
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      const int q = step * S + u * P + i;
      idx_next[u] = (q < ntrg) ? flat_g[q] : kNone;
    }
  };
  if (nsteps > 0) load_idx(0);
  auto at = [](const R* base, uint32_t byte_off) -> const R* { return (const R*)((const char*)base + byte_off); };
  auto fetch = [&](int step) {
    uint32_t trg[SPL];
#pragma unroll
    for (int u = 0; u < SPL; u++) trg[u] = idx_next[u];
    if (step + 1 < nsteps) load_idx(step + 1);
    own = false;
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (trg[u] != kNone) {
        own = own || (trg[u] - own_lo < own_n);
        const R* const qx = at(a.l.xt, trg[u] * (uint32_t)(3 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < 3; k++) px[u][k] = qx[k];
#pragma unroll
        for (int m = 0; m < M; m++) {
          if (m < a.nact) {                                 // (wave-uniform; the rows past nact stay 0)
            const R* const qw = at(a.l.w + m * a.w_stride, trg[u] * (uint32_t)(K1 * sizeof(R)));
#pragma unroll
            for (int k = 0; k < K1; k++) pw[u][m][k] = qw[k];
          }
        }
      }
    }
  };
  V* const slice = tile + g * SLICE;
  if (nsteps > 0) fetch(0);
  for (int step = 0; step < nsteps; step++) {
    __syncthreads();   // previous slices fully consumed
    const int cnt = ntrg - step * S;                        // targets of this group in this step: >= S (full), 1 .. S - 1 (its last), <= 0 (done)
    const bool known_coincident = __any(own);               // (of the step being staged now: `own` belongs to the targets fetched for it)
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (u * P + i < cnt) {
        R rec[NRECP] = {};
        Ker::template pack_tm<R, M>(rec, px[u], pw[u]);
#pragma unroll
        for (int v = 0; v < NV; v++) {
          V q;
#pragma unroll
          for (int e = 0; e < VN; e++) q[e] = rec[v * VN + e];
          slice[(u * P + i) * NV + v] = q;
        }
      }
    }
    if (step + 1 < nsteps) fetch(step + 1);
    __syncthreads();

    R tacc[T][M][K0];
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
          for (int k = 0; k < K0; k++) tacc[j][m][k] = 0;
      auto one_target = [&](int t) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V q = slice[t * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = q[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
          const R d[3] = {rec[0] - xs[j][0], rec[1] - xs[j][1], rec[2] - xs[j][2]};
          if constexpr (KC::HAS_VARIANT) Ker::template pair_tm<R, MODE, MASKED, M, VARIANT>(tacc[j], d, xn[j], rec, a.l.ctx, K);
          else Ker::template pair_tm<R, MODE, MASKED, M>(tacc[j], d, xn[j], rec, a.l.ctx, K);
        }
      };
      if (full) {
#pragma unroll UnrollOf<T, M * Ker::K0>::value
        for (int t = 0; t < S; t++) one_target(t);
      } else {                                              // a group's last step: its remaining targets, the other groups' lanes idle
        int cmax = cnt;
        for (int o = 32; o > 0; o >>= 1) { const int q = __shfl_xor(cmax, o); cmax = (q > cmax) ? q : cmax; }
        cmax = __builtin_amdgcn_readfirstlane(cmax < S ? cmax : S);
        for (int t = 0; t < cmax; t++)
          if (t < cnt) one_target(t);
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
          for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);
    }
    if (repaired) run_step(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K0; k++) acc[j][m][k] += tacc[j][m][k];
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int sl = (j0 + j) * P + i;
    const bool store = live && sl < pg.nt;
    const int64_t s = pg.t0 + (store ? sl : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_t_acc<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const gm = a.l.g_src + m * a.g_stride + s * K0;
#pragma unroll
        for (int k = 0; k < K0; k++) gm[k] += acc[j][m][k] * a.l.scale;
      }
    }
  }
}

// The dispatch of lists_transpose_kernel over the plan's seven item shapes.  An item cut for two owners per lane holds both (TWO) or runs twice.
template <class Ker, class R, int MODE, int M>
__global__ void __launch_bounds__(kListWave, 2) lists_multi_transpose_kernel(const ListMultiTArgs<R> a) {
  using V = typename VecOf<R>::type;
  using F = ListMultiTForm<Ker, R, M>;
  static_assert(F::FITS, "this form's LDS tile leaves less than two waves per SIMD: it is not built (ltmulti_*.hip)");
  constexpr bool TWO = F::TWO;
  constexpr int SPL = F::SPL2 ? 2 : 1;
  __shared__ V tile[F::TILE_WORDS];
  using KC = typename Ker::template Consts<R>;
  __shared__ double kscratch[F::SCRATCH];
  const KC K = make_consts<KC>(kscratch, a.l.ctx, MODE);
  const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;      // XCD x walks its share of the item list (lists_transpose_kernel)
  if (j >= a.l.xcd_first[xcd + 1] - a.l.xcd_first[xcd]) return;
  const ListItem it = a.l.items[a.l.xcd_first[xcd] + j];
  if (it.nranges < 0) {      // packed small source ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) {
      lists_multi_t_packed_item<Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, 0);
    } else if (cls == 1) {
      if constexpr (TWO) lists_multi_t_packed_item<Ker, R, MODE, M, 8, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_t_packed_item<Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, h);
      }
    } else if (cls == 2) {
      if constexpr (TWO) lists_multi_t_packed_item<Ker, R, MODE, M, 16, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_t_packed_item<Ker, R, MODE, M, 16, 1, SPL>(a, it, tile, K, h);
      }
    } else {
      if constexpr (TWO) lists_multi_t_packed_item<Ker, R, MODE, M, 32, 2, 1>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_t_packed_item<Ker, R, MODE, M, 32, 1, 1>(a, it, tile, K, h);
      }
    }
    return;
  }
  if (it.nt > kListWave) {
    if constexpr (TWO) lists_multi_t_item<Ker, R, MODE, M, 2, false>(a, it, tile, K, 0);
    else {
#pragma unroll 1
      for (int h = 0; h < 2; h++) lists_multi_t_item<Ker, R, MODE, M, 1, false>(a, it, tile, K, h);
    }
  } else if (it.nt > kListWave / 2) {
    lists_multi_t_item<Ker, R, MODE, M, 1, false>(a, it, tile, K, 0);
  } else {
    lists_multi_t_item<Ker, R, MODE, M, 1, true>(a, it, tile, K, 0);
  }
}

// ---- launch table: one per built-in kernel (ltmulti_<Kernel>.hip), none for plugin kernels ---------------------------------------------
constexpr int kNumListMultiTM = 3;                   // forms of 2, 4 and 8 weight vectors
constexpr int kListMultiTM[kNumListMultiTM] = {2, 4, 8};
template <class R> using ListsMultiTLaunch = void (*)(const ListMultiTArgs<R>&, int64_t nblocks, hipStream_t);
struct ListsMultiTEntry {
  ListsMultiTLaunch<double> f64[kNumMode][kNumListMultiTM];   // null: no such form
  ListsMultiTLaunch<float> f32[kNumMode][kNumListMultiTM];    // modes 0 and 1 (mode 2 aliases 1)
};

template <class Ker, class R, int MODE, int M> void launch_lists_multi_t(const ListMultiTArgs<R>& a, int64_t nblocks, hipStream_t st) {
  hipLaunchKernelGGL((lists_multi_transpose_kernel<Ker, R, MODE, M>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}
template <class Ker, int M, bool D, bool F> void fill_lists_multi_t(ListsMultiTEntry& e, int i) {
  if constexpr (D) {
    e.f64[0][i] = launch_lists_multi_t<Ker, double, 0, M>; e.f64[1][i] = launch_lists_multi_t<Ker, double, 1, M>; e.f64[2][i] = launch_lists_multi_t<Ker, double, 2, M>;
  }
  if constexpr (F) {
    e.f32[0][i] = launch_lists_multi_t<Ker, float, 0, M>; e.f32[1][i] = launch_lists_multi_t<Ker, float, 1, M>; e.f32[2][i] = e.f32[1][i];
  }
}
// MD, MF: the widest form built in fp64 and in fp32 (2, 4 or 8; the narrower ones are built with it)
template <class Ker, int MD, int MF> ListsMultiTEntry make_lists_multi_t_entry() {
  ListsMultiTEntry e{};
  fill_lists_multi_t<Ker, 2, (MD >= 2), (MF >= 2)>(e, 0);
  fill_lists_multi_t<Ker, 4, (MD >= 4), (MF >= 4)>(e, 1);
  fill_lists_multi_t<Ker, 8, (MD >= 8), (MF >= 8)>(e, 2);
  return e;
}

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
