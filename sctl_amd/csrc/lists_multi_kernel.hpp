// Several densities over the P2P lists in one launch: the list evaluator of include/sctl_amd/device/lists_kernel.hpp with M densities per
// source record (ukernels.hpp: NREC_M / pack_m / pair_m).  What a pair costs that does not depend on the density — and here also what a
// SOURCE costs: its index, the gather of its coordinates, its place in the tile — is paid once for M densities.
//
// Same scheme as lists_kernel: one wave64 per work item, XCD-owned shares (xcd_first), every target owned by one lane, sums kept in
// registers in list order and written once, speculative unmasked tiles / steps with repair, the known_coincident shortcut of the packed
// items; no atomics, no workspace, deterministic.  The PLAN is the single-density plan: the kernel walks the same ListItem / ListRange /
// PackedGroup / flat-index arrays, all seven item shapes.  What differs:
//   * records are NREC_M<M> reals (pack_m), the pair is pair_m into acc[M][K1]: a lane holds T x M x K1 sums and as many per-tile sums;
//   * densities are density-major: density m of source s is f[m * f_stride + s * K0 + k], its result v_trg[m * v_stride + t * K1 + k];
//   * the last pass of a call may use fewer densities than the form's M (nact): the others are packed as 0 and never stored;
//   * an item the plan cut for two targets per lane (128 targets, packed classes 1 - 3) runs its targets in TWO HALVES over the same
//     source sequence where the registers do not hold two targets at width M (ListMultiForm::TWO): the item is not shrunk;
//   * where the packed tile of 128 records would cost the second wave per SIMD, the packed groups take one source per lane and step
//     instead of two (ListMultiForm::SPL2): a tile of 64 records, as the one-range items use.
// fp32 runs this exact vector-pipe pair at every accuracy, as eval_multi_kernel does.
#pragma once
#include <sctl_amd/device/launch.hpp>
#include <sctl_amd/device/lists_kernel.hpp>

namespace sctl_amd {

template <class R> struct ListMultiArgs {
  ListArgs<R> l;      // f: density 0 of this pass, v_trg: its result
  int64_t f_stride;   // density m at l.f + m * f_stride
  int64_t v_stride;   // its result at l.v_trg + m * v_stride, accumulated into
  int nact;           // densities in use, 1 <= nact <= M
};

// A workgroup is ONE wave: two waves per SIMD are eight workgroups per CU, so a form may use an eighth of the CU's 160 KB of LDS.
constexpr int kListMultiLdsBudget = 160 * 1024 / 8;

// Shape of the (kernel, precision, M) form.  SPL2 / FITS follow from the LDS bytes alone; TWO is an estimate of the live registers (sums
// and per-tile sums, the record, the sources fetched ahead, the targets; in 32-bit registers, + 40 for addresses, constants and
// bookkeeping) against the 256 a wave may have at two waves per SIMD.  The launch tables (lmulti_*.hip) name the widths that are built;
// what the compiler made of every one of them is in DESIGN.md §4.6 and held to ScratchSize 0 by tests/test_lists_densities_cpu.py.
template <class Ker, class R, int M> struct ListMultiForm {
  static constexpr int VN = VecOf<R>::N;
  static constexpr int NV = (Ker::template NREC_M<M> + VN - 1) / VN;
  static constexpr int SCRATCH = Ker::template Consts<R>::LDS_DOUBLES > 0 ? Ker::template Consts<R>::LDS_DOUBLES : 1;
  static constexpr bool SPL2 = kPackedTileWords(NV) * 16 + SCRATCH * 8 <= kListMultiLdsBudget;
  static constexpr int TILE_WORDS = SPL2 ? kPackedTileWords(NV) : kListTile * NV + 8;   // 8 groups x (8 or 16 records + 1 word)
  static constexpr bool FITS = TILE_WORDS * 16 + SCRATCH * 8 <= kListMultiLdsBudget;
  static constexpr int regs(int t, int spl) {
    return (int)(sizeof(R) / 4) * (2 * t * M * Ker::K1 + NV * VN + spl * (3 + Ker::ND + M * Ker::K0) + 3 * t) + 40;
  }
  static constexpr bool TWO = regs(2, SPL2 ? 2 : 1) <= 252;   // (256 by the estimate spilt: Stokes3D_DxU fp64, 4 densities)
};

// lists_item of lists_kernel.hpp for M densities.  T targets per lane are held; slot j of the lane is target (j0 + j) * 64 + lane of the
// item (j0 = 1: the second half of a 128-target item run in halves).
template <class Ker, class R, int MODE, int M, int T, bool SPLIT, class KC, class V>
__device__ __forceinline__ void lists_multi_item(const ListMultiArgs<R>& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  static_assert(!SPLIT || T == 1, "replicas are for small one-target-per-lane items");
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_M<M>;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  const int lane = threadIdx.x;
  const ListRange* const rg = a.l.ranges + it.first_range;

  int P = kListWave;                       // lanes per replica
  if (SPLIT) { P = 8; while (P < it.nt) P <<= 1; }
  const int nrep = kListWave / P, rep = lane / P;

  R xt[T][3], acc[T][M][K1];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int tl = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    if (tl >= it.nt) tl = it.nt - 1;      // idle lanes repeat the last target; never stored
    const int64_t t = it.t0 + tl;
#pragma unroll
    for (int k = 0; k < 3; k++) xt[j][k] = a.l.xt[t * 3 + k];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K1; k++) acc[j][m][k] = 0;
  }

  // cursor into the concatenated source sequence (wave-uniform): range r, offset o inside it
  int r = 0;
  int64_t o = 0;
  R sx[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sf[M][K0];
#pragma unroll
  for (int m = 0; m < M; m++)
#pragma unroll
    for (int k = 0; k < K0; k++) sf[m][k] = 0;
  // fetch the next (up to) 64 sources of the sequence into registers, lane i the i-th of them, with their M densities; returns how many
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
      for (int k = 0; k < 3; k++) sx[k] = a.l.xs[mine * 3 + k];
#pragma unroll
      for (int k = 0; k < ND; k++) sn[k] = a.l.xn[mine * ND + k];
#pragma unroll
      for (int m = 0; m < M; m++) {
        if (m < a.nact) {                  // (wave-uniform; the rows past nact stay 0)
          const R* const pf = a.l.f + m * a.f_stride + mine * K0;
#pragma unroll
          for (int k = 0; k < K0; k++) sf[m][k] = pf[k];
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
      Ker::template pack_m<R, M>(rec, sx, sn, sf);
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
          if constexpr (KC::HAS_VARIANT) Ker::template pair_m<R, MODE, MASKED, M, VARIANT>(tacc[j], d, rec, a.l.ctx, K);
          else Ker::template pair_m<R, MODE, MASKED, M>(tacc[j], d, rec, a.l.ctx, K);
        }
      };
      if (SPLIT) {                         // replica `rep` takes sources rep, rep + nrep, ... of the tile
        const int cnt = (ns_cur + nrep - 1) / nrep;   // wave-uniform trip count; the tail of a short tile is predicated
        for (int i = 0; i < cnt; i++) {
          const int s = i * nrep + rep;
          if (s < ns_cur) one_source(s);
        }
      } else if (ns_cur == kListTile) {
#pragma unroll UnrollOf<T, M * Ker::K1>::value
        for (int s = 0; s < kListTile; s++) one_source(s);
      } else {
        for (int s = 0; s < ns_cur; s++) one_source(s);
      }
    };
    auto run_tile = [&](auto masked_tag) {   // (one-wave work items: the small tables, variants 0 / 1 only, as in lists_kernel)
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
          for (int k = 0; k < K1; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 4 > tiles + 4) always_masked = true;   // mostly coincident points (tiny boxes): stop speculating
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) acc[j][m][k] += tacc[j][m][k];
  }

  if (SPLIT) {                             // add the replicas' sums: lanes l, l ^ P, l ^ 2P, ... hold the same target
    for (int off = P; off < kListWave; off <<= 1)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) acc[0][m][k] += __shfl_xor(acc[0][m][k], off);
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int tl = SPLIT ? (lane & (P - 1)) : ((j0 + j) * kListWave + lane);
    const bool store = tl < it.nt && (!SPLIT || rep == 0);
    const int64_t t = it.t0 + (store ? tl : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_acc<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const v = a.l.v_trg + m * a.v_stride + t * K1;
#pragma unroll
        for (int k = 0; k < K1; k++) v[k] += acc[j][m][k] * a.l.scale;   // generic-kernel.txx:184
      }
    }
  }
}

// lists_packed_item of lists_kernel.hpp for M densities.  T targets per lane are held; slot j of a lane is target (j0 + j) * P + i of its
// group (j0 = 1: the second half of a two-targets-per-lane class run in halves; a wave whose groups all fit the first half skips it).
template <class Ker, class R, int MODE, int M, int P, int T, int SPL, class KC, class V>
__device__ __forceinline__ void lists_multi_packed_item(const ListMultiArgs<R>& a, const ListItem& it, V* tile, const KC& K, const int j0) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::template NREC_M<M>;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  constexpr int G = kListWave / P, S = P * SPL, SLICE = S * NV + 1;   // S sources per group and step (SPL per lane); 16-byte words per group slice (+ 1: bank spread)
  static_assert(G * SLICE <= ListMultiForm<Ker, R, M>::TILE_WORDS, "the packed slices fit the form's LDS tile");
  const int lane = threadIdx.x, g = lane / P, i = lane % P;
  const bool live = g < it.nt;                              // (it.nt = groups of this item)
  const PackedGroup pg = a.l.groups[it.t0 + (live ? g : 0)];
  if (j0 > 0 && !__any(live && pg.nt > j0 * P)) return;    // wave-uniform: no group of this wave reaches into the second half
  const int nsrc = live ? pg.nsrc : 0;
  const bool self = (const void*)a.l.xs == (const void*)a.l.xt;

  R xt[T][3], acc[T][M][K1];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int tl = (j0 + j) * P + i;
    if (tl >= pg.nt) tl = pg.nt - 1;                        // idle slots repeat the last target; never stored
    const int64_t t = pg.t0 + tl;
#pragma unroll
    for (int k = 0; k < 3; k++) xt[j][k] = a.l.xt[t * 3 + k];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K1; k++) acc[j][m][k] = 0;
  }
  int nmax = nsrc;                                          // the longest sequence of the wave decides the trip count
  for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(nmax, o); nmax = (w > nmax) ? w : nmax; }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  const int nsteps = (nmax + S - 1) / S;

  R sx[SPL][3], sn[SPL][3], sf[SPL][M][K0];
#pragma unroll
  for (int u = 0; u < SPL; u++) {
#pragma unroll
    for (int k = 0; k < 3; k++) { sx[u][k] = 0; sn[u][k] = 0; }
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int k = 0; k < K0; k++) sf[u][m][k] = 0;
  }
  // Sources one step ahead, their indices two steps ahead, 32-bit byte offsets from scalar bases: as in lists_packed_item.  The M density
  // rows are M scalar bases (f + m * f_stride) with the same lane offset.
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t own_lo = (uint32_t)pg.t0, own_n = self ? (uint32_t)pg.nt : 0u;   // (own points exist only when the sources ARE the targets)
  const uint32_t* const flat_g = a.l.flat + pg.flat_off;
  bool own = false;    // a source this lane holds for the coming step is one of its group's targets
  uint32_t idx_next[SPL];
  auto load_idx = [&](int step) {
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      const int q = step * S + u * P + i;
      idx_next[u] = (q < nsrc) ? flat_g[q] : kNone;
    }
  };
  if (nsteps > 0) load_idx(0);
  auto at = [](const R* base, uint32_t byte_off) -> const R* { return (const R*)((const char*)base + byte_off); };
  auto fetch = [&](int step) {
    uint32_t src[SPL];
#pragma unroll
    for (int u = 0; u < SPL; u++) src[u] = idx_next[u];
    if (step + 1 < nsteps) load_idx(step + 1);
    own = false;
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (src[u] != kNone) {
        own = own || (src[u] - own_lo < own_n);
        const R* const px = at(a.l.xs, src[u] * (uint32_t)(3 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < 3; k++) sx[u][k] = px[k];
        if (ND > 0) {
          const R* const pn = at(a.l.xn, src[u] * (uint32_t)(ND * sizeof(R)));
#pragma unroll
          for (int k = 0; k < ND; k++) sn[u][k] = pn[k];
        }
#pragma unroll
        for (int m = 0; m < M; m++) {
          if (m < a.nact) {                                 // (wave-uniform; the rows past nact stay 0)
            const R* const pf = at(a.l.f + m * a.f_stride, src[u] * (uint32_t)(K0 * sizeof(R)));
#pragma unroll
            for (int k = 0; k < K0; k++) sf[u][m][k] = pf[k];
          }
        }
      }
    }
  };
  V* const slice = tile + g * SLICE;
  if (nsteps > 0) fetch(0);
  for (int step = 0; step < nsteps; step++) {
    __syncthreads();   // previous slices fully consumed
    const int cnt = nsrc - step * S;                        // sources of this group in this step: >= S (full), 1 .. S - 1 (its last), <= 0 (done)
    const bool known_coincident = __any(own);               // (of the step being staged now: `own` belongs to the sources fetched for it)
#pragma unroll
    for (int u = 0; u < SPL; u++) {
      if (u * P + i < cnt) {
        R rec[NRECP] = {};
        Ker::template pack_m<R, M>(rec, sx[u], sn[u], sf[u]);
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

    R tacc[T][M][K1];
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
          for (int k = 0; k < K1; k++) tacc[j][m][k] = 0;
      auto one_source = [&](int s) {
        R rec[NRECP];
#pragma unroll
        for (int v = 0; v < NV; v++) {
          const V w = slice[s * NV + v];
#pragma unroll
          for (int e = 0; e < VN; e++) rec[v * VN + e] = w[e];
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
          const R d[3] = {xt[j][0] - rec[0], xt[j][1] - rec[1], xt[j][2] - rec[2]};
          if constexpr (KC::HAS_VARIANT) Ker::template pair_m<R, MODE, MASKED, M, VARIANT>(tacc[j], d, rec, a.l.ctx, K);
          else Ker::template pair_m<R, MODE, MASKED, M>(tacc[j], d, rec, a.l.ctx, K);
        }
      };
      if (full) {
#pragma unroll UnrollOf<T, M * Ker::K1>::value
        for (int s = 0; s < S; s++) one_source(s);
      } else {                                              // a group's last step: its remaining sources, the other groups' lanes idle
        int cmax = cnt;
        for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(cmax, o); cmax = (w > cmax) ? w : cmax; }
        cmax = __builtin_amdgcn_readfirstlane(cmax < S ? cmax : S);
        for (int s = 0; s < cmax; s++)
          if (s < cnt) one_source(s);
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
          for (int k = 0; k < K1; k++) bad |= !(fabs_(tacc[j][m][k]) <= max_finite<R>());
      repaired = __any(bad);
    }
    if (repaired) run_step(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int m = 0; m < M; m++)
#pragma unroll
        for (int k = 0; k < K1; k++) acc[j][m][k] += tacc[j][m][k];
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int tl = (j0 + j) * P + i;
    const bool store = live && tl < pg.nt;
    const int64_t t = pg.t0 + (store ? tl : 0);
#pragma unroll
    for (int m = 0; m < M; m++) {
      if (m >= a.nact) break;
      finish_acc<Ker, R, MODE>(acc[j][m]);
      if (store) {
        R* const v = a.l.v_trg + m * a.v_stride + t * K1;
#pragma unroll
        for (int k = 0; k < K1; k++) v[k] += acc[j][m][k] * a.l.scale;   // generic-kernel.txx:184
      }
    }
  }
}

// The dispatch of lists_kernel over the plan's seven item shapes.  An item cut for two targets per lane holds both (TWO) or runs twice.
template <class Ker, class R, int MODE, int M>
__global__ void __launch_bounds__(kListWave, 2) lists_multi_kernel(const ListMultiArgs<R> a) {
  using V = typename VecOf<R>::type;
  using F = ListMultiForm<Ker, R, M>;
  static_assert(F::FITS, "this form's LDS tile leaves less than two waves per SIMD: it is not built (lmulti_*.hip)");
  constexpr bool TWO = F::TWO;
  constexpr int SPL = F::SPL2 ? 2 : 1;
  __shared__ V tile[F::TILE_WORDS];
  using KC = typename Ker::template Consts<R>;
  __shared__ double kscratch[F::SCRATCH];
  const KC K = make_consts<KC>(kscratch, a.l.ctx, MODE);
  const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;      // XCD x walks its share of the item list (lists_kernel)
  if (j >= a.l.xcd_first[xcd + 1] - a.l.xcd_first[xcd]) return;
  const ListItem it = a.l.items[a.l.xcd_first[xcd] + j];
  if (it.nranges < 0) {      // packed small target ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) {
      lists_multi_packed_item<Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, 0);
    } else if (cls == 1) {
      if constexpr (TWO) lists_multi_packed_item<Ker, R, MODE, M, 8, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_packed_item<Ker, R, MODE, M, 8, 1, SPL>(a, it, tile, K, h);
      }
    } else if (cls == 2) {
      if constexpr (TWO) lists_multi_packed_item<Ker, R, MODE, M, 16, 2, SPL>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_packed_item<Ker, R, MODE, M, 16, 1, SPL>(a, it, tile, K, h);
      }
    } else {
      if constexpr (TWO) lists_multi_packed_item<Ker, R, MODE, M, 32, 2, 1>(a, it, tile, K, 0);
      else {
#pragma unroll 1
        for (int h = 0; h < 2; h++) lists_multi_packed_item<Ker, R, MODE, M, 32, 1, 1>(a, it, tile, K, h);
      }
    }
    return;
  }
  if (it.nt > kListWave) {
    if constexpr (TWO) lists_multi_item<Ker, R, MODE, M, 2, false>(a, it, tile, K, 0);
    else {
#pragma unroll 1
      for (int h = 0; h < 2; h++) lists_multi_item<Ker, R, MODE, M, 1, false>(a, it, tile, K, h);
    }
  } else if (it.nt > kListWave / 2) {
    lists_multi_item<Ker, R, MODE, M, 1, false>(a, it, tile, K, 0);
  } else {
    lists_multi_item<Ker, R, MODE, M, 1, true>(a, it, tile, K, 0);
  }
}

// ---- launch table: one per built-in kernel (lmulti_<Kernel>.hip), none for plugin kernels ----------------------------------------------
constexpr int kNumListMultiM = 3;                    // forms of 2, 4 and 8 densities
constexpr int kListMultiM[kNumListMultiM] = {2, 4, 8};
template <class R> using ListsMultiLaunch = void (*)(const ListMultiArgs<R>&, int64_t nblocks, hipStream_t);
struct ListsMultiEntry {
  ListsMultiLaunch<double> f64[kNumMode][kNumListMultiM];   // null: no such form
  ListsMultiLaunch<float> f32[kNumMode][kNumListMultiM];    // modes 0 and 1 (mode 2 aliases 1)
};

template <class Ker, class R, int MODE, int M> void launch_lists_multi(const ListMultiArgs<R>& a, int64_t nblocks, hipStream_t st) {
  hipLaunchKernelGGL((lists_multi_kernel<Ker, R, MODE, M>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}
template <class Ker, int M, bool D, bool F> void fill_lists_multi(ListsMultiEntry& e, int i) {
  if constexpr (D) {
    e.f64[0][i] = launch_lists_multi<Ker, double, 0, M>; e.f64[1][i] = launch_lists_multi<Ker, double, 1, M>; e.f64[2][i] = launch_lists_multi<Ker, double, 2, M>;
  }
  if constexpr (F) {
    e.f32[0][i] = launch_lists_multi<Ker, float, 0, M>; e.f32[1][i] = launch_lists_multi<Ker, float, 1, M>; e.f32[2][i] = e.f32[1][i];
  }
}
// MD, MF: the widest form built in fp64 and in fp32 (2, 4 or 8; the narrower ones are built with it)
template <class Ker, int MD, int MF> ListsMultiEntry make_lists_multi_entry() {
  ListsMultiEntry e{};
  fill_lists_multi<Ker, 2, (MD >= 2), (MF >= 2)>(e, 0);
  fill_lists_multi<Ker, 4, (MD >= 4), (MF >= 4)>(e, 1);
  fill_lists_multi<Ker, 8, (MD >= 8), (MF >= 8)>(e, 2);
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

}  // namespace sctl_amd
