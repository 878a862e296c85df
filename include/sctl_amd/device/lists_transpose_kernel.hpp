// Transposed batched list evaluation for gfx950: the adjoint of lists_kernel's sum over the same lists,
//     g[s,k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[t,k1],
// in ONE launch.  It relates to lists_kernel.hpp as eval_transpose_kernel.hpp relates to eval_kernel.hpp: the scheme is the forward list kernel's
//  with the roles of the two point sets exchanged.
//   * a work item = up to 64*T SOURCES of one source range (leaf box) + ALL target ranges listed for that box; one wave64 per item;
//   * every source is owned by exactly one item, so sums are accumulated in registers in list order and written once: deterministic, no atomics,
//     no partial-sum workspace — which is why the plan asks of the SOURCE ranges what the forward plan asks of the target ranges;
//   * a lane holds its owners' coordinates, their normals where ND > 0, and K0 sums; the item's target ranges stream as ONE concatenated sequence
//     through a 64-record LDS tile of pack_t() records (NREC_T reals: coordinates, then what the pair needs of w[K1]); the next tile's targets and
//     weights are fetched into registers while the current tile is evaluated;
//   * the pair is pair_t with d = x_trg - x_src, the forward sign; a tile runs unmasked into per-tile sums and is repaired when a coincident pair
//     shows up, as in lists_kernel.hpp;
//   * small owner ranges are PACKED, 64 / P to a wave, every group of lanes walking its own flat sequence of TARGET indices.
// The work list has the forward kernel's layout (ListItem, ListRange, PackedGroup) with the meanings exchanged: an item's t0 / nt name its OWNERS
// (sources), a range's s0 / ns the STREAMED points (targets), and the flat index list holds target indices.
#pragma once
#include "lists_kernel.hpp"

namespace sctl_amd {

template <class R> struct ListTArgs {
  int32_t xcd_first[9];   // items [xcd_first[x], xcd_first[x + 1]) are the share of XCD x
  const ListItem* items;  // t0, nt: the item's sources
  const ListRange* ranges;   // s0, ns: target ranges
  const R* xs;      // [Ns*3]   owners
  const R* xn;      // [Ns*ND] or null
  const R* xt;      // [Nt*3]   streamed
  const R* w;       // [Nt*K1]  target weights, streamed
  R* g_src;         // [Ns*K0], accumulated into
  R scale;
  KerCtx ctx;
  const PackedGroup* groups;   // packed items only: t0, nt the group's sources, nsrc its streamed targets
  const uint32_t* flat;        // their target sequences: indices into xt / w
};

// One work item with T sources per lane; SPLIT: replicas of 8 / 16 / 32 lanes for at most 32 owners (lists_item in lists_kernel.hpp).
template <class Ker, class R, int MODE, int T, bool SPLIT, class KC, class V>
__device__ __forceinline__ void lists_t_item(const ListTArgs<R>& a, const ListItem& it, V* tile, const KC& K) {
  static_assert(!SPLIT || T == 1, "replicas are for small one-owner-per-lane items");
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::NREC_T, NN = ND ? 3 : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  const int lane = threadIdx.x;
  const ListRange* const rg = a.ranges + it.first_range;

  int P = kListWave;                       // lanes per replica
  if (SPLIT) { P = 8; while (P < it.nt) P <<= 1; }
  const int nrep = kListWave / P, rep = lane / P;

  R xs[T][3], xn[T][NN], acc[T][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int sl = SPLIT ? (lane & (P - 1)) : (j * kListWave + lane);
    if (sl >= it.nt) sl = it.nt - 1;      // idle lanes repeat the last owner; never stored
    const int64_t s = it.t0 + sl;
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.xn[s * ND + k] : R(0);
#pragma unroll
    for (int k = 0; k < K0; k++) acc[j][k] = 0;
  }

  // cursor into the concatenated target sequence (wave-uniform): range r, offset o inside it
  int r = 0;
  int64_t o = 0;
  R px[3] = {0, 0, 0}, pw[K1];
#pragma unroll
  for (int k = 0; k < K1; k++) pw[k] = 0;
  // fetch the next (up to) 64 targets of the sequence into registers, lane i the i-th of them; returns how many
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
      for (int k = 0; k < 3; k++) px[k] = a.xt[mine * 3 + k];
#pragma unroll
      for (int k = 0; k < K1; k++) pw[k] = a.w[mine * K1 + k];
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
      pack_t_record<Ker, R, MODE>(rec, px, pw);
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
      if (SPLIT) {                         // replica `rep` takes targets rep, rep + nrep, ... of the tile
        const int cnt = (nt_cur + nrep - 1) / nrep;   // wave-uniform trip count; the tail of a short tile is predicated
        for (int i = 0; i < cnt; i++) {
          const int t = i * nrep + rep;
          if (t < nt_cur) one_target(t);
        }
      } else if (nt_cur == kListTile) {
#pragma unroll UnrollOf<T, Ker::K0>::value
        for (int t = 0; t < kListTile; t++) one_target(t);
      } else {
        for (int t = 0; t < nt_cur; t++) one_target(t);
      }
    };
    auto run_tile = [&](auto masked_tag) {   // a launch-uniform special case of the kernel (Helmholtz: real wavenumber) has its own loop
      if constexpr (KC::HAS_VARIANT) {
        if (K.variant(a.ctx) & 1) run_tile_v(masked_tag, std::integral_constant<int, 1>());   // (one-wave work items: the small tables, variants 0 / 1 only)
        else run_tile_v(masked_tag, std::integral_constant<int, 0>());
      } else {
        run_tile_v(masked_tag, std::integral_constant<int, 0>());
      }
    };
    bool repaired = true;
    tiles++;
    if (!always_masked) {
      run_tile(std::false_type());
      bool bad = K.tile_bad(a.ctx);
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][k]) <= max_finite<R>());
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 4 > tiles + 4) always_masked = true;   // mostly coincident points (tiny boxes): stop speculating
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][k] += tacc[j][k];
  }

  if (SPLIT) {                             // add the replicas' sums: lanes l, l ^ P, l ^ 2P, ... hold the same owner
    for (int off = P; off < kListWave; off <<= 1)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[0][k] += __shfl_xor(acc[0][k], off);
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int sl = SPLIT ? (lane & (P - 1)) : (j * kListWave + lane);
    finish_t_acc<Ker, R, MODE>(acc[j]);
    if (sl < it.nt && (!SPLIT || rep == 0)) {
      const int64_t s = it.t0 + sl;
#pragma unroll
      for (int k = 0; k < K0; k++) a.g_src[s * K0 + k] += acc[j][k] * a.scale;
    }
  }
}

// One PACKED work item: up to 64 / P small source ranges, P lanes x T owners per lane each (lists_packed_item in lists_kernel.hpp).  Group g = lane / P walks
// its own TARGET sequence S = P * SPL targets at a time through its slice of the LDS tile (slices one 16-byte word apart from a multiple of 32 banks); target
// indices are loaded two steps ahead, coordinates and weights one step ahead.  A step whose fetched target lies in the group's own owner range — possible only
// when r_src == r_trg is one array — runs masked at once.
template <class Ker, class R, int MODE, int P, int T, int SPL, class KC, class V>
__device__ __forceinline__ void lists_t_packed_item(const ListTArgs<R>& a, const ListItem& it, V* tile, const KC& K) {
  constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NREC = Ker::NREC_T, NN = ND ? 3 : 1;
  constexpr int VN = VecOf<R>::N;
  constexpr int NV = (NREC + VN - 1) / VN;
  constexpr int NRECP = NV * VN;
  constexpr int G = kListWave / P, S = P * SPL, SLICE = S * NV + 1;   // S targets per group and step (SPL per lane); 16-byte words per group slice (+ 1: bank spread)
  static_assert(G * SLICE <= kPackedTileWords(NV), "the packed slices fit the list kernel's LDS tile");
  const int lane = threadIdx.x, g = lane / P, i = lane % P;
  const bool live = g < it.nt;                              // (it.nt = groups of this item)
  const PackedGroup pg = a.groups[it.t0 + (live ? g : 0)];
  const int ntrg = live ? pg.nsrc : 0;                      // streamed targets of the group
  const bool self = (const void*)a.xs == (const void*)a.xt;

  R xs[T][3], xn[T][NN], acc[T][K0];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int sl = j * P + i;
    if (sl >= pg.nt) sl = pg.nt - 1;                        // idle slots repeat the last owner; never stored
    const int64_t s = pg.t0 + sl;
#pragma unroll
    for (int k = 0; k < 3; k++) xs[j][k] = a.xs[s * 3 + k];
#pragma unroll
    for (int k = 0; k < NN; k++) xn[j][k] = ND ? a.xn[s * ND + k] : R(0);
#pragma unroll
    for (int k = 0; k < K0; k++) acc[j][k] = 0;
  }
  int nmax = ntrg;                                          // the longest sequence of the wave decides the trip count
  for (int o = 32; o > 0; o >>= 1) { const int q = __shfl_xor(nmax, o); nmax = (q > nmax) ? q : nmax; }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  const int nsteps = (nmax + S - 1) / S;

  R px[SPL][3], pw[SPL][K1];
#pragma unroll
  for (int u = 0; u < SPL; u++) {
#pragma unroll
    for (int k = 0; k < 3; k++) px[u][k] = 0;
#pragma unroll
    for (int k = 0; k < K1; k++) pw[u][k] = 0;
  }
  // 32-bit throughout: the plan packs small owner ranges only while Nt * max(3, TrgDim) * sizeof(R) fits 32 bits (lists.hip), so a target's byte
  // offset into xt and w fits an unsigned 32-bit register
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t own_lo = (uint32_t)pg.t0, own_n = self ? (uint32_t)pg.nt : 0u;   // (own points exist only when the sources ARE the targets)
  const uint32_t* const flat_g = a.flat + pg.flat_off;
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
        const R* const qx = at(a.xt, trg[u] * (uint32_t)(3 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < 3; k++) px[u][k] = qx[k];
        const R* const qw = at(a.w, trg[u] * (uint32_t)(K1 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < K1; k++) pw[u][k] = qw[k];
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
        pack_t_record<Ker, R, MODE>(rec, px[u], pw[u]);
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

    R tacc[T][K0];
    const bool full = __all(cnt >= S);                      // wave-uniform: every group has a whole slice (all steps but the groups' last ones)
    auto run_step_v = [&](auto masked_tag, auto variant_tag) {
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
          const V q = slice[t * NV + v];
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
      if (full) {
#pragma unroll UnrollOf<T, Ker::K0>::value
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
        if (K.variant(a.ctx) & 1) run_step_v(masked_tag, std::integral_constant<int, 1>());
        else run_step_v(masked_tag, std::integral_constant<int, 0>());
      } else {
        run_step_v(masked_tag, std::integral_constant<int, 0>());
      }
    };
    bool repaired = true;
    if (!known_coincident) {
      run_step(std::false_type());
      bool bad = K.tile_bad(a.ctx);
#pragma unroll
      for (int j = 0; j < T; j++)
#pragma unroll
        for (int k = 0; k < K0; k++) bad |= !(fabs_(tacc[j][k]) <= max_finite<R>());
      repaired = __any(bad);
    }
    if (repaired) run_step(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++)
#pragma unroll
      for (int k = 0; k < K0; k++) acc[j][k] += tacc[j][k];
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int sl = j * P + i;
    finish_t_acc<Ker, R, MODE>(acc[j]);
    if (live && sl < pg.nt) {
      const int64_t s = pg.t0 + sl;
#pragma unroll
      for (int k = 0; k < K0; k++) a.g_src[s * K0 + k] += acc[j][k] * a.scale;
    }
  }
}

// The item shapes are the forward kernel's: more than 64 owners two per lane, 33..64 one per lane, fewer (when not packed) replicas of 8..32 lanes; the four
// packed classes 8 x 1, 8 x 2, 16 x 2 and 32 x 2 owners.  The LDS tile is sized from NREC_T (the traction kernel streams 10 reals against 6 forward).
template <class Ker, class R, int MODE>
__global__ void __launch_bounds__(kListWave) lists_transpose_kernel(const ListTArgs<R> a) {
  using V = typename VecOf<R>::type;
  constexpr int NV = (Ker::NREC_T + VecOf<R>::N - 1) / VecOf<R>::N;
  __shared__ V tile[kPackedTileWords(NV)];
  using KC = typename Ker::template Consts<R>;
  __shared__ double kscratch[KC::LDS_DOUBLES > 0 ? KC::LDS_DOUBLES : 1];
  const KC K = make_consts<KC>(kscratch, a.ctx, MODE);
  // XCD x walks its own share of the item list, as in lists_kernel: the items of one source box and of its neighbours meet in one L2
  const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;
  if (j >= a.xcd_first[xcd + 1] - a.xcd_first[xcd]) return;
  const ListItem it = a.items[a.xcd_first[xcd] + j];
  if (it.nranges < 0) {      // packed small source ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) lists_t_packed_item<Ker, R, MODE, 8, 1, 2>(a, it, tile, K);
    else if (cls == 1) lists_t_packed_item<Ker, R, MODE, 8, 2, 2>(a, it, tile, K);
    else if (cls == 2) lists_t_packed_item<Ker, R, MODE, 16, 2, 2>(a, it, tile, K);
    else lists_t_packed_item<Ker, R, MODE, 32, 2, 1>(a, it, tile, K);
    return;
  }
  if (it.nt > kListWave) lists_t_item<Ker, R, MODE, 2, false>(a, it, tile, K);
  else if (it.nt > kListWave / 2) lists_t_item<Ker, R, MODE, 1, false>(a, it, tile, K);
  else lists_t_item<Ker, R, MODE, 1, true>(a, it, tile, K);
}

}  // namespace sctl_amd
