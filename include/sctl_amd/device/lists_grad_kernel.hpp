// Geometry gradients of a kernel sum over P2P lists for gfx950: with target weights w, L = sum_lists <w_trg, A_list v_src> and the pair's scalar
// phi_ts = sum_k0 sum_k1 w[t,k1] U(x_t - x_s, n_s)[k0][k1] f[s,k0] (ukernels.hpp: pair_g),
//     g_trg[t,j] +=  scale * sum_{l : t in target range l} sum_{s in source range l} d phi_ts / d d_j      SIDE 0: the TARGETS own the output, the sources stream
//     g_src[s,j] += -scale * sum_{l : s in source range l} sum_{t in target range l} d phi_ts / d d_j      SIDE 1: the SOURCES own the outputs, the targets stream
//     g_nrm[s,j] +=  scale * sum_{l : s in source range l} sum_{t in target range l} d phi_ts / d n_j      SIDE 1, kernels with a normal, out of the same pass
// It relates to eval_grad_kernel.hpp as lists_kernel.hpp relates to eval_kernel.hpp: the pair, the sign conventions (d = x_trg - x_src on both sides, the
// minus of g_src once when the sums leave the registers, a coincident pair contributes 0, outputs are accumulated into) and the plain streamed records
// ({x_s, n_s, f_s} on side 0, {x_t, w_t} on side 1) are the all-pairs gradient's; the work decomposition is the list kernels'.  SIDE 0 walks the plan's
// FORWARD work list, SIDE 1 its TRANSPOSE work list, unchanged (ListItem, ListRange, PackedGroup, the flat index list; all seven item shapes):
//   * one wave64 per work item, XCD-owned shares (xcd_first); every owner is held by one lane of one item, sums are kept in registers in list order and
//     written once: deterministic, no atomics, no workspace;
//   * a lane holds per owner its coordinates, w[K1] (SIDE 0) or the normal and f[K0] (SIDE 1), and 3 sums (+ 3 for the normal gradient);
//   * a tile (a packed step) runs unmasked into per-tile sums; one compare over the 3 (+ 3) sums finds a coincident pair (inf / NaN) and the tile is run
//     again masked; an item that keeps being repaired stops speculating (always_masked); a packed step known to hold its group's own points (the caller's
//     sources ARE its targets: one array) is run masked at once.
// The walkers below are lists_item / lists_packed_item of lists_kernel.hpp written out again for the gradient — an owner payload, two outputs, the plain
// record — and not two more policies of those walkers: lists_kernel.hpp is untouched, so no shipped list kernel can change in registers.
// An item the plan cut for two owners per lane holds both: every (kernel, precision, mode, side) compiles to ScratchSize 0 and at most 256 vector registers
// that way (DESIGN.md §4.17 has the table, tests/test_lists_grad_cpu.py holds the units to it), so no form runs its owners in two halves.
#pragma once
#include "lists_kernel.hpp"

namespace sctl_amd {

template <class R> struct ListGArgs {
  int32_t xcd_first[9];   // items [xcd_first[x], xcd_first[x + 1]) are the share of XCD x
  const ListItem* items;  // t0, nt: the item's owners
  const ListRange* ranges;   // s0, ns: streamed ranges
  const R* xo;      // [No*3]   owners' coordinates: r_trg (SIDE 0), r_src (SIDE 1)
  const R* xst;     // [Nst*3]  streamed coordinates
  const R* xn;      // source normals or null: the streamed set's [Nst*ND] (SIDE 0), the owners' [No*ND] (SIDE 1)
  const R* f;       // source densities: [Nst*K0] (SIDE 0), [No*K0] (SIDE 1)
  const R* w;       // target weights:   [No*K1] (SIDE 0), [Nst*K1] (SIDE 1)
  R* g;             // [No*3] coordinate gradient, accumulated into; null: not stored
  R* gn;            // [No*3] normal gradient (SIDE 1, ND > 0), likewise
  R scale;
  KerCtx ctx;
  const PackedGroup* groups;   // packed items only
  const uint32_t* flat;        // their streamed sequences: indices into the streamed arrays
};

// What follows from (kernel, precision, side) alone
template <class Ker, class R, int SIDE> struct ListGradForm {
  static constexpr int K0 = Ker::K0, K1 = Ker::K1, ND = Ker::ND, NN = ND ? 3 : 1;
  static constexpr bool WANT_N = (SIDE == 1 && ND > 0);
  static constexpr int NF = (SIDE == 1) ? K0 : 1, NW = (SIDE == 0) ? K1 : 1;   // what an owner holds of f and of w (the other is a placeholder)
  static constexpr int NPAY = (SIDE == 0) ? ND + K0 : K1;                      // what a streamed record holds after its coordinates
  static constexpr int VN = VecOf<R>::N;
  static constexpr int NV = (3 + NPAY + VN - 1) / VN;                          // 16-byte LDS words per record
  static constexpr int NRECP = NV * VN;
};

// owner oi: its coordinates and w (SIDE 0) or normal and f (SIDE 1)
template <class Ker, class R, int SIDE, class F = ListGradForm<Ker, R, SIDE>>
__device__ __forceinline__ void lists_grad_load_owner(const ListGArgs<R>& a, int64_t oi, R (&x)[3], R (&n)[F::NN], R (&f)[F::NF], R (&w)[F::NW]) {
#pragma unroll
  for (int k = 0; k < 3; k++) x[k] = a.xo[oi * 3 + k];
#pragma unroll
  for (int k = 0; k < F::NN; k++) n[k] = F::WANT_N ? a.xn[oi * F::ND + k] : R(0);
  if constexpr (SIDE == 1) {
#pragma unroll
    for (int k = 0; k < F::K0; k++) f[k] = a.f[oi * F::K0 + k];
    w[0] = 0;
  } else {
#pragma unroll
    for (int k = 0; k < F::K1; k++) w[k] = a.w[oi * F::K1 + k];
    f[0] = 0;
  }
}

// a staged point (coordinates sx, payload sp) as a record of NV words at dst
template <class Ker, class R, int SIDE, class V, class F = ListGradForm<Ker, R, SIDE>>
__device__ __forceinline__ void lists_grad_stage(V* dst, const R (&sx)[3], const R (&sp)[F::NPAY]) {
  R rec[F::NRECP] = {};
  rec[0] = sx[0]; rec[1] = sx[1]; rec[2] = sx[2];
#pragma unroll
  for (int k = 0; k < F::NPAY; k++) rec[3 + k] = sp[k];
#pragma unroll
  for (int v = 0; v < F::NV; v++) {
    V q;
#pragma unroll
    for (int e = 0; e < F::VN; e++) q[e] = rec[v * F::VN + e];
    dst[v] = q;
  }
}

// the record at src against the lane's T owners: pair_g with d = x_trg - x_src on both sides, exactly as eval_grad_kernel calls it
template <class Ker, class R, int MODE, int SIDE, bool MASKED, int VARIANT, int T, class V, class KC, class F = ListGradForm<Ker, R, SIDE>>
__device__ __forceinline__ void lists_grad_point(R (&G)[T][3], R (&N)[T][F::NN], const R (&xo)[T][3], const R (&on)[T][F::NN], const R (&of)[T][F::NF],
                                                 const R (&ow)[T][F::NW], const V* src, const KerCtx& ctx, const KC& K) {
  R rec[F::NRECP];
#pragma unroll
  for (int v = 0; v < F::NV; v++) {
    const V q = src[v];
#pragma unroll
    for (int e = 0; e < F::VN; e++) rec[v * F::VN + e] = q[e];
  }
  // the streamed point's share of the pair's inputs
  R st_n[F::NN], st_f[SIDE == 0 ? F::K0 : 1], st_w[SIDE == 1 ? F::K1 : 1];
  st_n[0] = 0; st_f[0] = 0; st_w[0] = 0;
  if constexpr (SIDE == 0) {
#pragma unroll
    for (int k = 0; k < F::ND; k++) st_n[k] = rec[3 + k];
#pragma unroll
    for (int k = 0; k < F::K0; k++) st_f[k] = rec[3 + F::ND + k];
  } else {
#pragma unroll
    for (int k = 0; k < F::K1; k++) st_w[k] = rec[3 + k];
  }
  auto pair = [&](R (&Gj)[3], R (&Nj)[F::NN], const R (&d)[3], const R (&n)[F::NN], const R (&f)[F::K0], const R (&w)[F::K1]) {
    if constexpr (KC::HAS_VARIANT) Ker::template pair_g<R, MODE, MASKED, VARIANT, F::WANT_N>(Gj, Nj, d, n, f, w, ctx, K);
    else Ker::template pair_g<R, MODE, MASKED, F::WANT_N>(Gj, Nj, d, n, f, w, ctx, K);
  };
#pragma unroll
  for (int j = 0; j < T; j++) {
    if constexpr (SIDE == 0) {
      const R d[3] = {xo[j][0] - rec[0], xo[j][1] - rec[1], xo[j][2] - rec[2]};
      pair(G[j], N[j], d, st_n, st_f, ow[j]);
    } else {
      const R d[3] = {rec[0] - xo[j][0], rec[1] - xo[j][1], rec[2] - xo[j][2]};
      pair(G[j], N[j], d, on[j], of[j], st_w);
    }
  }
}

// one compare over the 3 (+ 3) per-tile sums of every owner: a coincident pair left inf / NaN in them
template <bool WANT_N, class R, int T, int NN> __device__ __forceinline__ bool lists_grad_bad(const R (&G)[T][3], const R (&N)[T][NN]) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < T; j++) {
#pragma unroll
    for (int k = 0; k < 3; k++) bad |= !(fabs_(G[j][k]) <= max_finite<R>());
    if constexpr (WANT_N) {
#pragma unroll
      for (int k = 0; k < 3; k++) bad |= !(fabs_(N[j][k]) <= max_finite<R>());
    }
  }
  return bad;
}

// the sums of owner oi leave the registers: g_src takes its minus sign here (d d / d x_src = -1)
template <class Ker, class R, int SIDE, class F = ListGradForm<Ker, R, SIDE>>
__device__ __forceinline__ void lists_grad_store(const ListGArgs<R>& a, int64_t oi, const R (&G)[3], const R (&N)[F::NN]) {
  if (a.g) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.g[oi * 3 + k] += ((SIDE == 1) ? -G[k] : G[k]) * a.scale;
  }
  if constexpr (F::WANT_N) {
    if (a.gn) {
#pragma unroll
      for (int k = 0; k < 3; k++) a.gn[oi * 3 + k] += N[k] * a.scale;
    }
  }
}

// One work item with T owners per lane: lists_item of lists_kernel.hpp for the gradient.  Slot j of the lane is owner j * 64 + lane of the item.
// SPLIT: at most 32 owners, 64 / P replicas of P lanes, each taking every (64 / P)-th point
// of a tile; their sums are added with a butterfly of lane shuffles (a fixed order).
template <class Ker, class R, int MODE, int SIDE, int T, bool SPLIT, class KC, class V>
__device__ __forceinline__ void lists_grad_item(const ListGArgs<R>& a, const ListItem& it, V* tile, const KC& K) {
  static_assert(!SPLIT || T == 1, "replicas are for small one-owner-per-lane items");
  using F = ListGradForm<Ker, R, SIDE>;
  constexpr int NN = F::NN, NPAY = F::NPAY, NV = F::NV;
  const int lane = threadIdx.x;
  const ListRange* const rg = a.ranges + it.first_range;

  int P = kListWave;                       // lanes per replica
  if (SPLIT) { P = 8; while (P < it.nt) P <<= 1; }
  const int nrep = kListWave / P, rep = lane / P;

  R xo[T][3], on[T][NN], of[T][F::NF], ow[T][F::NW], accG[T][3], accN[T][NN];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int ol = SPLIT ? (lane & (P - 1)) : (j * kListWave + lane);
    if (ol >= it.nt) ol = it.nt - 1;      // idle lanes repeat the last owner; never stored
    lists_grad_load_owner<Ker, R, SIDE>(a, it.t0 + ol, xo[j], on[j], of[j], ow[j]);
#pragma unroll
    for (int k = 0; k < 3; k++) accG[j][k] = 0;
#pragma unroll
    for (int k = 0; k < NN; k++) accN[j][k] = 0;
  }

  // cursor into the concatenated streamed sequence (wave-uniform): range r, offset o inside it
  int r = 0;
  int64_t o = 0;
  R sx[3] = {0, 0, 0}, sp[NPAY];
#pragma unroll
  for (int k = 0; k < NPAY; k++) sp[k] = 0;
  // fetch the next (up to) 64 points of the sequence into registers, lane i the i-th of them; returns how many
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
      for (int k = 0; k < 3; k++) sx[k] = a.xst[mine * 3 + k];
      if constexpr (SIDE == 0) {
#pragma unroll
        for (int k = 0; k < F::ND; k++) sp[k] = a.xn[mine * F::ND + k];
#pragma unroll
        for (int k = 0; k < F::K0; k++) sp[F::ND + k] = a.f[mine * F::K0 + k];
      } else {
#pragma unroll
        for (int k = 0; k < F::K1; k++) sp[k] = a.w[mine * F::K1 + k];
      }
    }
    return fill;
  };

  int repairs = 0, tiles = 0;
  bool always_masked = false;
  int ns = fetch();
  while (ns > 0) {
    __syncthreads();   // previous tile fully consumed
    if (lane < ns) lists_grad_stage<Ker, R, SIDE>(tile + lane * NV, sx, sp);
    const int ns_cur = ns;
    ns = fetch();      // loads for the next tile are in flight during this tile's arithmetic
    __syncthreads();

    R tG[T][3], tN[T][NN];
    auto run_tile_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) tG[j][k] = 0;
#pragma unroll
        for (int k = 0; k < NN; k++) tN[j][k] = 0;
      }
      auto one_point = [&](int s) { lists_grad_point<Ker, R, MODE, SIDE, MASKED, VARIANT, T>(tG, tN, xo, on, of, ow, tile + s * NV, a.ctx, K); };
      if (SPLIT) {                         // replica `rep` takes points rep, rep + nrep, ... of the tile
        const int cnt = (ns_cur + nrep - 1) / nrep;   // wave-uniform trip count; the tail of a short tile is predicated
        for (int i = 0; i < cnt; i++) {
          const int s = i * nrep + rep;
          if (s < ns_cur) one_point(s);
        }
      } else if (ns_cur == kListTile) {
#pragma unroll 2
        for (int s = 0; s < kListTile; s++) one_point(s);
      } else {
        for (int s = 0; s < ns_cur; s++) one_point(s);
      }
    };
    auto run_tile = [&](auto masked_tag) {   // (one-wave work items: the small tables, variants 0 / 1 only, as in the other list kernels)
      if constexpr (KC::HAS_VARIANT) {
        if (K.variant(a.ctx) & 1) run_tile_v(masked_tag, std::integral_constant<int, 1>());
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
      bad |= lists_grad_bad<F::WANT_N>(tG, tN);
      repaired = __any(bad);                 // wave-uniform
      if (repaired && (++repairs) * 4 > tiles + 4) always_masked = true;   // mostly coincident points (tiny boxes): stop speculating
    }
    if (repaired) run_tile(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++) {
#pragma unroll
      for (int k = 0; k < 3; k++) accG[j][k] += tG[j][k];
      if constexpr (F::WANT_N) {
#pragma unroll
        for (int k = 0; k < 3; k++) accN[j][k] += tN[j][k];
      }
    }
  }

  if (SPLIT) {                             // add the replicas' sums: lanes l, l ^ P, l ^ 2P, ... hold the same owner
    for (int off = P; off < kListWave; off <<= 1) {
#pragma unroll
      for (int k = 0; k < 3; k++) accG[0][k] += __shfl_xor(accG[0][k], off);
      if constexpr (F::WANT_N) {
#pragma unroll
        for (int k = 0; k < 3; k++) accN[0][k] += __shfl_xor(accN[0][k], off);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int ol = SPLIT ? (lane & (P - 1)) : (j * kListWave + lane);
    if (ol < it.nt && (!SPLIT || rep == 0)) lists_grad_store<Ker, R, SIDE>(a, it.t0 + ol, accG[j], accN[j]);
  }
}

// One PACKED work item: lists_packed_item of lists_kernel.hpp for the gradient.  Up to 64 / P small owner ranges, P lanes x T owners per lane each; slot j of
// a lane is owner j * P + i of its group.  Points are fetched one step ahead, their indices two steps ahead, by 32-bit byte offsets from scalar bases: the plan packs small
// ranges only while every streamed array of its direction is under 4 GB, and the gradient streams no wider array than that direction's kernel does — r_src,
// n_src, v_src on side 0 (FORWARD), r_trg, w_trg on side 1 (TRANSPOSE).
template <class Ker, class R, int MODE, int SIDE, int P, int T, int SPL, class KC, class V>
__device__ __forceinline__ void lists_grad_packed_item(const ListGArgs<R>& a, const ListItem& it, V* tile, const KC& K) {
  using F = ListGradForm<Ker, R, SIDE>;
  constexpr int NN = F::NN, NPAY = F::NPAY, NV = F::NV;
  constexpr int G = kListWave / P, S = P * SPL, SLICE = S * NV + 1;   // S points per group and step (SPL per lane); 16-byte words per group slice (+ 1: bank spread)
  static_assert(G * SLICE <= kPackedTileWords(NV), "the packed slices fit the kernel's LDS tile");
  const int lane = threadIdx.x, g = lane / P, i = lane % P;
  const bool live = g < it.nt;                              // (it.nt = groups of this item)
  const PackedGroup pg = a.groups[it.t0 + (live ? g : 0)];
  const int nstr = live ? pg.nsrc : 0;                      // streamed points of the group
  const bool self = (const void*)a.xst == (const void*)a.xo;

  R xo[T][3], on[T][NN], of[T][F::NF], ow[T][F::NW], accG[T][3], accN[T][NN];
#pragma unroll
  for (int j = 0; j < T; j++) {
    int ol = j * P + i;
    if (ol >= pg.nt) ol = pg.nt - 1;                        // idle slots repeat the last owner; never stored
    lists_grad_load_owner<Ker, R, SIDE>(a, pg.t0 + ol, xo[j], on[j], of[j], ow[j]);
#pragma unroll
    for (int k = 0; k < 3; k++) accG[j][k] = 0;
#pragma unroll
    for (int k = 0; k < NN; k++) accN[j][k] = 0;
  }
  int nmax = nstr;                                          // the longest sequence of the wave decides the trip count
  for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(nmax, o); nmax = (w > nmax) ? w : nmax; }
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  const int nsteps = (nmax + S - 1) / S;

  R sx[SPL][3], sp[SPL][NPAY];
#pragma unroll
  for (int u = 0; u < SPL; u++) {
#pragma unroll
    for (int k = 0; k < 3; k++) sx[u][k] = 0;
#pragma unroll
    for (int k = 0; k < NPAY; k++) sp[u][k] = 0;
  }
  constexpr uint32_t kNone = 0xffffffffu;
  const uint32_t own_lo = (uint32_t)pg.t0, own_n = self ? (uint32_t)pg.nt : 0u;   // (own points exist only when the sources ARE the targets)
  const uint32_t* const flat_g = a.flat + pg.flat_off;
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
        const R* const px = at(a.xst, str[u] * (uint32_t)(3 * sizeof(R)));
#pragma unroll
        for (int k = 0; k < 3; k++) sx[u][k] = px[k];
        if constexpr (SIDE == 0) {
          if constexpr (F::ND > 0) {
            const R* const pn = at(a.xn, str[u] * (uint32_t)(F::ND * sizeof(R)));
#pragma unroll
            for (int k = 0; k < F::ND; k++) sp[u][k] = pn[k];
          }
          const R* const pf = at(a.f, str[u] * (uint32_t)(F::K0 * sizeof(R)));
#pragma unroll
          for (int k = 0; k < F::K0; k++) sp[u][F::ND + k] = pf[k];
        } else {
          const R* const pw = at(a.w, str[u] * (uint32_t)(F::K1 * sizeof(R)));
#pragma unroll
          for (int k = 0; k < F::K1; k++) sp[u][k] = pw[k];
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
    for (int u = 0; u < SPL; u++)
      if (u * P + i < cnt) lists_grad_stage<Ker, R, SIDE>(slice + (u * P + i) * NV, sx[u], sp[u]);
    if (step + 1 < nsteps) fetch(step + 1);
    __syncthreads();

    R tG[T][3], tN[T][NN];
    const bool full = __all(cnt >= S);                      // wave-uniform: every group has a whole slice (all steps but the groups' last ones)
    auto run_step_v = [&](auto masked_tag, auto variant_tag) {
      constexpr bool MASKED = decltype(masked_tag)::value;
      constexpr int VARIANT = decltype(variant_tag)::value;
      K.begin_tile();
#pragma unroll
      for (int j = 0; j < T; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) tG[j][k] = 0;
#pragma unroll
        for (int k = 0; k < NN; k++) tN[j][k] = 0;
      }
      auto one_point = [&](int s) { lists_grad_point<Ker, R, MODE, SIDE, MASKED, VARIANT, T>(tG, tN, xo, on, of, ow, slice + s * NV, a.ctx, K); };
      if (full) {
#pragma unroll 2
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
      bad |= lists_grad_bad<F::WANT_N>(tG, tN);
      repaired = __any(bad);
    }
    if (repaired) run_step(std::true_type());
#pragma unroll
    for (int j = 0; j < T; j++) {
#pragma unroll
      for (int k = 0; k < 3; k++) accG[j][k] += tG[j][k];
      if constexpr (F::WANT_N) {
#pragma unroll
        for (int k = 0; k < 3; k++) accN[j][k] += tN[j][k];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < T; j++) {
    const int ol = j * P + i;
    if (live && ol < pg.nt) lists_grad_store<Ker, R, SIDE>(a, pg.t0 + ol, accG[j], accN[j]);
  }
}

// The dispatch of the list kernels over the plan's seven item shapes.
template <class Ker, class R, int MODE, int SIDE>
__global__ void __launch_bounds__(kListWave) lists_grad_kernel(const ListGArgs<R> a) {
  using V = typename VecOf<R>::type;
  constexpr int NV = ListGradForm<Ker, R, SIDE>::NV;
  __shared__ V tile[kPackedTileWords(NV)];   // 64 records for the one-range items; the packed items' slices: 8 x (16 records + 1 word)
  using KC = typename Ker::template Consts<R>;
  __shared__ double kscratch[KC::LDS_DOUBLES > 0 ? KC::LDS_DOUBLES : 1];
  const KC K = make_consts<KC>(kscratch, a.ctx, MODE);
  const int xcd = blockIdx.x % 8, j = blockIdx.x / 8;      // XCD x walks its share of the item list (as the other list kernels do)
  if (j >= a.xcd_first[xcd + 1] - a.xcd_first[xcd]) return;
  const ListItem it = a.items[a.xcd_first[xcd] + j];
  if (it.nranges < 0) {      // packed small owner ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) lists_grad_packed_item<Ker, R, MODE, SIDE, 8, 1, 2>(a, it, tile, K);
    else if (cls == 1) lists_grad_packed_item<Ker, R, MODE, SIDE, 8, 2, 2>(a, it, tile, K);
    else if (cls == 2) lists_grad_packed_item<Ker, R, MODE, SIDE, 16, 2, 2>(a, it, tile, K);
    else lists_grad_packed_item<Ker, R, MODE, SIDE, 32, 2, 1>(a, it, tile, K);
    return;
  }
  if (it.nt > kListWave) lists_grad_item<Ker, R, MODE, SIDE, 2, false>(a, it, tile, K);
  else if (it.nt > kListWave / 2) lists_grad_item<Ker, R, MODE, SIDE, 1, false>(a, it, tile, K);
  else lists_grad_item<Ker, R, MODE, SIDE, 1, true>(a, it, tile, K);
}

// ---- launch table: one per built-in kernel (sctl_amd/csrc/inst_lg_<Kernel>.hip), inside the library; none for plugin kernels ----------
template <class R> using ListsGLaunch = void (*)(const ListGArgs<R>&, int64_t nblocks, hipStream_t);
struct ListsGradEntry {
  double grad_factor[3];            // pair_g() of mode m accumulates grad_factor[m] x the derivative (GradFactorOf)
  ListsGLaunch<double> f64[3][2];   // [mode][side]
  ListsGLaunch<float> f32[3][2];    // modes 0 and 1 (mode 2 aliases mode 1)
};
template <class Ker, class R, int MODE, int SIDE> void launch_lists_grad(const ListGArgs<R>& a, int64_t nblocks, hipStream_t st) {
  hipLaunchKernelGGL((lists_grad_kernel<Ker, R, MODE, SIDE>), dim3((unsigned)nblocks), dim3(kListWave), 0, st, a);
}
template <class Ker> ListsGradEntry make_lists_grad_entry() {
  ListsGradEntry e{};
  for (int m = 0; m < 3; m++) e.grad_factor[m] = GradFactorOf<Ker>::value(m);
#define SCTL_AMD_ROW_LG(R, arr, M, MM) arr[M][0] = launch_lists_grad<Ker, R, MM, 0>; arr[M][1] = launch_lists_grad<Ker, R, MM, 1>;
  SCTL_AMD_ROW_LG(double, e.f64, 0, 0) SCTL_AMD_ROW_LG(double, e.f64, 1, 1) SCTL_AMD_ROW_LG(double, e.f64, 2, 2)
  SCTL_AMD_ROW_LG(float, e.f32, 0, 0) SCTL_AMD_ROW_LG(float, e.f32, 1, 1) SCTL_AMD_ROW_LG(float, e.f32, 2, 1)
#undef SCTL_AMD_ROW_LG
  return e;
}

// defined in inst_lg_*.hip
const ListsGradEntry& lists_grad_Laplace3D_FxU();
const ListsGradEntry& lists_grad_Laplace3D_DxU();
const ListsGradEntry& lists_grad_Laplace3D_FxdU();
const ListsGradEntry& lists_grad_Stokes3D_FxU();
const ListsGradEntry& lists_grad_Stokes3D_DxU();
const ListsGradEntry& lists_grad_Stokes3D_FxT();
const ListsGradEntry& lists_grad_Stokes3D_FSxU();
const ListsGradEntry& lists_grad_Stokes3D_FxUP();
const ListsGradEntry& lists_grad_Laplace3D_FDxUdU();
const ListsGradEntry& lists_grad_Helmholtz3D_FxU();

}  // namespace sctl_amd
