// Transposed batched list evaluation for gfx950: the adjoint of lists_kernel's sum over the same lists,
//     g[s,k0] += scale * sum_{l : s in source range l} sum_{t in target range l} sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[t,k1],
// in ONE launch.  It relates to lists_kernel.hpp as eval_transpose_kernel.hpp relates to eval_kernel.hpp: the scheme is the forward list kernel's
//  with the roles of the two point sets exchanged, and so is the code: lists_item and lists_packed_item of
// lists_kernel.hpp with the policy DirTrans (dir.hpp).  This file holds the arguments and the kernel's name.
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

// The item shapes are the forward kernel's.  The LDS tile is sized from NREC_T (the traction kernel streams 10 reals against 6 forward).
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
  if (it.nranges < 0) {      // packed small owner ranges
    const int cls = -1 - it.nranges;
    if (cls == 0) lists_packed_item<DirTrans, Ker, R, MODE, 8, 1, 2>(a, it, tile, K);
    else if (cls == 1) lists_packed_item<DirTrans, Ker, R, MODE, 8, 2, 2>(a, it, tile, K);
    else if (cls == 2) lists_packed_item<DirTrans, Ker, R, MODE, 16, 2, 2>(a, it, tile, K);
    else lists_packed_item<DirTrans, Ker, R, MODE, 32, 2, 1>(a, it, tile, K);
    return;
  }
  if (it.nt > kListWave) lists_item<DirTrans, Ker, R, MODE, 2, false>(a, it, tile, K);
  else if (it.nt > kListWave / 2) lists_item<DirTrans, Ker, R, MODE, 1, false>(a, it, tile, K);
  else lists_item<DirTrans, Ker, R, MODE, 1, true>(a, it, tile, K);
}

}  // namespace sctl_amd
