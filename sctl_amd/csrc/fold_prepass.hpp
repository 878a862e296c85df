// What the fp64 tile-centred single layer decides about a source ONCE PER LAUNCH instead of once per (wave, tile): the class of its density and
// where its record goes (centered_kernel.hpp: fold_prepass_kernel writes the records, the FOLD branch of centered_kernel reads them).
//
// The kernel folds the density into its far records, k = 1 / f^2 (CenteredFxU), and keeps the far sources of either sign apart because the sign
// is an instruction modifier, not data.  Neither the sign nor k depends on the wave's centre, so the pre-pass groups the sources of a split by sign
// into tiles of 64 records {x, y, z, k} that hold one sign only:
//   positive records   rank i  ->  slot i                                              (tiles from the front of the split's area)
//   negative records   rank i  ->  slot cap - 64 (i / 64 + 1) + i % 64                 (tiles from the back; cap = chunk + 128)
// The rank of a source is the number of sources of its class before it in the split, so the grouping is a pure function of the densities.  The
// last tile of either sign is padded with records of k = 0, which no real record has.  f == 0 is dropped (contributes exactly 0).  A density that
// is not finite, or whose k lies outside [2^-900, 2^900] — no |x_s'|^2 in [2^-300, 2^300] could then bring k |x_s'|^2 into the kernel's band
// [2^-600, 2^600] — goes to the split's exception list and takes the exact pair for every wave.
//
// Plain code with no HIP types: a host program includes this header as it is (tests/cpp/fold_prepass_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCTL_AMD_FOLD_HD __host__ __device__
#else
#define SCTL_AMD_FOLD_HD
#endif

namespace sctl_amd {

constexpr int kFoldTile = 64;   // records per tile (= kWaveTile)

// 1: positive tiles, -1: negative tiles, 0: dropped, 2: exception list.  k = 1 / f^2 where the class is +-1.
SCTL_AMD_FOLD_HD inline int fold_prep_class(double f, double& k) {
  k = 0;
  if (f == 0.0) return 0;
  const double kk = 1.0 / (f * f);   // f * f over- or underflows to inf or 0 beyond ~1e+-154: kk is then 0 or inf; NaN fails the comparisons
  if (!(kk >= 0x1p-900 && kk <= 0x1p900)) return 2;
  k = kk;
  return f > 0.0 ? 1 : -1;
}

// record slots of a split's area
SCTL_AMD_FOLD_HD inline int64_t fold_prep_cap(int64_t chunk) { return chunk + 2 * kFoldTile; }
SCTL_AMD_FOLD_HD inline int64_t fold_prep_tiles(int64_t n) { return (n + kFoldTile - 1) / kFoldTile; }
SCTL_AMD_FOLD_HD inline int64_t fold_prep_tile_base(bool neg, int64_t tile, int64_t cap) { return neg ? cap - (tile + 1) * kFoldTile : tile * kFoldTile; }
SCTL_AMD_FOLD_HD inline int64_t fold_prep_slot(bool neg, int64_t rank, int64_t cap) { return fold_prep_tile_base(neg, rank / kFoldTile, cap) + rank % kFoldTile; }

// The pre-pass block of a launch with `splits` splits of `chunk` sources (byte offsets, each a multiple of 256):
//   hdr  int32[splits][4]        {positive tiles, negative tiles, exceptions, 0}
//   rec  double[splits][cap][4]  {x, y, z, k}
//   idx  uint32[splits][cap]     the record's source, counted from the split's first (read for the few sources a wave finds near)
//   exc  uint32[splits][chunk]   the exceptions' sources, likewise
struct FoldPrepLayout {
  int64_t cap, rec, idx, exc, bytes;
  static SCTL_AMD_FOLD_HD int64_t pad(int64_t b) { return (b + 255) & ~(int64_t)255; }
  SCTL_AMD_FOLD_HD FoldPrepLayout(int64_t splits, int64_t chunk) {
    cap = fold_prep_cap(chunk);
    rec = pad(splits * 4 * (int64_t)sizeof(int32_t));
    idx = rec + pad(splits * cap * 4 * (int64_t)sizeof(double));
    exc = idx + pad(splits * cap * (int64_t)sizeof(uint32_t));
    bytes = exc + pad(splits * chunk * (int64_t)sizeof(uint32_t));
  }
};

}  // namespace sctl_amd
