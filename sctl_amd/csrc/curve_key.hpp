// The sort key that orders the targets of the tile-centred kernels (centered.hip): the index of a point's cell along the 3-D HILBERT curve
// over the bounding box of the points, 21 bits per axis, 63 bits in all.
//
// Why Hilbert and not the bit interleave (Morton, Z-curve) of rounds 1-5: a wave takes 64 T CONSECUTIVE targets of the order and every source
// within twice their radius takes the exact pair.  Consecutive cells of the Hilbert curve share a face, so a range of the order is a connected
// chain of cells; the Z-curve jumps — from the end of one octant to the start of the next, at every level — and a range that straddles a jump
// has a bounding box many times its share of the volume.  Near share per 256-target cluster at 2^20 uniform points: DESIGN.md §4.2.
//
// Plain integer code with no HIP types: a host program includes this header as it is (tests/cpp/curve_key_main.cpp, tools/near_share.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCTL_AMD_CURVE_HD __host__ __device__
#else
#define SCTL_AMD_CURVE_HD
#endif

namespace sctl_amd {

constexpr int kCurveBits = 21;   // per axis: 3 x 21 = 63 bits, what the radix sort is told to look at

// the low 21 bits of v, one in every third bit of the result
SCTL_AMD_CURVE_HD inline uint64_t curve_spread21(uint64_t v) {
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x1f00000000ffffull;
  v = (v | (v << 16)) & 0x1f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

// Hilbert index of the cell (x0, x1, x2), each coordinate below 2^bits (1 <= bits <= 21), as a number below 2^(3 bits).  J. Skilling,
// "Programming the Hilbert curve" (AIP Conf. Proc. 707, 2004), the transpose form: undo the rotations and reflections level by level from the
// top (per axis one test and one masked exchange or inversion), Gray-encode, interleave — x0's bit is the most significant of each triple.
SCTL_AMD_CURVE_HD inline uint64_t hilbert_key3(uint32_t x0, uint32_t x1, uint32_t x2, int bits = kCurveBits) {
  uint32_t X[3] = {x0, x1, x2};
  const uint32_t M = 1u << (bits - 1);
  for (uint32_t Q = M; Q > 1; Q >>= 1) {
    const uint32_t P = Q - 1;
    for (int i = 0; i < 3; i++) {
      if (X[i] & Q) X[0] ^= P;
      else { const uint32_t t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
    }
  }
  X[1] ^= X[0];
  X[2] ^= X[1];
  uint32_t t = 0;
  for (uint32_t Q = M; Q > 1; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1;
  return (curve_spread21(X[0] ^ t) << 2) | (curve_spread21(X[1] ^ t) << 1) | curve_spread21(X[2] ^ t);
}

// A coordinate as a cell number in [0, 2^21) of the box [lo, lo + w].  An axis of zero extent (w == 0: all points on a plane, a line, or one point)
// gives cell 0 for every point; a NaN coordinate gives 0 (every comparison fails), and so does any coordinate once the box has an infinite side
// (x / inf = 0, inf / inf = NaN): a valid cell somewhere harmless in the order — the kernel's far test then fails for the whole wave (a non-finite
// centre) and its pairs take the exact path.
SCTL_AMD_CURVE_HD inline uint32_t curve_cell(double x, double lo, double w) {
  const double top = 2097151.0;   // 2^21 - 1
  const double q = (w > 0) ? (x - lo) / w * top : 0.0;
  return (q > 0) ? (uint32_t)((q < top) ? q : top) : 0u;
}

// the key of a point in the box {lo[3], hi[3]}: a pure function of the coordinates and the box
SCTL_AMD_CURVE_HD inline uint64_t curve_key(const double (&p)[3], const double* box) {
  return hilbert_key3(curve_cell(p[0], box[0], box[3] - box[0]), curve_cell(p[1], box[1], box[4] - box[1]), curve_cell(p[2], box[2], box[5] - box[2]));
}

}  // namespace sctl_amd
