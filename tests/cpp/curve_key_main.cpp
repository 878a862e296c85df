// Host program around sctl_amd/csrc/curve_key.hpp for tests/test_curve_key.py and tools/near_share.py: the device code's key functions, called on the CPU.
//   curve_key_main cells <bits>     stdin: n, then n triples of cell numbers           -> one key per line (hilbert_key3 with that many bits per axis)
//   curve_key_main points           stdin: n, then n triples of coordinates (%la or %g) -> one key per line: bounding box (NaN ignored, as bbox_partial_kernel
//                                                                                          does), then curve_key
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sctl_amd/csrc/curve_key.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  long long n = 0;
  if (std::scanf("%lld", &n) != 1 || n < 0) return 2;
  if (!std::strcmp(argv[1], "cells") && argc == 3) {
    const int bits = std::atoi(argv[2]);
    if (bits < 1 || bits > sctl_amd::kCurveBits) return 2;
    for (long long i = 0; i < n; i++) {
      unsigned a, b, c;
      if (std::scanf("%u %u %u", &a, &b, &c) != 3) return 3;
      std::printf("%" PRIu64 "\n", sctl_amd::hilbert_key3(a, b, c, bits));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "points")) {
    std::vector<double> x((size_t)n * 3);
    for (auto& v : x)
      if (std::scanf("%lf", &v) != 1) return 3;
    double box[6] = {1.7976931348623157e308, 1.7976931348623157e308, 1.7976931348623157e308, -1.7976931348623157e308, -1.7976931348623157e308, -1.7976931348623157e308};
    for (long long i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) {
        const double v = x[i * 3 + k];
        box[k] = (v < box[k]) ? v : box[k];
        box[3 + k] = (v > box[3 + k]) ? v : box[3 + k];
      }
    for (long long i = 0; i < n; i++) {
      const double p[3] = {x[i * 3], x[i * 3 + 1], x[i * 3 + 2]};
      std::printf("%" PRIu64 "\n", sctl_amd::curve_key(p, box));
    }
    return 0;
  }
  return 2;
}
