// Host program for tests/test_staging.py: the HIP-free host helpers of sctl_amd/csrc/staging.hpp — add_into / store_or_add, scatter_slab (what brings an
// operator's device slabs back into the caller's rows) and the staging buffer's slice arithmetic — against plain reference loops, built with
// -fsanitize=address,undefined so that an index or a slice that is off by one aborts the run.  Prints the number of cases checked; exit code 1 on a mismatch.
#include "../../sctl_amd/csrc/staging.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sctl_amd;

struct HeapAlloc {   // exactly `bytes`, so that the sanitizer sees a slice that passes the reservation
  using error = int;
  static constexpr int ok = 0;
  static int alloc(char** p, size_t bytes) { *p = (char*)std::malloc(bytes); return *p ? 0 : 1; }
  static void free(char* p) { std::free(p); }
};

template <class R> static R value(int64_t i, int salt) { return (R)((i * 37 + salt * 11) % 101) / (R)8 - (R)5; }

template <class R> static int scatter_cases(int real) {
  int cases = 0;
  for (int nd : {1, 3}) for (int k1 : {1, 3}) for (int64_t nt : {0, 1, 5}) for (int with_perm : {0, 1}) for (int accumulate : {0, 1}) {
    const int64_t t0 = 2, Nt = t0 + nt + 3;   // the slab is a part of the caller's targets
    std::vector<int64_t> perm((size_t)nt);
    for (int64_t i = 0; i < nt; i++) perm[(size_t)i] = (i * 3 + 1) % Nt;   // distinct targets anywhere in the caller's rows (checked below)
    for (int64_t i = 0; i < nt; i++) for (int64_t j = 0; j < i; j++) if (perm[(size_t)i] == perm[(size_t)j]) { std::puts("test bug: perm"); return -1; }
    std::vector<R> out((size_t)(nd * Nt * k1)), slab((size_t)(nd * nt * k1));
    for (size_t i = 0; i < out.size(); i++) out[i] = value<R>((int64_t)i, 1);
    for (size_t i = 0; i < slab.size(); i++) slab[i] = value<R>((int64_t)i, 2);
    std::vector<R> want = out;
    for (int m = 0; m < nd; m++) for (int64_t i = 0; i < nt; i++) for (int c = 0; c < k1; c++) {   // the reference loop
      R& e = want[(size_t)((m * Nt + (with_perm ? perm[(size_t)i] : t0 + i)) * k1 + c)];
      e = (accumulate ? e : (R)0) + slab[(size_t)((m * nt + i) * k1 + c)];
    }
    scatter_slab(real, out.data(), slab.data(), nd, Nt, nt, t0, k1, with_perm ? perm.data() : nullptr, accumulate != 0);
    if (out != want) { std::printf("scatter_slab differs: real %d nd %d k1 %d nt %d perm %d accumulate %d\n", real, nd, k1, (int)nt, with_perm, accumulate); return -1; }
    // store_or_add / add_into on the same data: one contiguous row
    std::vector<R> dst((size_t)(nt * k1)), ref;
    for (size_t i = 0; i < dst.size(); i++) dst[i] = value<R>((int64_t)i, 3);
    ref = dst;
    for (size_t i = 0; i < ref.size(); i++) ref[i] = (accumulate ? ref[i] : (R)0) + slab[i];
    store_or_add(real, dst.data(), slab.data(), nt * k1, accumulate != 0);
    if (dst != ref) { std::printf("store_or_add differs: real %d n %d accumulate %d\n", real, (int)(nt * k1), accumulate); return -1; }
    cases++;
  }
  return cases;
}

// what a host call does with its staging: reserve the sum of the padded sizes, then take one slice per transfer and fill it
static int staging_cases() {
  int cases = 0;
  const size_t sizes[][4] = {{0, 0, 0, 0}, {1, 0, 255, 256}, {257, 8, 0, 4}, {12, 36, 0, 4}, {300 * 24, 257 * 24, 0, 257 * 8}};
  PinnedBufT<HeapAlloc> stage;
  for (const auto& s : sizes) {
    size_t total = 0;
    for (size_t b : s) total += pad256(b);
    if (stage.reserve(total) != 0) return -1;
    char* last_end = stage.p;
    for (size_t b : s) {
      if (pad256(b) < b || pad256(b) % 256 != 0 || pad256(b) >= b + 256) { std::puts("pad256 is wrong"); return -1; }
      char* q = stage.take(b);
      if (q < last_end || (size_t)(q - stage.p) % 256 != 0) { std::puts("slices overlap or are not aligned"); return -1; }
      if (b) std::memset(q, 0x5a, b);   // past the reservation: the sanitizer aborts
      last_end = q + b;
    }
    if (stage.used > stage.cap && total > 0) { std::puts("slices pass the reservation"); return -1; }
    cases++;
  }
  char* one = PinnedBufT<HeapAlloc>::reserve_and_take(&stage, 100000);   // grows: the old block goes
  if (!one) return -1;
  std::memset(one, 1, 100000);
  return cases + 1;
}

int main() {
  const int a = scatter_cases<double>(SCTL_AMD_F64), b = scatter_cases<float>(SCTL_AMD_F32), c = staging_cases();
  if (a < 0 || b < 0 || c < 0) return 1;
  if (real_size(SCTL_AMD_F64) != 8 || real_size(SCTL_AMD_F32) != 4) return 1;
  std::printf("%d %d %d\n", a, b, c);
  return 0;
}
