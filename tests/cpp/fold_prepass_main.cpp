// Host driver of sctl_amd/csrc/fold_prepass.hpp for tests/test_fold_prepass.py: the header's own functions, compiled with g++.
//   fold_prepass_main <chunk>  < "n\n f_0\n f_1\n ..."   (densities as C99 hex floats, nan, inf)
// walks the sources of every split in order, as the device's fixed-order scan does, and prints
//   per source  "s <class> <slot or exception rank or -1> <k as a hex float>"
//   per split   "h <positive tiles> <negative tiles> <exceptions>"
// and first of all "l <cap> <rec> <idx> <exc> <bytes>", the layout of the block.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sctl_amd/csrc/fold_prepass.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const long long chunk = std::atoll(argv[1]);
  long long n = 0;
  if (std::scanf("%lld", &n) != 1 || chunk <= 0 || chunk % sctl_amd::kFoldTile) return 2;
  std::vector<double> f((size_t)n);
  for (auto& v : f) {
    char buf[64];
    if (std::scanf("%63s", buf) != 1) return 2;
    v = std::strtod(buf, nullptr);
  }
  const long long splits = (n + chunk - 1) / chunk;
  const sctl_amd::FoldPrepLayout L(splits, chunk);
  std::printf("l %lld %lld %lld %lld %lld\n", (long long)L.cap, (long long)L.rec, (long long)L.idx, (long long)L.exc, (long long)L.bytes);
  for (long long sp = 0; sp < splits; sp++) {
    long long npos = 0, nneg = 0, nexc = 0;
    for (long long s = sp * chunk; s < n && s < (sp + 1) * chunk; s++) {
      double k;
      const int cls = sctl_amd::fold_prep_class(f[(size_t)s], k);
      long long where = -1;
      if (cls == 1) where = sctl_amd::fold_prep_slot(false, npos++, L.cap);
      else if (cls == -1) where = sctl_amd::fold_prep_slot(true, nneg++, L.cap);
      else if (cls == 2) where = nexc++;
      std::printf("s %d %lld %a\n", cls, where, k);
    }
    std::printf("h %lld %lld %lld\n", (long long)sctl_amd::fold_prep_tiles(npos), (long long)sctl_amd::fold_prep_tiles(nneg), nexc);
  }
  return 0;
}
