// Host-side helpers that every translation unit of libsctl_amd.so uses around a transfer: the one place where `real` picks double or float, adding a
// staged result into the caller's array, and the pinned staging buffer.  No HIP here (the allocator is a template parameter: internal.hpp binds it to
// hipHostMalloc), so tests/cpp/staging_main.cpp runs all of it on the CPU under a sanitizer.
#pragma once
#include <sctl_amd.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#pragma GCC visibility push(hidden)
namespace sctl_amd {

inline size_t real_size(int real) { return real == SCTL_AMD_F64 ? 8 : 4; }
// fn(R{}) with R = double or float: the ONLY place that turns the run-time `real` into a type
template <class F> auto with_real(int real, F&& fn) { return real == SCTL_AMD_F64 ? fn(double{}) : fn(float{}); }

// dst[i] += src[i] (the accumulate semantics of GenericKernel::Eval, generic-kernel.txx:182-186; the scale factor was applied on the device)
inline void add_into(int real, void* dst, const void* src, int64_t n) {
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    R* d = (R*)dst;
    const R* s = (const R*)src;
    for (int64_t i = 0; i < n; i++) d[i] += s[i];
    return 0;
  });
}
inline void store_or_add(int real, void* dst, const void* src, int64_t n, bool accumulate) {
  if (accumulate) add_into(real, dst, src, n);
  else if (n > 0) std::memcpy(dst, src, (size_t)n * real_size(real));
}

// A device's slab of nd density-major result rows -> the caller's rows of Nt targets, k1 components each: slab row m, target i goes to target perm[i]
// (perm: the slab's part of a permutation, so device threads write disjoint entries) or, without perm, to target t0 + i.
inline void scatter_slab(int real, void* out, const void* slab, int nd, int64_t Nt, int64_t nt, int64_t t0, int k1, const int64_t* perm, bool accumulate) {
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    for (int m = 0; m < nd; m++) {
      R* orow = (R*)out + (int64_t)m * Nt * k1;
      const R* srow = (const R*)slab + (int64_t)m * nt * k1;
      if (!perm) { store_or_add(real, orow + t0 * k1, srow, nt * k1, accumulate); continue; }
      for (int64_t i = 0; i < nt; i++)
        for (int c = 0; c < k1; c++) {
          R& e = orow[perm[i] * k1 + c];
          e = (accumulate ? e : R(0)) + srow[i * k1 + c];
        }
    }
    return 0;
  });
}

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// Pinned staging memory for every host<->device transfer of the host-pointer entry points: the caller's pageable
// arrays are copied into a pinned slice by the CPU and DMA'd from there, so the copy is asynchronous to the host and never depends on
// how the runtime stages pageable memory.  History: round 1 introduced this after seeing the OLD contents of a reused, rewritten host
// array arrive on the device about once per thousand transfers, and blamed the H2D copy.  Round 2 could not reproduce that — neither
// stand-alone (tools/ubench/h2d_reuse.hip) nor inside the library with the staging compiled out (tools/h2d_in_library.py: 0 wrong
// results in 4000 iterations x 2 runtimes, profiles/r02_platform_probes.txt) — while the memory-pool fault that was removed at the
// same time IS reproducible (workspace.hpp): the stale results were most likely that fault.  The staging stays (its cost, one CPU
// memcpy, ~1.5 % at 2^20 points, is what the runtime's own pageable path pays too).
// Alloc: { using error; static constexpr error ok; static error alloc(char**, size_t); static void free(char*); }
template <class Alloc>
struct PinnedBufT {
  char* p = nullptr;
  size_t cap = 0, used = 0;
  ~PinnedBufT() { if (p) Alloc::free(p); }
  typename Alloc::error reserve(size_t bytes) {   // discards the contents; call before the first take() of a transfer batch
    used = 0;
    if (bytes <= cap) return Alloc::ok;
    release();
    typename Alloc::error e = Alloc::alloc(&p, bytes);
    if (e == Alloc::ok) cap = bytes;
    return e;
  }
  void release() { if (p) { Alloc::free(p); p = nullptr; cap = 0; } }
  char* take(size_t bytes) {           // 256-byte aligned slice
    char* q = p + used;
    used += pad256(bytes);
    return q;
  }
  static char* reserve_and_take(void* self, size_t bytes) {   // one slice holding `bytes` (for comm_gather_to_device); nullptr if out of memory
    PinnedBufT* b = (PinnedBufT*)self;
    return b->reserve(bytes) == Alloc::ok ? b->take(bytes) : nullptr;
  }
};

}  // namespace sctl_amd
#pragma GCC visibility pop
