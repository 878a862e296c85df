// The screened Coulomb (Yukawa) functor of yukawa_kernel.hip WITH a transposed form: a plugin that supplies pair_t gets the transposed entries
// (sctl_amd_eval_transpose_*) besides everything else.  The kernel is symmetric, K0 = K1 = 1, so pair_t is pair's arithmetic on a target record.
// tests/test_gpu_transpose.py compiles this file, loads it and checks both directions against the functor written in numpy.
#include <sctl_amd/device/kernel_plugin.hpp>

struct Yukawa3D_FxU_T {
  static constexpr int ID = -1, K0 = 1, K1 = 1, ND = 0, NREC = 4, NREC_T = 4, FLOPS = 10;
  static constexpr const char* NAME = "Yukawa3D-FxU-T";
  template <class R> using Consts = sctl_amd::DefaultConsts<R>;
  static constexpr double scale() { return 1 / (4 * sctl_amd::kPi); }
  static constexpr double acc_factor(int /*mode*/) { return 1; }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0];
  }
  template <class R, int MODE, bool MASKED>
  static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const sctl_amd::KerCtx& ctx, const Consts<R>& K) {
    const R r2 = sctl_amd::len2(d);
    const R rinv = sctl_amd::rsqrt_masked<MODE, MASKED>(r2, K.rsq);
    const R r = r2 * rinv;
    acc[0] = sctl_amd::fma_(rec[3], rinv * exp_(-R(ctx.v[0]) * r), acc[0]);
  }
  // the transposed form: record x_t, w; the owner's normal (none here: R[1]) comes from registers
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) { rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; }
  template <class R, int MODE, bool MASKED>
  static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&)[1], const R* rec, const sctl_amd::KerCtx& ctx, const Consts<R>& K) {
    pair<R, MODE, MASKED>(acc, d, rec, ctx, K);
  }
  static __device__ __forceinline__ double exp_(double x) { return ::exp(x); }
  static __device__ __forceinline__ float exp_(float x) { return ::expf(x); }
};

SCTL_AMD_REGISTER_KERNEL(Yukawa3D_FxU_T, /*context: lambda*/ 8)
