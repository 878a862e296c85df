// Device micro-kernels for gfx950: one struct per Green's function.
//
// Each struct replaces one functor of the reference's include/sctl/kernel_functions.hpp (cited per struct)
// but is NOT a transcription: the reference builds the K0 x K1 matrix U and then does K0*K1 FMAs
// (generic-kernel.txx:81-90); here every kernel is the contracted form  acc[k1] += sum_k0 U[k0][k1] f[k0]
// written with the fewest fp64 VALU instructions (MI355X fp64 FMA issues at 4 cycles per wave64, the
// reciprocal-square-root seed at 16 — tools/ubench/valu_rates.hip), and source records are pre-packed in
// LDS (e.g. normal*density for double-layer kernels) so that the per-pair work is minimal.
//
// Interface used by eval_kernel.hpp:
//   K0, K1, ND          SrcDim, TrgDim, NormalDim (generic-kernel.hpp:59-84)
//   NREC                reals per packed source record in LDS (multiple of 16 bytes for R = double and float)
//   FLOPS, scale()      kernel_functions.hpp FLOPS() / uKerScaleFactor
//   pack(rec, x, n, f)  build the LDS record of one source from the AoS inputs
//   pair<R,MODE,MASKED>(acc, d, rec, ctx, K)   one pair interaction, d = x_trg - x_src  (generic-kernel.txx:83)
// and the multi-density forms used by sctl_amd/csrc/rows_kernel.hpp, forward (M densities on the same sources and targets):
//   NREC_M<M>                  reals per LDS record: x, the normal where ND > 0, then M densities of K0 reals (pack_multi), padded to 16 bytes
//   pack_m<R,M>(rec, x, n, f)  f[M][K0]: the record holds the geometry once and the densities as they are (no density is pre-multiplied
//                              into the geometry: a double-layer record keeps n and applies each f in pair_m)
//   pair_m<R,MODE,MASKED,M>(acc, d, rec, ctx, K)   acc[M][K1]: the density-independent factors of the pair (distance, reciprocal square root
//                              and its refinement, Helmholtz's e^{ikr}) once, then one contraction per density.  Same masking and acc_factor
//                              as pair(): a launch scales both forms alike.
// and the transposed forms used by eval_transpose_kernel.hpp (g[s,k0] += sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] w[t,k1]: the SOURCE owns the output and
// its normal, the TARGETS stream):
//   NREC_T                     reals per streamed target record: the coordinates, then what the pair needs of w[K1]
//   pack_t<R>(rec, x_t, w)     or pack_t_mode<R,MODE> where the record depends on the accuracy mode, as pack_mode does
//   pair_t<R,MODE,MASKED[,VARIANT]>(acc, d, n, rec, ctx, K)   acc[k0] += sum_k1 U(d, n)[k0][k1] w[k1] with the SAME d = x_trg - x_src as pair(), n the owner's
//                              normal (R[3], or R[1] unused when ND == 0) from registers.  Same rsqrt helpers, modes, masking and acc_factor as pair().
//   finish_t<R>(acc) / finish_t_mode<R,MODE>(acc)   optional, applied once to a source's K0 sums (FinishTOf)
// and the transposed forms for several weight vectors used by sctl_amd/csrc/rows_kernel.hpp, transposed (M weight vectors on the same targets and sources):
//   NREC_TM<M>                 reals per streamed target record: x_t once, then what the pair needs of each of the M weight vectors, padded to 16 bytes
//   pack_tm<R,M>(rec, x_t, w)  w[M][K1]: the weights as they are (the traction kernel: the six symmetric sums of each); nothing mode-dependent is folded in
//   pair_tm<R,MODE,MASKED,M[,VARIANT]>(acc, d, n, rec, ctx, K)   acc[M][K0]: what does not depend on w (distance, reciprocal square root and its refinement,
//                              d.n, Helmholtz's reduction and polynomial) once, then one contraction per weight vector.  Same d = x_trg - x_src, masking,
//                              acc_factor and finish_t / finish_t_mode as pair_t(): a launch scales and finishes both forms alike.
// and the gradient form used by eval_grad_kernel.hpp from both of its sides (the pair's scalar phi = sum_k0 sum_k1 w[k1] U(d, n)[k0][k1] f[k0]):
//   pair_g<R,MODE,MASKED[,VARIANT],WANT_N>(G, N, d, n, f, w, ctx, K)   G[j] += d phi / d d_j and, where WANT_N, N[j] += d phi / d n_j, with the SAME
//                              d = x_trg - x_src as pair(); n (R[3], or R[1] unused when ND == 0), f[K0] and w[K1] are the plain inputs, from registers
//                              on the owner's side and from the streamed record on the other.  Every phi is a sum of terms P(d, n, f, w) r^-p with P
//                              polynomial, so grad phi = sum (grad P y^p - p P y^(p+2) d) with y = 1/r: the forms below take the NORMALISED
//                              rsqrt_masked<MODE, MASKED> (rsqrt_grad: fp32 always refined) (a gradient mixes the powers p and p + 2, and its owner holds no record a factor could be
//                              folded into), so the sums need no per-mode factor.  A kernel that accumulates a multiple anyway names it in the
//                              optional grad_factor(mode) (GradFactorOf; Helmholtz3D_FxU: its tables reduce the mode's C r).
// and its form for M density / weight rows used by sctl_amd/csrc/multi_grad_kernel.hpp (optional, HasPairGM):
//   pair_gm<R,MODE,MASKED[,VARIANT],WANT_N,M>(G, N, d, n, f, w, ctx, K)   f[M][K0], w[M][K1]: adds the derivatives of sum_m phi(f[m], w[m]).  Same d, root,
//                              masking and grad_factor as pair_g; what does not depend on the rows is done once per pair.  phi is bilinear in (f, w), so the rows
//                              are first contracted into the block C = sum_m f_m (x) w_m (contract_rows) and <U, C> is differentiated once — except the
//                              traction kernel, whose rank-one terms run row by row (DESIGN.md §4.16 has the counts).
// and the tangent form used by sctl_amd/csrc/jvp_kernel.hpp (the forward-mode twin of pair_g: the derivative of the pair's K1 values along a perturbation of
// the geometry, the densities held fixed):
//   pair_j<R,MODE,MASKED[,VARIANT]>(acc, d, e, n, m, f, ctx, K)   acc[k1] += sum_k0 [(e.grad_d) U(d, n) + (m.grad_n) U(d, n)][k0][k1] f[k0], with the SAME
//                              d = x_trg - x_src as pair(), e = delta d = delta x_trg - delta x_src and m = delta n_src (R[3], or R[1] unused when ND == 0);
//                              n and f[K0] are the plain inputs.  phi of pair_g is linear in w, so acc[k1] is the coefficient of w[k1] in
//                              grad_d phi . e + grad_n phi . m: the same powers of y = 1/r, hence the same root (rsqrt_grad: the NORMALISED rsqrt_masked, fp32
//                              always refined), the same masking (a coincident pair adds 0) and the same grad_factor(mode) as pair_g.  Helmholtz takes G from
//                              pair()'s tables and variants; the wavenumber is not differentiated.  One exception to the root: the fp32 form of
//                              Laplace3D_FDxUdU, the only tangent that rises to y^7, takes r^2, one Newton step from the masked fp32 seed and y^2, y^3 in
//                              fp64, whatever the mode (the comment there).  DESIGN.md §4.18 has the forms and the counts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "fastmath.hpp"

namespace sctl_amd {

constexpr double kPi = 3.141592653589793238462643383279502884;

// Kernel context passed by value in the launch arguments (replaces the host ctx_ptr, generic-kernel.hpp:150).
struct KerCtx { double v[4]; };

// ---- masked reciprocal square root ---------------------------------------------------------------------
// Semantics of approx_rsqrt<digits>(r2, r2 > 0) (vec.txx:361-364, intrin-wrapper.hpp:539-555): 0 where
// r2 == 0, else r2^-1/2 to `digits` digits.  The seed is the hardware v_rsq_f64 / v_rsq_f32 (measured max
// relative error 2^-24.2 / 2^-23.3, tools/ubench/rsq_accuracy.hip); v_rsq(0) = +inf, whose high word is
// replaced by 0 with two 32-bit VALU ops (the low word of +inf is already 0).  Refinement, with
// e = 1 - x y^2 computed by one FMA so that it is exact to fp64 rounding:
//   MODE 0: seed only                                (>= 7 digits)
//   MODE 1: one Newton step,  y + y e / 2            (error 3/8 e^2 <= 4.3e-15, rms 3.5e-16: >= 14 digits)
//   MODE 2: one Halley step,  y + y e (1/2 + 3/8 e)  (error O(e^3): rounding only)
// With y = 0 every refinement returns 0, so the mask survives; NaN/inf inputs propagate as in the reference.
// MASKED = false skips the two mask instructions (9.5 % of the Laplace kernel's time, tools/ubench/laplace_variants):
// a coincident pair then yields inf/NaN, which eval_kernel.hpp detects per LDS tile and repairs by re-running that
// tile with MASKED = true — the result is identical to the always-masked evaluation.
// The one constant that is not a hardware inline constant (3/8) lives in a VGPR pair for the whole kernel
// (RsqConst, made opaque to the optimiser so that it is not re-materialised with v_mov per use).
// (The two constants of the four-instruction cubic step rsqrt_cubic83 below: c = 1 + m 2^-25 with m = round(2/3 2^25), and k = 4 (c - 1) - (c - 1)^2,
// both exact doubles.)  They are wave-uniform and live in scalar registers: an fp64 VALU instruction takes one scalar operand for free, and the
// tile-centred kernel has no vector registers to spare.
constexpr double kCubicC = 0x1.aaaaaa8000000p+0, kCubicK = 0x1.1c71c6e38e38ep+1;
// (and of its forms for r^-3 and r^-5, rsqrt3_cubic / rsqrt5_cubic: c = 7/5, k = 28/75 and c = 9/7, k = 36/245, rounded the same way)
constexpr double kCubic3C = 0x1.6666660000000p+0, kCubic3K = 0x1.7e4b170a3d700p-2, kCubic5C = 0x1.4924920000000p+0, kCubic5K = 0x1.2cee3c14e5e00p-3;
template <class R> struct RsqConst {
  R c38, c53, k209, c3, k3, c5, k5;
  __device__ __forceinline__ RsqConst() : c38(R(0.375)), c53(R(kCubicC)), k209(R(kCubicK)), c3(R(kCubic3C)), k3(R(kCubic3K)), c5(R(kCubic5C)), k5(R(kCubic5K)) {
    asm volatile("" : "+v"(c38), "+s"(c53), "+s"(k209), "+s"(c3), "+s"(k3), "+s"(c5), "+s"(k5));
  }
};

template <int MODE, bool MASKED> __device__ __forceinline__ double rsqrt_masked(double r2, const RsqConst<double>& K) {
  double y = __builtin_amdgcn_rsq(r2);
  if (MASKED) {
  // r2 == 0 -> y = +inf = {hi 0x7ff00000, lo 0} -> 0: one 32-bit compare + one v_cndmask on the high word.
  // The empty asm only stops the optimiser from widening this into a 64-bit compare; the compare and select
  // themselves are compiler-generated so that the gfx950 trans->VALU hazard after v_rsq_f64 is padded correctly
  // (an asm block reading the v_rsq result directly is NOT padded and read a stale register: observed as a NaN).
  int hi = __double2hiint(y);
  asm("" : "+v"(hi));
  hi = (hi == 0x7ff00000) ? 0 : hi;
  y = __hiloint2double(hi, __double2loint(y));
  }
  if (MODE >= 1) {
    const double a = r2 * y;
    const double e = __builtin_fma(-a, y, 1.0);
    const double ye = y * e;
    if (MODE == 1) y = __builtin_fma(ye, 0.5, y);
    else y = __builtin_fma(ye, __builtin_fma(e, K.c38, 0.5), y);
  }
  return y;
}
template <int MODE, bool MASKED> __device__ __forceinline__ float rsqrt_masked(float r2, const RsqConst<float>&) {
  float y = __builtin_amdgcn_rsqf(r2);
  if (MASKED) y = (__float_as_uint(y) == 0x7f800000u) ? 0.0f : y;   // r2 == 0 -> +inf -> 0
  if (MODE >= 1) {   // one Newton step in fp32 (only when more than 7 digits are asked of fp32)
    const float a = r2 * y;
    const float e = __builtin_fmaf(-a, y, 1.0f);
    y = __builtin_fmaf(y * e, 0.5f, y);
  }
  return y;
}

// Per-kernel constants, constructed once at kernel entry and passed to every pair() call.
// A kernel may ask for LDS_DOUBLES doubles of workgroup scratch, which its Consts constructor fills (all lanes of the
// workgroup call it; it may synchronise).
template <class R> struct DefaultConsts {
  static constexpr int LDS_DOUBLES = 0;
  static constexpr bool HAS_VARIANT = false;   // true: pair<R, MODE, MASKED, VARIANT> exists and variant(ctx) picks it per launch (0 .. NUM_VARIANTS-1, default 2)
  RsqConst<R> rsq;
  __device__ __forceinline__ explicit DefaultConsts(double*) {}
  // hooks of the speculative (unmasked) tile pass of eval_kernel: a kernel whose fast path has a precondition records
  // violations per lane and reports them at the end of the tile, which is then re-run on the careful path
  __device__ __forceinline__ void begin_tile() const {}
  __device__ __forceinline__ bool tile_bad(const KerCtx&) const { return false; }
};
// The Helmholtz kernel runs on the modes' unnormalised reciprocal square roots too (rsqrt_scaled below: C / r with C = 2 for MODE 1, A = 2.6666666 for
// MODE 2): the amplitude's C goes into the scale, and the distance comes out as r2 (C / r) = C r at the price of the normalised one.  C by mode:
constexpr double helmholtz_dist_factor(int mode) { return mode == 1 ? 2.0 : mode == 2 ? 0x1.5555550000000p+1 : 1.0; }
template <class R> struct HelmholtzConsts;
template <> struct HelmholtzConsts<float> {          // fp32: libm sincosf / expf
  static constexpr int LDS_DOUBLES = 0;
  static constexpr bool HAS_VARIANT = true;
  static constexpr int NUM_VARIANTS = 2;
  __device__ __forceinline__ int variant(const KerCtx& ctx) const { return ctx.v[1] == 0 ? 1 : 0; }
  RsqConst<float> rsq;
  float cinv = 1.0f;       // 1 / C: pair() forms C r from the mode's unnormalised C / r (helmholtz_dist_factor)
  __device__ __forceinline__ explicit HelmholtzConsts(double*) {}
  __device__ __forceinline__ HelmholtzConsts(double*, int, const KerCtx&, int mode) : cinv((float)(1.0 / helmholtz_dist_factor(mode))) {}
  __device__ __forceinline__ void begin_tile() const {}
  __device__ __forceinline__ bool tile_bad(const KerCtx&) const { return false; }
};
template <> struct HelmholtzConsts<double> {         // fp64: table-driven e^{ikr} (fastmath.hpp), tables in LDS
  // Two table sets.  The all-pairs evaluator (256-lane workgroups that live for thousands of tiles) offers LDS_DOUBLES_ALL_PAIRS and, when
  // the wavenumber allows it (Re k > 0, |Im k| <= Re k / 4), runs the ONE-reduction form: 2048 complex nodes with the decay folded in +
  // 256 period factors (34 KB).  The one-wave evaluators (lists, matrix blocks) keep the small tables (10 KB) of the two-reduction form:
  // 34 KB per 64 lanes would cost them their occupancy.
  static constexpr int LDS_DOUBLES = fastmath::kTableDoubles;
  static constexpr int LDS_DOUBLES_ALL_PAIRS = fastmath::kCexpTableDoubles > fastmath::kTableDoubles ? fastmath::kCexpTableDoubles : fastmath::kTableDoubles;
  static constexpr bool HAS_VARIANT = true;
  static constexpr int NUM_VARIANTS = 4;               // 0: complex k, two reductions; 1: real k, sincos only; 2: complex k, one reduction; 3: real k, one reduction
  bool one_reduction;
  __device__ __forceinline__ int variant(const KerCtx& ctx) const { return (ctx.v[1] == 0 ? 1 : 0) + (one_reduction ? 2 : 0); }
  RsqConst<double> rsq;
  fastmath::TabCoeffsK tk;     // reduction and polynomial constants with the launch's wavenumber folded in: functions of the distance
  fastmath::CexpCoeffsK ck;    // the same for the one-reduction form
  const double* table;
  double cdist, cinv;          // C and 1 / C of the distance pair() hands over (C r)
  // (a Consts type constructible from (double*, int, const KerCtx&[, int mode]) is handed the scratch capacity, the launch's context and its accuracy mode: make_consts below)
  __device__ __forceinline__ HelmholtzConsts(double* lds, int lds_doubles, const KerCtx& ctx) : HelmholtzConsts(lds, lds_doubles, ctx, 0) {}
  __device__ __forceinline__ HelmholtzConsts(double* lds, int lds_doubles, const KerCtx& ctx, int mode) : table(lds), cdist(helmholtz_dist_factor(mode)), cinv(1.0 / helmholtz_dist_factor(mode)) {
    one_reduction = lds_doubles >= fastmath::kCexpTableDoubles && fastmath::CexpCoeffsK::usable(ctx.v[0], -ctx.v[1]);   // (+17 % over two reductions: profiles/r03_ab_helmholtz_one_reduction.txt)
    {
      const fastmath::Coeffs full;                   // the table-free polynomials, used here only
      if (one_reduction) fastmath::fill_cexp_tables(lds, (int)threadIdx.x, (int)blockDim.x, ctx.v[0], -ctx.v[1], full, fastmath::TabCoeffs());
      else fastmath::fill_tables(lds, (int)threadIdx.x, (int)blockDim.x, full);
    }
    __syncthreads();
    if (one_reduction) {
      ck.set_scaled(ctx.v[0], -ctx.v[1], fastmath::TabCoeffs(), cdist);   // the one-reduction form reduces C r directly
      ck.pin();
    } else {
      tk.set_scaled(ctx.v[0], -ctx.v[1], fastmath::TabCoeffs(), cdist);
      tk.pin();
    }
  }
  __device__ __forceinline__ HelmholtzConsts(double* lds, const KerCtx& ctx) : HelmholtzConsts(lds, LDS_DOUBLES, ctx) {}
  // the table-driven forms need |Re k| r <= kSincosTabMaxArg and |Im k| r <= kExpTabMaxArg (one reduction: Re k r <= kCexpMaxPhase): the
  // speculative pass only tracks the largest distance
  // (a distance is >= +0 or NaN, so its HIGH WORD orders like the number: the maximum is one 32-bit integer instruction per pair, and a
  // NaN's high word is larger than any finite one, which sends its tile to the careful pass)
  mutable unsigned rmax_hi = 0;
  __device__ __forceinline__ void begin_tile() const { rmax_hi = 0; }
  __device__ __forceinline__ void note_distance(double r) const {
    const unsigned h = (unsigned)__double2hiint(r);
    rmax_hi = (h > rmax_hi) ? h : rmax_hi;
  }
  __device__ __forceinline__ bool tile_bad(const KerCtx& ctx) const {
    const double rmax = __hiloint2double((int)(rmax_hi + 1u), 0);   // the next high word up bounds every low word
    if (one_reduction) return !(ctx.v[0] * rmax <= fastmath::kCexpMaxPhase * cdist);   // (the distances recorded are C r)
    return !(__builtin_fabs(ctx.v[0]) * rmax <= fastmath::kSincosTabMaxArg * cdist && __builtin_fabs(ctx.v[1]) * rmax <= fastmath::kExpTabMaxArg * cdist);
  }
};

// A kernel whose pair() leaves some entries of acc to be derived from others — a symmetric output: the traction kernel fills the upper
// triangle only — supplies `template <class R> static void finish(R (&acc)[K1])`, or `template <class R, int MODE> static void finish_mode(...)`
// when what is left to do depends on the accuracy mode (the fused Laplace kernel: its potential and its gradient accumulate different powers
// of the unnormalised 1/r); the evaluators apply it once, when the sums leave the registers (finish_acc).
template <class Ker, class R, int MODE, class = void, class = void> struct FinishOf {
  static __device__ __forceinline__ void apply(R (&)[Ker::K1]) {}
};
template <class Ker, class R, int MODE, class V> struct FinishOf<Ker, R, MODE, std::void_t<decltype(&Ker::template finish<R>)>, V> {
  static __device__ __forceinline__ void apply(R (&acc)[Ker::K1]) { Ker::template finish<R>(acc); }
};
template <class Ker, class R, int MODE> struct FinishOf<Ker, R, MODE, void, std::void_t<decltype(&Ker::template finish_mode<R, MODE>)>> {
  static __device__ __forceinline__ void apply(R (&acc)[Ker::K1]) { Ker::template finish_mode<R, MODE>(acc); }
};
template <class Ker, class R, int MODE> __device__ __forceinline__ void finish_acc(R (&acc)[Ker::K1]) { FinishOf<Ker, R, MODE>::apply(acc); }

// The LDS record of one source: Ker::pack<R>, or `template <class R, int MODE> static void pack_mode(rec, x, n, f)` when the record depends on
// the accuracy mode (kernels that keep a density pre-multiplied by a power of the unnormalised 1/r's factor, below).
template <class Ker, class R, int MODE, class = void> struct PackOf {
  static __device__ __forceinline__ void apply(R* rec, const R* x, const R* n, const R* f) { Ker::template pack<R>(rec, x, n, f); }
};
template <class Ker, class R, int MODE> struct PackOf<Ker, R, MODE, std::void_t<decltype(&Ker::template pack_mode<R, MODE>)>> {
  static __device__ __forceinline__ void apply(R* rec, const R* x, const R* n, const R* f) { Ker::template pack_mode<R, MODE>(rec, x, n, f); }
};
template <class Ker, class R, int MODE> __device__ __forceinline__ void pack_record(R* rec, const R* x, const R* n, const R* f) { PackOf<Ker, R, MODE>::apply(rec, x, n, f); }

// The transposed form of a kernel (pair_t and its record) is optional: a functor without it evaluates A only.  HasPairT detects the streamed record's size,
// which every transposed form must name; PackTOf / FinishTOf pick pack_t or pack_t_mode and the optional finish_t / finish_t_mode as PackOf / FinishOf do.
template <class Ker, class = void> struct HasPairT : std::false_type {};
template <class Ker> struct HasPairT<Ker, std::void_t<decltype(Ker::NREC_T), decltype(&Ker::template pair_t<double, 0, true>)>> : std::true_type {};
template <class Ker, class R, int MODE, class = void> struct PackTOf {
  static __device__ __forceinline__ void apply(R* rec, const R* x, const R* w) { Ker::template pack_t<R>(rec, x, w); }
};
template <class Ker, class R, int MODE> struct PackTOf<Ker, R, MODE, std::void_t<decltype(&Ker::template pack_t_mode<R, MODE>)>> {
  static __device__ __forceinline__ void apply(R* rec, const R* x, const R* w) { Ker::template pack_t_mode<R, MODE>(rec, x, w); }
};
template <class Ker, class R, int MODE> __device__ __forceinline__ void pack_t_record(R* rec, const R* x, const R* w) { PackTOf<Ker, R, MODE>::apply(rec, x, w); }
template <class Ker, class R, int MODE, class = void, class = void> struct FinishTOf {
  static __device__ __forceinline__ void apply(R (&)[Ker::K0]) {}
};
template <class Ker, class R, int MODE, class V> struct FinishTOf<Ker, R, MODE, std::void_t<decltype(&Ker::template finish_t<R>)>, V> {
  static __device__ __forceinline__ void apply(R (&acc)[Ker::K0]) { Ker::template finish_t<R>(acc); }
};
template <class Ker, class R, int MODE> struct FinishTOf<Ker, R, MODE, void, std::void_t<decltype(&Ker::template finish_t_mode<R, MODE>)>> {
  static __device__ __forceinline__ void apply(R (&acc)[Ker::K0]) { Ker::template finish_t_mode<R, MODE>(acc); }
};
template <class Ker, class R, int MODE> __device__ __forceinline__ void finish_t_acc(R (&acc)[Ker::K0]) { FinishTOf<Ker, R, MODE>::apply(acc); }

// The gradient form of a kernel (pair_g) is optional too: a functor without it evaluates A and, with pair_t, A^T only.  HasPairG detects it in either
// spelling, pair_g<R, MODE, MASKED, WANT_N> or, for a kernel with launch-uniform variants, pair_g<R, MODE, MASKED, VARIANT, WANT_N>.
template <class Ker, class = void, class = void> struct HasPairG : std::false_type {};
template <class Ker, class V> struct HasPairG<Ker, std::void_t<decltype(&Ker::template pair_g<double, 0, true, false>)>, V> : std::true_type {};
template <class Ker> struct HasPairG<Ker, void, std::void_t<decltype(&Ker::template pair_g<double, 0, true, 0, false>)>> : std::true_type {};
// ... and so is its form for several rows (pair_gm): a functor with pair_g alone has its rows evaluated one at a time
template <class Ker, class = void, class = void> struct HasPairGM : std::false_type {};
template <class Ker, class V> struct HasPairGM<Ker, std::void_t<decltype(&Ker::template pair_gm<double, 0, true, false, 2>)>, V> : std::true_type {};
template <class Ker> struct HasPairGM<Ker, void, std::void_t<decltype(&Ker::template pair_gm<double, 0, true, 0, false, 2>)>> : std::true_type {};
// pair_g of mode m accumulates GradFactorOf<Ker>::value(m) x the derivative: Ker::grad_factor(m) when named, else 1
template <class Ker, class = void> struct GradFactorOf { static constexpr double value(int) { return 1; } };
template <class Ker> struct GradFactorOf<Ker, std::void_t<decltype(Ker::grad_factor(0))>> { static constexpr double value(int mode) { return Ker::grad_factor(mode); } };

// Per-kernel constants of a launch: Consts(lds, capacity, ctx) when the type takes the scratch capacity (in doubles) and the context,
// Consts(lds, ctx) when it takes the context, Consts(lds) otherwise.
template <class KC> __device__ __forceinline__ KC make_consts(double* lds, int lds_doubles, const KerCtx& ctx) {
  if constexpr (std::is_constructible<KC, double*, int, const KerCtx&>::value) return KC(lds, lds_doubles, ctx);
  else if constexpr (std::is_constructible<KC, double*, const KerCtx&>::value) return KC(lds, ctx);
  else return KC(lds);
}
template <class KC> __device__ __forceinline__ KC make_consts(double* lds, const KerCtx& ctx) { return make_consts<KC>(lds, KC::LDS_DOUBLES, ctx); }
// ... and the accuracy mode of the launch, for a Consts type constructible from (double*, int, const KerCtx&, int mode): constants that depend on
// which reciprocal square root pair() will use (HelmholtzConsts: the table reduction takes the distance as C r)
template <class KC> __device__ __forceinline__ KC make_consts(double* lds, int lds_doubles, const KerCtx& ctx, int mode) {
  if constexpr (std::is_constructible<KC, double*, int, const KerCtx&, int>::value) return KC(lds, lds_doubles, ctx, mode);
  else return make_consts<KC>(lds, lds_doubles, ctx);
}
template <class KC> __device__ __forceinline__ KC make_consts(double* lds, const KerCtx& ctx, int mode) { return make_consts<KC>(lds, KC::LDS_DOUBLES, ctx, mode); }
// Scratch the all-pairs evaluator offers a kernel: LDS_DOUBLES_ALL_PAIRS when the Consts type names one, LDS_DOUBLES otherwise.
template <class KC, class = void> struct AllPairsScratch { static constexpr int value = KC::LDS_DOUBLES; };
template <class KC> struct AllPairsScratch<KC, std::void_t<decltype(KC::LDS_DOUBLES_ALL_PAIRS)>> { static constexpr int value = KC::LDS_DOUBLES_ALL_PAIRS; };
// Number of launch-uniform variants of pair(): NUM_VARIANTS when named, else 2 for a HAS_VARIANT kernel (pair<R, MODE, MASKED, bool>).
template <class KC, class = void> struct NumVariants { static constexpr int value = KC::HAS_VARIANT ? 2 : 1; };
template <class KC> struct NumVariants<KC, std::void_t<decltype(KC::NUM_VARIANTS)>> { static constexpr int value = KC::NUM_VARIANTS; };

template <class R> __device__ __forceinline__ R fma_(R a, R b, R c);
template <> __device__ __forceinline__ double fma_<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float fma_<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <class R> __device__ __forceinline__ R len2(const R (&d)[3]) { return fma_(d[2], d[2], fma_(d[1], d[1], d[0] * d[0])); }
template <class R> __device__ __forceinline__ R dot3(const R (&d)[3], const R* v) { return fma_(d[2], v[2], fma_(d[1], v[1], d[0] * v[0])); }

// MODE 1 for kernels whose terms all carry the same power of 1/r: the Newton step without its halving, y0 (3 - r2 y0^2) = 2/r
// (>= 14 digits), three instructions instead of four.  The factor 2^p goes into the scale applied once per target
// (Ker::acc_factor): this is the accuracy ParticleFMM (10 digits) and BoundaryIntegralOp (tol 1e-10) ask for by default, so it is
// the form the reference's own callers run.  With the masked seed y0 = 0 the result is 0, so the r = 0 rule survives.
// The step always lands low: with d the seed's relative error it returns (2/r)(1 - 3/2 d^2 - ...), measured over 1.3e8 arguments
// (tools/ubench/rsq_refine_accuracy.hip) mean -1.725e-16, range [-4.27e-15, +2.5e-16].  A one-sided error is a bias, and a bias does not
// average out over a sum; its mean is folded into acc_factor (newton2_factor(p) for a kernel whose terms carry (2/r)^p), i.e. into the
// scale applied once per target: no instruction, the per-pair error keeps its width and loses its offset.  (Centring the RANGE instead —
// a factor 1 + 3/4 d_max^2 — would put the worst case at +-2.1e-15 but move the mean to +1.9e-15: rms 1.9e-15 against 3.0e-16.)
constexpr double kNewton2MeanErr = -1.725e-16;
constexpr double newton2_factor(int p) { return (p == 1 ? 2.0 : p == 3 ? 8.0 : 32.0) * (1.0 + p * kNewton2MeanErr); }
// The refinements below come in two forms: the product y0 P itself, and the two factors {y0, P} (rsqrt_scaled_split) for a caller that fuses
// the product into its accumulate, acc = fma(y0, P, acc) — the folded far pair of the tile-centred single layer (centered_kernel.hpp), whose
// source record carries the density inside y0.
template <class R> struct RsqSplit { R y, p; };
template <bool MASKED, class R> __device__ __forceinline__ RsqSplit<R> rsqrt_newton2_split(R r2, const RsqConst<R>& K) {
  const R y = rsqrt_masked<0, MASKED>(r2, K);
  const R a = r2 * y;
  return {y, fma_(-a, y, R(3))};
}
template <bool MASKED, class R> __device__ __forceinline__ R rsqrt_newton2(R r2, const RsqConst<R>& K) {
  const RsqSplit<R> s = rsqrt_newton2_split<MASKED>(r2, K);
  return s.y * s.p;
}

// MODE 2 (full precision, the default) for the same kernels: the CUBIC step without its normalisation, in FOUR instructions.
// With w = r2 y0^2 = 1 - e the Halley polynomial 1 + e/2 + 3/8 e^2 is 3/8 (w^2 - 10/3 w + 5) = 3/8 ((w - 5/3)^2 + 20/9): a monic
// quadratic in w, i.e. ONE FMA for z = r2 (y0 y0) - 5/3 and one for z z + 20/9 — the small quantity e is never formed —
//     y0 ((r2 y0^2 - 5/3)^2 + 20/9) = (8/3) / r (1 + 5/16 e^3 + ...),
// against five instructions for y0 + y0 e (1/2 + 3/8 e); the factor (8/3)^p goes into the scale applied once per target, as for MODE 1.
// The constants need not BE 5/3 and 20/9, only be consistent: with c - 1 = B/2 and k = A - (c - 1)^2 the polynomial is A + B e + e^2, and what
// matters is B / A = 1/2 to ~2^-31 (its error is multiplied by e <= 2^-23) and 1/A = 3/8 to ~2^-8 (multiplied by e^2).  So c - 1 is 2/3 rounded
// to 25 bits, A = 4 (c - 1) = 2.666666627 and k = A - (c - 1)^2 are then EXACT doubles, B / A is exactly 1/2, 1/A is 3/8 (1 + 1.5e-8), and
// the scale carries no rounding of the factor for p = 1 (cubic83_factor(3), (5) are A^3, A^5 correctly rounded).
// Accuracy (tools/ubench/rsq_refine_accuracy.hip, 1.3e8 arguments against long double, profiles/r03_rsq_refine_accuracy.txt): three roundings
// sit on the main path (y0 y0, the polynomial, the product) where Halley's correction term has one, so the worst case is that of the reference's
// own default approx_rsqrt (2.5 ulp) rather than Halley's 1.25 ulp, with a smaller rms than the reference's.
// With the masked seed y0 = 0 the result is 0; an unmasked coincident pair gives z = 0 * inf = NaN, which the speculative pass detects.
constexpr double cubic83_factor(int p) { return p == 1 ? 0x1.5555550000000p+1 : p == 3 ? 0x1.2f684af684bdep+4 : 0x1.0db20937d5dcdp+7; }
template <bool MASKED> __device__ __forceinline__ RsqSplit<double> rsqrt_cubic83_split(double r2, const RsqConst<double>& K) {
  const double y = rsqrt_masked<0, MASKED>(r2, K);
  const double z = __builtin_fma(r2, y * y, -K.c53);
  return {y, __builtin_fma(z, z, K.k209)};
}
template <bool MASKED> __device__ __forceinline__ double rsqrt_cubic83(double r2, const RsqConst<double>& K) {
  const RsqSplit<double> s = rsqrt_cubic83_split<MASKED>(r2, K);
  return s.y * s.p;
}
// fp32 never runs MODE 2 (capi.hip: mode_for); kept consistent with the shared scale factor
template <bool MASKED> __device__ __forceinline__ float rsqrt_cubic83(float r2, const RsqConst<float>& K) { return rsqrt_masked<1, MASKED>(r2, K) * (float)cubic83_factor(1); }
// 1/r times the factor Ker::acc_factor(MODE) accounts for, for a kernel whose terms all carry the same power of 1/r
// (A/B against the five-instruction Halley step, one box: profiles/r03_ab_cubic83.txt, +11 % on the headline)
template <int MODE, bool MASKED, class R> __device__ __forceinline__ R rsqrt_scaled(R r2, const RsqConst<R>& K) {
  if constexpr (MODE == 1) return rsqrt_newton2<MASKED>(r2, K);
  else if constexpr (MODE == 2) return rsqrt_cubic83<MASKED>(r2, K);
  else return rsqrt_masked<0, MASKED>(r2, K);
}
// ... as the factors {y0, P} with y0 P = rsqrt_scaled<MODE> (fp64; MODE 0: P = 1).  Both refinements depend on r2 only through w = r2 y0^2, so they
// are scale-invariant: for r2 = k r^2 the seed is y0 = 1 / (sqrt(k) r) and y0 P is the mode's C / r times 1 / sqrt(k), with the same relative error.
template <int MODE, bool MASKED> __device__ __forceinline__ RsqSplit<double> rsqrt_scaled_split(double r2, const RsqConst<double>& K) {
  if constexpr (MODE == 1) return rsqrt_newton2_split<MASKED>(r2, K);
  else if constexpr (MODE == 2) return rsqrt_cubic83_split<MASKED>(r2, K);
  else return {rsqrt_masked<0, MASKED>(r2, K), 1.0};
}
constexpr double rsqrt_scaled_factor(int mode, int p) { return mode == 1 ? newton2_factor(p) : mode == 2 ? cubic83_factor(p) : 1; }
// r^-3 and r^-5 for the kernels that need only that power (double layer, gradient, stresslet, traction).  MODE 2 does not cube the refined 1/r:
// (1 - e)^(-3/2) = 1 + 3/2 e + 15/8 e^2 + ... and (1 - e)^(-5/2) = 1 + 5/2 e + 35/8 e^2 + ... are again monic quadratics in w = r2 y0^2 up to a
// factor, 15/8 ((w - 7/5)^2 + 28/75) and 35/8 ((w - 9/7)^2 + 36/245), so
//     y0 s ((r2 s - 7/5)^2 + 28/75) = (8/15) / r^3,      y0 s^2 ((r2 s - 9/7)^2 + 36/245) = (8/35) / r^5,      s = y0^2,
// in five and six instructions where the cubic step and its powers take six and seven, and with fewer roundings on the way.  Constants as for
// the first power: c - 1 = 2/5 (2/7) rounded to a 25-bit multiple of 3 (5), A = 4/3 (c - 1) (4/5 (c - 1)) and k = A - (c - 1)^2 exact doubles, so
// that the ratio of the polynomial's first two coefficients is exactly 3/2 (5/2) and the factor A needs no rounding.
constexpr double kCubic3A = 0x1.1111100000000p-1, kCubic5A = 0x1.d41d400000000p-3;
template <bool MASKED> __device__ __forceinline__ double rsqrt3_cubic(double r2, const RsqConst<double>& K) {
  const double y = rsqrt_masked<0, MASKED>(r2, K), s = y * y;
  const double z = __builtin_fma(r2, s, -K.c3);
  return (y * s) * __builtin_fma(z, z, K.k3);
}
template <bool MASKED> __device__ __forceinline__ double rsqrt5_cubic(double r2, const RsqConst<double>& K) {
  const double y = rsqrt_masked<0, MASKED>(r2, K), s = y * y;
  const double z = __builtin_fma(r2, s, -K.c5);
  return (y * (s * s)) * __builtin_fma(z, z, K.k5);
}
constexpr double rsqrt_pow_factor(int mode, int p) { return mode == 2 ? (p == 1 ? cubic83_factor(1) : p == 3 ? kCubic3A : kCubic5A) : rsqrt_scaled_factor(mode, p); }
// r^-P times rsqrt_pow_factor(MODE, P), P = 3 or 5
template <int MODE, int P, bool MASKED, class R> __device__ __forceinline__ R rsqrt_pow_scaled(R r2, const RsqConst<R>& K) {
  static_assert(P == 3 || P == 5, "powers 3 and 5");
  if constexpr (MODE == 2 && std::is_same<R, double>::value) return P == 3 ? rsqrt3_cubic<MASKED>(r2, K) : rsqrt5_cubic<MASKED>(r2, K);
  else if constexpr (MODE == 2) {   // fp32 never runs MODE 2 (capi.hip: mode_for); kept consistent with the shared scale factor
    const R y = rsqrt_masked<1, MASKED>(r2, K), y2 = y * y;
    return (P == 3 ? y2 * y : y2 * y2 * y) * R(rsqrt_pow_factor(2, P));
  } else {
    const R y = rsqrt_scaled<MODE, MASKED>(r2, K), y2 = y * y;
    return P == 3 ? y2 * y : y2 * y2 * y;
  }
}

// Kernels whose terms carry SEVERAL powers of 1/r — Stokeslet-like u = (f + (r.f) r / r^2) / r — can use the unnormalised y = C / r as well when
// the record keeps the density twice: f for the dot product, whose term then carries y^3 = C^3 / r^3, and C^2 f for the term in y alone.  One
// fp64 instruction per pair less, paid with K0 more reals per source in LDS; the factor C^3 goes into the scale.  rsqrt_scaled_c2 is C^2: 4
// (exact) for the Newton step, A^2 (A has 24 bits: exact) for the cubic step, 1 for the bare seed.
constexpr double rsqrt_scaled_c2(int mode) { return rsqrt_scaled_factor(mode, 1) == 1 ? 1.0 : mode == 1 ? 4.0 : cubic83_factor(1) * cubic83_factor(1); }

// 1/r of the gradient forms: the normalised rsqrt_masked of the mode, except that fp32 never takes the bare seed.  A gradient raises y to the powers p + 2 = 3 .. 7,
// so the seed's 2^-23.3 becomes several ulp per pair, and it does not average out over a sum (measured, Laplace3D-FDxUdU fp32 300 x 2000: rel-L2 5.1e-7 with the seed,
// 2.0e-7 with one Newton step, 0.7e-7 for the same formula in torch float32): "full precision of fp32" costs the gradient three more fp32 instructions per pair.
template <int MODE, bool MASKED, class R> __device__ __forceinline__ R rsqrt_grad(R r2, const RsqConst<R>& K) {
  return rsqrt_masked<(std::is_same<R, float>::value && MODE == 0) ? 1 : MODE, MASKED>(r2, K);
}

// The gradient of the Stokeslet family, phi = fw y + A B y^3 with y = 1/r, A and B linear in d with gradients f and w (three components each):
//   grad phi = y^3 (B f + A w - d (fw + 3 A B y^2))
template <class R> __device__ __forceinline__ void stokeslet_grad(R (&G)[3], const R (&d)[3], R y, const R* f, const R* w, R A, R B, R fw) {
  const R y2 = y * y, y3 = y2 * y;
  const R c = fma_((A * B) * R(3), y2, fw);
#pragma unroll
  for (int j = 0; j < 3; j++) G[j] = fma_(y3, fma_(B, f[j], fma_(A, w[j], -(c * d[j]))), G[j]);
}

// The tangent of the Stokeslet family, u_k = f_k y + A d_k y^3 with A linear in d and dA = e.f (three components): with eps = d.e,
//   du_k = y^3 (A e_k + (e.f) d_k - eps (f_k + 3 A y^2 d_k))
template <class R> __device__ __forceinline__ void stokeslet_jvp(R* acc, const R (&d)[3], const R (&e)[3], R y, const R* f, R A, R ef) {
  const R y2 = y * y, y3 = y2 * y;
  const R eps = dot3(d, e);
  const R c = fma_((A * R(3)) * y2, eps, -ef);
#pragma unroll
  for (int j = 0; j < 3; j++) acc[j] = fma_(y3, fma_(A, e[j], -fma_(c, d[j], eps * f[j])), acc[j]);
}

// ---- gradient forms of several density / weight rows (pair_gm of every struct below) --------------------------------------------------------
// Every phi is bilinear in (f, w), so the sum over rows of phi(f_m, w_m) is the single pair's form on the K0 x K1 block C = sum_m f_m (x) w_m:
// C[a][b] += f[m][a] w[m][b] over the leading A x B corner of the rows, M FMAs per entry.
template <int A, int B, class R, int M, int K0, int K1> __device__ __forceinline__ void contract_rows(R (&C)[A][B], const R (&f)[M][K0], const R (&w)[M][K1]) {
#pragma unroll
  for (int a = 0; a < A; a++)
#pragma unroll
    for (int b = 0; b < B; b++) {
      R c = f[0][a] * w[0][b];
#pragma unroll
      for (int m = 1; m < M; m++) c = fma_(f[m][a], w[m][b], c);
      C[a][b] = c;
    }
}
// The Stokeslet family on the block C (and, for FSxU / FxUP, the 3-vector s of its extra row or column): phi = tr C y + (d^T C d + d.s) y^3, so with
// u = (C + C^T) d, q = (d.u) / 2 + d.s:   grad phi = y^3 (u + s - d (tr C + 3 q y^2)).  EXTRA: there is an s (Stokes3D-FxU has none)
template <bool EXTRA, class R> __device__ __forceinline__ void stokeslet_grad_c(R (&G)[3], const R (&d)[3], R y, const R (&C)[3][3], const R (&s)[3]) {
  const R y2 = y * y, y3 = y2 * y;
  R u[3];
#pragma unroll
  for (int j = 0; j < 3; j++) u[j] = fma_(C[j][2] + C[2][j], d[2], fma_(C[j][1] + C[1][j], d[1], (C[j][0] + C[0][j]) * d[0]));
  R q = dot3(d, u) * R(0.5);
  if constexpr (EXTRA) {
    q += dot3(d, s);
#pragma unroll
    for (int j = 0; j < 3; j++) u[j] += s[j];
  }
  const R c = fma_(q * R(3), y2, (C[0][0] + C[1][1]) + C[2][2]);
#pragma unroll
  for (int j = 0; j < 3; j++) G[j] = fma_(y3, fma_(-c, d[j], u[j]), G[j]);
}

// ---- multi-density records (pack_m / pair_m of every struct below) -------------------------------------------------
constexpr int nrec_multi(int nd, int k0, int m) { return (3 + nd + m * k0 + 1) / 2 * 2; }
template <int ND, int K0, class R, int M> __device__ __forceinline__ void pack_multi(R* rec, const R* x, const R* n, const R (&f)[M][K0]) {
  rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2];
#pragma unroll
  for (int k = 0; k < ND; k++) rec[3 + k] = n[k];
#pragma unroll
  for (int m = 0; m < M; m++)
#pragma unroll
    for (int k = 0; k < K0; k++) rec[3 + ND + m * K0 + k] = f[m][k];
}
#define SCTL_AMD_MULTI_RECORD                                                                                                          \
  template <int M> static constexpr int NREC_M = nrec_multi(ND, K0, M);                                                               \
  template <class R, int M> static __device__ __forceinline__ void pack_m(R* rec, const R* x, const R* n, const R (&f)[M][K0]) {      \
    pack_multi<ND, K0>(rec, x, n, f);                                                                                                 \
  }
// ---- transposed records of several weight vectors (pack_tm / pair_tm of every struct below): x_t, then M x `per_w` reals ---------------
constexpr int nrec_tm(int per_w, int m) { return (3 + m * per_w + 1) / 2 * 2; }
#define SCTL_AMD_MULTI_T_RECORD                                                                                                        \
  template <int M> static constexpr int NREC_TM = nrec_tm(K1, M);                                                                     \
  template <class R, int M> static __device__ __forceinline__ void pack_tm(R* rec, const R* x, const R (&w)[M][K1]) {                 \
    pack_multi<0, K1>(rec, x, (const R*)nullptr, w);                                                                                  \
  }

// ---- Laplace single layer: u = f / r          (kernel_functions.hpp:15-31) -------------------------------
struct Laplace3D_FxU {
  static constexpr int ID = 0, K0 = 1, K1 = 1, ND = 0, NREC = 4, FLOPS = 6;
  static constexpr const char* NAME = "Laplace3D-FxU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 1 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 1); }   // MODE 1 accumulates f (2/r), MODE 2 f (8/3)/r
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R rinv = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);   // MODE 1: 2/r, MODE 2: (8/3)/r
    acc[0] = fma_(rec[3], rinv, acc[0]);
  }
  // multi: 1 FMA per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R rinv = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);
#pragma unroll
    for (int m = 0; m < M; m++) acc[m][0] = fma_(rec[3 + m], rinv, acc[m][0]);
  }
  // transposed: the kernel is symmetric, g += w / r; record x_t, w
  static constexpr int NREC_T = 4;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) { rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    acc[0] = fma_(rec[3], rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq), acc[0]);
  }
  // transposed, several weights: 1 FMA per weight vector
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R rinv = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);
#pragma unroll
    for (int m = 0; m < M; m++) acc[m][0] = fma_(rec[3 + m], rinv, acc[m][0]);
  }
  // gradient: phi = w f y, grad_d = -(w f) y^3 d
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R t = (f[0] * w[0]) * ((y * y) * y);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(-t, d[j], G[j]);
  }
  // tangent: u = f y, du = -f y^3 (d.e)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    acc[0] = fma_(-(f[0] * ((y * y) * y)), dot3(d, e), acc[0]);
  }
  // gradient, several rows: the scalar c = sum_m w_m f_m (M instructions), then pair_g with c for w f
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    R c[1][1];
    contract_rows(c, f, w);
    const R t = c[0][0] * ((y * y) * y);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(-t, d[j], G[j]);
  }
};

// ---- Laplace double layer: u = (r.n) f / r^3   (kernel_functions.hpp:33-51); record holds n*f ------------
struct Laplace3D_DxU {
  static constexpr int ID = 1, K0 = 1, K1 = 1, ND = 3, NREC = 6, FLOPS = 14;
  static constexpr const char* NAME = "Laplace3D-DxU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 1 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_pow_factor(mode, 3); }   // MODE 1 accumulates (r.n f) (2/r)^3, MODE 2 (r.n f) (8/15) / r^3
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = n[0] * f[0]; rec[4] = n[1] * f[0]; rec[5] = n[2] * f[0];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    acc[0] = fma_(dot3(d, rec + 3), rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq), acc[0]);
  }
  // multi: the record keeps n, each density is one FMA on (r.n) / r^3
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = dot3(d, rec + 3) * rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq);
#pragma unroll
    for (int m = 0; m < M; m++) acc[m][0] = fma_(rec[6 + m], t, acc[m][0]);
  }
  // transposed: g += (d.n) w / r^3 with the owner's n in registers: nothing of the pair can be pre-multiplied into the record, so w costs one
  // multiplication more than the forward pair's n f; record x_t, w
  static constexpr int NREC_T = 4;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) { rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    acc[0] = fma_(dot3(d, n), rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq) * rec[3], acc[0]);
  }
  // transposed, several weights: (d.n) / r^3 once, 1 FMA per weight vector
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = dot3(d, n) * rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq);
#pragma unroll
    for (int m = 0; m < M; m++) acc[m][0] = fma_(rec[3 + m], t, acc[m][0]);
  }
  // gradient: phi = c (d.n) y^3 with c = w f: grad_d = c y^3 (n - 3 (d.n) y^2 d), grad_n = c y^3 d
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R a = (f[0] * w[0]) * (y2 * y);
    const R b = (dot3(d, n) * R(-3)) * (y2 * a);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(a, n[j], fma_(b, d[j], G[j]));
    if constexpr (WANT_N) {
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(a, d[j], N[j]);
    }
  }
  // tangent: u = f (d.n) y^3, du = f y^3 (e.n + d.m - 3 (d.n) (d.e) y^2)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R a = f[0] * (y2 * y);
    const R s = fma_((dot3(d, n) * R(-3)) * y2, dot3(d, e), dot3(e, n) + dot3(d, m));
    acc[0] = fma_(a, s, acc[0]);
  }
  // gradient, several rows: the scalar c = sum_m w_m f_m (M instructions), then pair_g with c for w f
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    R c[1][1];
    contract_rows(c, f, w);
    const R a = c[0][0] * (y2 * y);
    const R b = (dot3(d, n) * R(-3)) * (y2 * a);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(a, n[j], fma_(b, d[j], G[j]));
    if constexpr (WANT_N) {
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(a, d[j], N[j]);
    }
  }
};

// ---- gradient of the Laplace single layer: u_j = f r_j / r^3, scale -1/(4 pi)   (kernel_functions.hpp:53-72)
struct Laplace3D_FxdU {
  static constexpr int ID = 2, K0 = 1, K1 = 3, ND = 0, NREC = 4, FLOPS = 11;
  static constexpr const char* NAME = "Laplace3D-FxdU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return -1 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_pow_factor(mode, 3); }   // MODE 1 accumulates f r (2/r)^3, MODE 2 f r (8/15) / r^3
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq) * rec[3];
    for (int j = 0; j < 3; j++) acc[j] = fma_(t, d[j], acc[j]);
  }
  // multi: r / r^3 once, 3 FMAs per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq);
    const R td[3] = {t * d[0], t * d[1], t * d[2]};
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(rec[3 + m], td[j], acc[m][j]);
  }
  // transposed: g += (d.w) / r^3, one dot product and one FMA; record x_t, w[3]
  static constexpr int NREC_T = 6;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; rec[4] = w[1]; rec[5] = w[2];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    acc[0] = fma_(dot3(d, rec + 3), rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq), acc[0]);
  }
  // transposed, several weights: d / r^3 once, 3 FMAs per weight vector
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = rsqrt_pow_scaled<MODE, 3, MASKED>(len2(d), K.rsq);
    const R td[3] = {t * d[0], t * d[1], t * d[2]};
#pragma unroll
    for (int m = 0; m < M; m++) acc[m][0] = fma_(td[2], rec[5 + 3 * m], fma_(td[1], rec[4 + 3 * m], fma_(td[0], rec[3 + 3 * m], acc[m][0])));
  }
  // gradient: phi = f (d.w) y^3: grad_d = f y^3 (w - 3 (d.w) y^2 d), the double layer's with w for n
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R a = f[0] * (y2 * y);
    const R b = (dot3(d, w) * R(-3)) * (y2 * a);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(a, w[j], fma_(b, d[j], G[j]));
  }
  // tangent: u_k = f d_k y^3, du_k = f y^3 (e_k - 3 (d.e) y^2 d_k)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R a = f[0] * (y2 * y);
    const R b = (dot3(d, e) * R(-3)) * y2;
#pragma unroll
    for (int j = 0; j < 3; j++) acc[j] = fma_(a, fma_(b, d[j], e[j]), acc[j]);
  }
  // gradient, several rows: the 3-vector v = sum_m f_m w_m (3 M instructions), then pair_g with f = 1 and w = v
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    R v[1][3];
    contract_rows(v, f, w);
    const R a = y2 * y;
    const R b = (dot3(d, v[0]) * R(-3)) * (y2 * a);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(a, v[0][j], fma_(b, d[j], G[j]));
  }
};

// ---- Stokeslet: u_j = f_j / r + (r.f) r_j / r^3, scale 1/(8 pi)   (kernel_functions.hpp:74-95) -----------
struct Stokes3D_FxU {
  static constexpr int ID = 3, K0 = 3, K1 = 3, ND = 0, NREC = 10, FLOPS = 23;
  static constexpr const char* NAME = "Stokes3D-FxU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 1 / (8 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 3); }   // pair() accumulates C^3 x the kernel value, C / r the mode's 1/r
  // record: x, f (for the dot product), C^2 f (the term in 1/r alone; rsqrt_scaled_c2)
  template <class R, int MODE> static __device__ __forceinline__ void pack_mode(R* rec, const R* x, const R*, const R* f) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; rec[4] = f[1]; rec[5] = f[2]; rec[6] = c2 * f[0]; rec[7] = c2 * f[1]; rec[8] = c2 * f[2]; rec[9] = 0;
  }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) { pack_mode<R, 0>(rec, x, n, f); }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R t = dot3(d, rec + 3) * (y * y);                                                  // C^2 (r.f) / r^2
    for (int j = 0; j < 3; j++) acc[j] = fma_(y, fma_(t, d[j], rec[6 + j]), acc[j]);         // C^3 (f_j + r_j (r.f) / r^2) / r: 1/r^3 is never formed
  }
  // multi: C^3 (f_j / r + (r.f) r_j / r^3) with r / r^3 and 1/r formed once; 9 instructions per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R y3 = (y * y) * y;
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));           // C^2 (C / r): the term in 1/r alone
    const R e[3] = {y3 * d[0], y3 * d[1], y3 * d[2]};                                         // C^3 r / r^3
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* f = rec + 3 + 3 * m;
      const R rf = dot3(d, f);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(e[j], rf, fma_(yc, f[j], acc[m][j]));
    }
  }
  // transposed: the block is symmetric, g = w / r + (d.w) d / r^3: the forward record and pair with w for f
  static constexpr int NREC_T = NREC;
  template <class R, int MODE> static __device__ __forceinline__ void pack_t_mode(R* rec, const R* x, const R* w) { pack_mode<R, MODE>(rec, x, nullptr, w); }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    pair<R, MODE, MASKED>(acc, d, rec, KerCtx{}, K);
  }
  // transposed, several weights: the block is symmetric, so pair_m with w for f (9 instructions per weight vector)
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx& ctx, const Consts<R>& K) {
    pair_m<R, MODE, MASKED, M>(acc, d, rec, ctx, K);
  }
  // gradient: phi = (f.w) y + (d.f)(d.w) y^3 (stokeslet_grad)
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    stokeslet_grad(G, d, y, f, w, dot3(d, f), dot3(d, w), dot3(f, w));
  }
  // tangent: u_k = f_k y + (d.f) d_k y^3 (stokeslet_jvp)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    stokeslet_jvp(acc, d, e, y, f, dot3(d, f), dot3(e, f));
  }
  // gradient, several rows: the 3 x 3 block C = sum_m f_m (x) w_m (9 M instructions), then stokeslet_grad_c
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    R C[3][3];
    contract_rows(C, f, w);
    const R s[3] = {0, 0, 0};
    stokeslet_grad_c<false>(G, d, y, C, s);
  }
};

// ---- stresslet: u_j = r_j (r.f)(r.n) / r^5, scale 3/(4 pi)   (kernel_functions.hpp:97-120) ----------------
struct Stokes3D_DxU {
  static constexpr int ID = 4, K0 = 3, K1 = 3, ND = 3, NREC = 10, FLOPS = 26;
  static constexpr const char* NAME = "Stokes3D-DxU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 3 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_pow_factor(mode, 5); }   // MODE 1 accumulates (...) (2/r)^5, MODE 2 (...) (8/35) / r^5
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) {
    for (int k = 0; k < 3; k++) { rec[k] = x[k]; rec[3 + k] = n[k]; rec[6 + k] = f[k]; }
    rec[9] = 0;
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = dot3(d, rec + 3) * dot3(d, rec + 6) * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    for (int j = 0; j < 3; j++) acc[j] = fma_(t, d[j], acc[j]);
  }
  // multi: (r.n) r / r^5 once, (r.f) and 3 FMAs per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R g = dot3(d, rec + 3) * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    const R gd[3] = {g * d[0], g * d[1], g * d[2]};
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R rf = dot3(d, rec + 6 + 3 * m);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(gd[j], rf, acc[m][j]);
    }
  }
  // transposed: g_i += d_i (d.w)(d.n) / r^5, the forward pair with the owner's n from registers; record x_t, w[3]
  static constexpr int NREC_T = 6;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; rec[4] = w[1]; rec[5] = w[2];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = dot3(d, n) * dot3(d, rec + 3) * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    for (int j = 0; j < 3; j++) acc[j] = fma_(t, d[j], acc[j]);
  }
  // transposed, several weights: (d.n) d / r^5 once, (d.w) and 3 FMAs per weight vector
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R g = dot3(d, n) * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    const R gd[3] = {g * d[0], g * d[1], g * d[2]};
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R dw = dot3(d, rec + 3 + 3 * m);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(gd[j], dw, acc[m][j]);
    }
  }
  // gradient: phi = a b c y^5 with a = d.n, b = d.f, c = d.w: grad_d = y^5 (bc n + ac f + ab w - 5 abc y^2 d), grad_n = bc y^5 d
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    const R a = dot3(d, n), b = dot3(d, f), c = dot3(d, w);
    const R bc = b * c, ac = a * c, ab = a * b;
    const R e = (ab * c) * (y2 * R(-5));
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(y5, fma_(bc, n[j], fma_(ac, f[j], fma_(ab, w[j], e * d[j]))), G[j]);
    if constexpr (WANT_N) {
      const R t = bc * y5;
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(t, d[j], N[j]);
    }
  }
  // tangent: u_k = a b d_k y^5 with a = d.n, b = d.f: du_k = y^5 (ab e_k + ((e.n + d.m) b + a (e.f) - 5 ab (d.e) y^2) d_k)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    const R a = dot3(d, n), b = dot3(d, f), ab = a * b;
    const R da = dot3(e, n) + dot3(d, m);
    const R c = fma_(ab * dot3(d, e), y2 * R(-5), fma_(da, b, a * dot3(e, f)));
#pragma unroll
    for (int j = 0; j < 3; j++) acc[j] = fma_(y5, fma_(ab, e[j], c * d[j]), acc[j]);
  }
  // gradient, several rows: the 3 x 3 block C = sum_m f_m (x) w_m (9 M instructions); phi = a q y^5 with a = d.n, q = d^T C d and u = (C + C^T) d = grad q:
  //   grad_d = y^5 (q n + a u - 5 a q y^2 d), grad_n = q y^5 d
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    R C[3][3], u[3];
    contract_rows(C, f, w);
#pragma unroll
    for (int j = 0; j < 3; j++) u[j] = fma_(C[j][2] + C[2][j], d[2], fma_(C[j][1] + C[1][j], d[1], (C[j][0] + C[0][j]) * d[0]));
    const R q = dot3(d, u) * R(0.5);
    const R a = dot3(d, n);
    const R e = (a * q) * (y2 * R(-5));
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(y5, fma_(q, n[j], fma_(a, u[j], e * d[j])), G[j]);
    if constexpr (WANT_N) {
      const R t = q * y5;
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(t, d[j], N[j]);
    }
  }
};

// ---- traction tensor: u_{jk} = (r.f) r_j r_k / r^5, scale -3/(4 pi)   (kernel_functions.hpp:122-146) -------
struct Stokes3D_FxT {
  static constexpr int ID = 5, K0 = 3, K1 = 9, ND = 0, NREC = 6, FLOPS = 39;
  static constexpr const char* NAME = "Stokes3D-FxT";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return -3 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_pow_factor(mode, 5); }   // MODE 1 accumulates (...) (2/r)^5, MODE 2 (...) (8/35) / r^5
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; rec[4] = f[1]; rec[5] = f[2];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R t = dot3(d, rec + 3) * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    for (int j = 0; j < 3; j++) {       // u_jk = u_kj: the upper triangle only (6 FMAs instead of 9); finish() fills in the rest
      const R tj = t * d[j];
      for (int k = j; k < 3; k++) acc[j * 3 + k] = fma_(tj, d[k], acc[j * 3 + k]);
    }
  }
  // multi: the six r_j r_k / r^5 once, (r.f) and 6 FMAs per density (upper triangle; finish() per density)
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R p = rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    R dd[6];
    int q = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const R pj = p * d[j];
#pragma unroll
      for (int k = j; k < 3; k++) dd[q++] = pj * d[k];
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R rf = dot3(d, rec + 3 + 3 * m);
      int i = 0;
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = j; k < 3; k++, i++) acc[m][j * 3 + k] = fma_(dd[i], rf, acc[m][j * 3 + k]);
    }
  }
  template <class R> static __device__ __forceinline__ void finish(R (&acc)[K1]) { acc[3] = acc[1]; acc[6] = acc[2]; acc[7] = acc[5]; }
  // transposed: g_i += d_i (d^T W d) / r^5 for the full 3 x 3 weight W = w[j*3+k] (no symmetry assumed).  Only the symmetric part of W enters the
  // quadratic form, so the record holds S = the diagonal and the sums W_jk + W_kj (j < k): d^T W d in 9 instructions where the nine entries take 12.
  // record x_t, S00 S01 S02 S11 S12 S22
  static constexpr int NREC_T = 10;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2];
    rec[3] = w[0]; rec[4] = w[1] + w[3]; rec[5] = w[2] + w[6]; rec[6] = w[4]; rec[7] = w[5] + w[7]; rec[8] = w[8]; rec[9] = 0;
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R a0 = fma_(rec[5], d[2], fma_(rec[4], d[1], rec[3] * d[0]));
    const R a1 = fma_(rec[7], d[2], rec[6] * d[1]);
    const R q = fma_(d[2] * rec[8], d[2], fma_(a1, d[1], a0 * d[0]));
    const R t = q * rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    for (int j = 0; j < 3; j++) acc[j] = fma_(t, d[j], acc[j]);
  }
  // transposed, several weights: the six d_j d_k / r^5 once; per weight vector the quadratic form against its six symmetric sums (6 instructions) and
  // 3 FMAs.  record x_t, then S00 S01 S02 S11 S12 S22 of each weight vector (pack_t's sums)
  template <int M> static constexpr int NREC_TM = nrec_tm(6, M);
  template <class R, int M> static __device__ __forceinline__ void pack_tm(R* rec, const R* x, const R (&w)[M][K1]) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2];
#pragma unroll
    for (int m = 0; m < M; m++) {
      R* s = rec + 3 + 6 * m;
      s[0] = w[m][0]; s[1] = w[m][1] + w[m][3]; s[2] = w[m][2] + w[m][6]; s[3] = w[m][4]; s[4] = w[m][5] + w[m][7]; s[5] = w[m][8];
    }
  }
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R p = rsqrt_pow_scaled<MODE, 5, MASKED>(len2(d), K.rsq);
    R dd[6];
    int q = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const R pj = p * d[j];
#pragma unroll
      for (int k = j; k < 3; k++) dd[q++] = pj * d[k];
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* s = rec + 3 + 6 * m;
      R t = s[0] * dd[0];
#pragma unroll
      for (int i = 1; i < 6; i++) t = fma_(s[i], dd[i], t);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(t, d[j], acc[m][j]);
    }
  }
  // gradient: phi = A q y^5 with A = d.f and q = d^T W d, W = w[j*3+k]: with v = (W + W^T) d = grad q and q = (d.v) / 2,
  //   grad_d = y^5 (q f + A v - 5 A q y^2 d)
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    R v[3];
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = fma_(w[j * 3 + 2] + w[6 + j], d[2], fma_(w[j * 3 + 1] + w[3 + j], d[1], (w[j * 3] + w[j]) * d[0]));
    const R q = dot3(d, v) * R(0.5);
    const R A = dot3(d, f);
    const R e = (A * q) * (y2 * R(-5));
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(y5, fma_(q, f[j], fma_(A, v[j], e * d[j])), G[j]);
  }
  // tangent: u_jk = A d_j d_k y^5 with A = d.f: du_jk = y^5 (g_j d_k + A d_j e_k), g = (e.f - 5 A (d.e) y^2) d + A e
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    const R A = dot3(d, f);
    const R c = fma_(A * dot3(d, e), y2 * R(-5), dot3(e, f));
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const R g = fma_(c, d[j], A * e[j]), Ad = A * d[j];
#pragma unroll
      for (int k = 0; k < 3; k++) acc[j * 3 + k] = fma_(y5, fma_(g, d[k], Ad * e[k]), acc[j * 3 + k]);
    }
  }
  // gradient, several rows: the rank-one terms row by row (the block f (x) w has 3 x 6 distinct entries: contracting it first costs about 21 M + 80
  // instructions and 18 more registers against 29 M + 26 here: 164 against 142 at M = 4).  Per row v, q and A as in pair_g, summed unscaled; y^5 and
  // y^2 applied once.
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y5 = (y2 * y2) * y;
    R H[3] = {0, 0, 0}, S = 0;
#pragma unroll
    for (int m = 0; m < M; m++) {
      R v[3];
#pragma unroll
      for (int j = 0; j < 3; j++) v[j] = fma_(w[m][j * 3 + 2] + w[m][6 + j], d[2], fma_(w[m][j * 3 + 1] + w[m][3 + j], d[1], (w[m][j * 3] + w[m][j]) * d[0]));
      const R q = dot3(d, v) * R(0.5);
      const R A = dot3(d, f[m]);
      S = fma_(A, q, S);
#pragma unroll
      for (int j = 0; j < 3; j++) H[j] = fma_(q, f[m][j], fma_(A, v[j], H[j]));
    }
    const R e = S * (y2 * R(-5));
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(y5, fma_(e, d[j], H[j]), G[j]);
  }
};

// ---- Stokeslet + source/sink: u_j = f_j / r + ((r.f) + f_3) r_j / r^3   (kernel_functions.hpp:148-172) ------
struct Stokes3D_FSxU {
  static constexpr int ID = 6, K0 = 4, K1 = 3, ND = 0, NREC = 10, FLOPS = 26;
  static constexpr const char* NAME = "Stokes3D-FSxU";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 1 / (8 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 3); }   // as the Stokeslet: C^3 x the kernel value
  template <class R, int MODE> static __device__ __forceinline__ void pack_mode(R* rec, const R* x, const R*, const R* f) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; rec[4] = f[1]; rec[5] = f[2]; rec[6] = f[3]; rec[7] = c2 * f[0]; rec[8] = c2 * f[1]; rec[9] = c2 * f[2];
  }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) { pack_mode<R, 0>(rec, x, n, f); }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                                 // C / r
    const R t = fma_(d[2], rec[5], fma_(d[1], rec[4], fma_(d[0], rec[3], rec[6]))) * (y * y);               // C^2 ((r.f) + f_3) / r^2
    for (int j = 0; j < 3; j++) acc[j] = fma_(y, fma_(t, d[j], rec[7 + j]), acc[j]);
  }
  // multi: as the Stokeslet's, with f_3 in the dot product
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R y3 = (y * y) * y;
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));           // C^2 (C / r): the term in 1/r alone
    const R e[3] = {y3 * d[0], y3 * d[1], y3 * d[2]};                                         // C^3 r / r^3
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* f = rec + 3 + 4 * m;
      const R rf = fma_(d[2], f[2], fma_(d[1], f[1], fma_(d[0], f[0], f[3])));
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(e[j], rf, fma_(yc, f[j], acc[m][j]));
    }
  }
  // transposed: three Stokeslet rows g_i += w_i / r + (d.w) d_i / r^3 and g_3 += (d.w) / r^3 — the velocity + pressure kernel's forward arithmetic
  // record x_t, w (for the dot product), C^2 w
  static constexpr int NREC_T = 10;
  template <class R, int MODE> static __device__ __forceinline__ void pack_t_mode(R* rec, const R* x, const R* w) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; rec[4] = w[1]; rec[5] = w[2]; rec[6] = c2 * w[0]; rec[7] = c2 * w[1]; rec[8] = c2 * w[2]; rec[9] = 0;
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);
    const R t = dot3(d, rec + 3) * (y * y);
    for (int j = 0; j < 3; j++) acc[j] = fma_(y, fma_(t, d[j], rec[6 + j]), acc[j]);
    acc[3] = fma_(t, y, acc[3]);
  }
  // transposed, several weights: the velocity + pressure kernel's pair_m with w for f (10 instructions per weight vector)
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R y3 = (y * y) * y;
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));           // C^2 (C / r): the term in 1/r alone
    const R e[3] = {y3 * d[0], y3 * d[1], y3 * d[2]};                                         // C^3 d / r^3
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* w = rec + 3 + 3 * m;
      const R dw = dot3(d, w);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(e[j], dw, fma_(yc, w[j], acc[m][j]));
      acc[m][3] = fma_(y3, dw, acc[m][3]);
    }
  }
  // gradient: phi = (f.w) y + ((d.f) + f_3)(d.w) y^3, the Stokeslet's with A = (d.f) + f_3 (stokeslet_grad)
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    stokeslet_grad(G, d, y, f, w, fma_(d[2], f[2], fma_(d[1], f[1], fma_(d[0], f[0], f[3]))), dot3(d, w), dot3(w, f));
  }
  // tangent: the Stokeslet's with A = (d.f) + f_3; e.f over the three force components (stokeslet_jvp)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    stokeslet_jvp(acc, d, e, y, f, fma_(d[2], f[2], fma_(d[1], f[1], fma_(d[0], f[0], f[3]))), dot3(e, f));
  }
  // gradient, several rows: the 4 x 3 block C = sum_m f_m (x) w_m (12 M instructions); its last row is the source / sink's s (stokeslet_grad_c)
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    R C4[4][3];
    contract_rows(C4, f, w);
    const R C[3][3] = {{C4[0][0], C4[0][1], C4[0][2]}, {C4[1][0], C4[1][1], C4[1][2]}, {C4[2][0], C4[2][1], C4[2][2]}};
    stokeslet_grad_c<true>(G, d, y, C, C4[3]);
  }
};

// ---- velocity + pressure: Stokeslet and p = (r.f) / r^3   (kernel_functions.hpp:174-198) -------------------
struct Stokes3D_FxUP {
  static constexpr int ID = 7, K0 = 3, K1 = 4, ND = 0, NREC = 10, FLOPS = 26;
  static constexpr const char* NAME = "Stokes3D-FxUP";
  template <class R> using Consts = DefaultConsts<R>;
  static constexpr double scale() { return 1 / (8 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 3); }   // velocity as the Stokeslet; the pressure (r.f) / r^3 carries C^3 by itself
  template <class R, int MODE> static __device__ __forceinline__ void pack_mode(R* rec, const R* x, const R*, const R* f) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; rec[4] = f[1]; rec[5] = f[2]; rec[6] = c2 * f[0]; rec[7] = c2 * f[1]; rec[8] = c2 * f[2]; rec[9] = 0;
  }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) { pack_mode<R, 0>(rec, x, n, f); }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);
    const R t = dot3(d, rec + 3) * (y * y);
    for (int j = 0; j < 3; j++) acc[j] = fma_(y, fma_(t, d[j], rec[6 + j]), acc[j]);
    acc[3] = fma_(t, y, acc[3]);
  }
  // multi: the Stokeslet's form plus the pressure (r.f) C^3 / r^3, 10 instructions per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R y3 = (y * y) * y;
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));           // C^2 (C / r): the term in 1/r alone
    const R e[3] = {y3 * d[0], y3 * d[1], y3 * d[2]};                                         // C^3 r / r^3
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* f = rec + 3 + 3 * m;
      const R rf = dot3(d, f);
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(e[j], rf, fma_(yc, f[j], acc[m][j]));
      acc[m][3] = fma_(y3, rf, acc[m][3]);
    }
  }
  // transposed: g_i += w_i / r + ((d.w_u) + w_p) d_i / r^3, the Stokeslet of the velocity weights plus d w_p / r^3 — the source/sink kernel's
  // forward arithmetic.  record x_t, w_u, w_p, C^2 w_u
  static constexpr int NREC_T = 10;
  template <class R, int MODE> static __device__ __forceinline__ void pack_t_mode(R* rec, const R* x, const R* w) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; rec[4] = w[1]; rec[5] = w[2]; rec[6] = w[3]; rec[7] = c2 * w[0]; rec[8] = c2 * w[1]; rec[9] = c2 * w[2];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);
    const R t = fma_(d[2], rec[5], fma_(d[1], rec[4], fma_(d[0], rec[3], rec[6]))) * (y * y);
    for (int j = 0; j < 3; j++) acc[j] = fma_(y, fma_(t, d[j], rec[7 + j]), acc[j]);
  }
  // transposed, several weights: the source/sink kernel's pair_m with w for f (9 instructions per weight vector)
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);                                  // C / r
    const R y3 = (y * y) * y;
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));           // C^2 (C / r): the term in 1/r alone
    const R e[3] = {y3 * d[0], y3 * d[1], y3 * d[2]};                                         // C^3 d / r^3
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R* w = rec + 3 + 4 * m;
      const R dw = fma_(d[2], w[2], fma_(d[1], w[1], fma_(d[0], w[0], w[3])));               // (d.w_u) + w_p
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][j] = fma_(e[j], dw, fma_(yc, w[j], acc[m][j]));
    }
  }
  // gradient: phi = (f.w_u) y + (d.f)((d.w_u) + w_p) y^3, the Stokeslet's with B = (d.w_u) + w_p (stokeslet_grad)
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    stokeslet_grad(G, d, y, f, w, dot3(d, f), fma_(d[2], w[2], fma_(d[1], w[1], fma_(d[0], w[0], w[3]))), dot3(f, w));
  }
  // tangent: the velocity as the Stokeslet (stokeslet_jvp); the pressure p = A y^3 with A = d.f: dp = y^3 (e.f - 3 A (d.e) y^2)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R A = dot3(d, f), ef = dot3(e, f);
    stokeslet_jvp(acc, d, e, y, f, A, ef);
    const R y2 = y * y;
    acc[3] = fma_(y2 * y, fma_((A * R(-3)) * y2, dot3(d, e), ef), acc[3]);
  }
  // gradient, several rows: the 3 x 4 block C = sum_m f_m (x) w_m (12 M instructions); its last column is the pressure's s (stokeslet_grad_c)
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    R C4[3][4];
    contract_rows(C4, f, w);
    const R C[3][3] = {{C4[0][0], C4[0][1], C4[0][2]}, {C4[1][0], C4[1][1], C4[1][2]}, {C4[2][0], C4[2][1], C4[2][2]}};
    const R s[3] = {C4[0][3], C4[1][3], C4[2][3]};
    stokeslet_grad_c<true>(G, d, y, C, s);
  }
};

// ---- NEW: Laplace single + double layer -> potential and gradient (BASELINE config 2) -----
//   u      = q / r + mu (r.n) / r^3
//   grad u = -q r / r^3 + mu ( n / r^3 - 3 (r.n) r / r^5 ),    scale 1/(4 pi);  record holds m = mu * n and q.
template <class R> struct FDxUdUConsts : DefaultConsts<R> {   // + the constant 3 in a register for the whole kernel (no inline constant; re-made per source otherwise)
  R c3;
  __device__ __forceinline__ explicit FDxUdUConsts(double* lds) : DefaultConsts<R>(lds), c3(R(3)) { asm volatile("" : "+v"(c3)); }
};
struct Laplace3D_FDxUdU {
  static constexpr int ID = 8, K0 = 2, K1 = 4, ND = 3, NREC = 10, FLOPS = 28;
  static constexpr const char* NAME = "Laplace3D-FDxUdU";
  template <class R> using Consts = FDxUdUConsts<R>;
  static constexpr double scale() { return 1 / (4 * kPi); }
  // With y = C / r (the mode's unnormalised 1/r) the gradient (m_j - r_j (q + 3 mu (r.n) / r^2)) / r^3 accumulates C^5 x its value when m and q are
  // kept as C^2 m, C^2 q beside the plain m of the dot product; the potential (q + mu (r.n) / r^2) / r then carries C^3 and is multiplied by C^2
  // once per target, when the sums leave the registers (finish_mode).
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 5); }
  // record: x, m = mu n (for the dot product), C^2 m, C^2 q
  template <class R, int MODE> static __device__ __forceinline__ void pack_mode(R* rec, const R* x, const R* n, const R* f) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2];
    rec[3] = n[0] * f[1]; rec[4] = n[1] * f[1]; rec[5] = n[2] * f[1];
    rec[6] = c2 * rec[3]; rec[7] = c2 * rec[4]; rec[8] = c2 * rec[5]; rec[9] = c2 * f[0];
  }
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) { pack_mode<R, 0>(rec, x, n, f); }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);   // C / r
    const R y2 = y * y;
    const R y3 = y2 * y;
    const R w = dot3(d, rec + 3) * y2;                      // C^2 mu (r.n) / r^2
    acc[0] = fma_(w, y, fma_(rec[9], y, acc[0]));           // C^3 (q / r + mu (r.n) / r^3)
    const R c = fma_(w, K.c3, rec[9]);                      // C^2 (q + 3 mu (r.n) / r^2)
    for (int j = 0; j < 3; j++) acc[1 + j] = fma_(y3, fma_(-d[j], c, rec[6 + j]), acc[1 + j]);   // C^5 (m_j - r_j c) / r^3
  }
  // multi: the record keeps n and (q, mu) per density.  With y = C / r, c2 = C^2 and dn = r.n, pair() accumulates
  //   u      += c2 q y + mu dn y^3                              (finish_mode multiplies by c2)
  //   grad_j += mu (c2 y^3 n_j - 3 dn y^5 r_j) - q c2 y^3 r_j
  // so the five factors in brackets are formed once and each density costs 8 FMAs.
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);   // C / r
    const R y2 = y * y;
    const R y3 = y2 * y;
    const R dn = dot3(d, rec + 3);
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));
    const R y3c = (rsqrt_scaled_c2(MODE) == 1.0) ? y3 : y3 * R(rsqrt_scaled_c2(MODE));
    const R g1 = dn * y3;
    const R a = (dn * y2) * K.c3 * y3;                      // 3 dn y^5
    R A[3], B[3];
#pragma unroll
    for (int j = 0; j < 3; j++) { A[j] = fma_(y3c, rec[3 + j], -a * d[j]); B[j] = y3c * d[j]; }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R q = rec[6 + 2 * m], mu = rec[7 + 2 * m];
      acc[m][0] = fma_(g1, mu, fma_(yc, q, acc[m][0]));
#pragma unroll
      for (int j = 0; j < 3; j++) acc[m][1 + j] = fma_(A[j], mu, fma_(-B[j], q, acc[m][1 + j]));
    }
  }
  template <class R, int MODE> static __device__ __forceinline__ void finish_mode(R (&acc)[K1]) { acc[0] *= R(rsqrt_scaled_c2(MODE)); }
  // transposed: two outputs from four weights (w_u, w_g).  With y = C / r, A = C^2 (d.w_g) / r^2 and dn = d.n
  //   g_q  += y (C^2 w_u - A)                                      C^3 x its value: finish_t_mode multiplies by C^2, as finish_mode does for the potential
  //   g_mu += y^3 (dn (C^2 w_u - 3 A) + C^2 (n.w_g))               C^5 x its value
  // record x_t, C^2 w_u, w_g (for d.w_g), C^2 w_g (for n.w_g)
  static constexpr int NREC_T = 10;
  template <class R, int MODE> static __device__ __forceinline__ void pack_t_mode(R* rec, const R* x, const R* w) {
    const R c2 = R(rsqrt_scaled_c2(MODE));
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = c2 * w[0];
    rec[4] = w[1]; rec[5] = w[2]; rec[6] = w[3]; rec[7] = c2 * w[1]; rec[8] = c2 * w[2]; rec[9] = c2 * w[3];
  }
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);   // C / r
    const R y2 = y * y;
    const R y3 = y2 * y;
    const R a = dot3(d, rec + 4) * y2;                      // C^2 (d.w_g) / r^2
    acc[0] = fma_(y, rec[3] - a, acc[0]);
    const R e = fma_(-a, K.c3, rec[3]);                     // C^2 (w_u - 3 (d.w_g) / r^2)
    const R h = fma_(n[2], rec[9], fma_(n[1], rec[8], fma_(n[0], rec[7], dot3(d, n) * e)));
    acc[1] = fma_(y3, h, acc[1]);
  }
  // transposed, several weights: the record keeps (w_u, w_g) per weight vector as they are.  With y = C / r, c2 = C^2 and dn = d.n, pair_t() accumulates
  //   g_q  += c2 y w_u - y^3 (d.w_g)                                   (finish_t_mode multiplies by c2)
  //   g_mu += (c2 dn y^3) w_u + sum_j (c2 y^3 n_j - 3 dn y^5 d_j) w_g[j]
  // so the eight factors are formed once (pair_m's A and B among them) and each weight vector costs 8 FMAs.
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R* rec, const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_scaled<MODE, MASKED>(len2(d), K.rsq);   // C / r
    const R y2 = y * y;
    const R y3 = y2 * y;
    const R dn = dot3(d, n);
    const R yc = (rsqrt_scaled_c2(MODE) == 1.0) ? y : y * R(rsqrt_scaled_c2(MODE));
    const R y3c = (rsqrt_scaled_c2(MODE) == 1.0) ? y3 : y3 * R(rsqrt_scaled_c2(MODE));
    const R g1 = dn * y3c;
    const R a = (dn * y2) * K.c3 * y3;                      // 3 dn y^5
    R A[3], B[3];
#pragma unroll
    for (int j = 0; j < 3; j++) { A[j] = fma_(y3c, n[j], -a * d[j]); B[j] = y3 * d[j]; }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R wu = rec[3 + 4 * m];
      const R* wg = rec + 4 + 4 * m;
      acc[m][0] = fma_(-B[2], wg[2], fma_(-B[1], wg[1], fma_(-B[0], wg[0], fma_(yc, wu, acc[m][0]))));
      acc[m][1] = fma_(A[2], wg[2], fma_(A[1], wg[1], fma_(A[0], wg[0], fma_(g1, wu, acc[m][1]))));
    }
  }
  // gradient: with q = f[0], mu = f[1], w_u = w[0], w_g = w[1..3], dn = d.n, B = d.w_g, nw = n.w_g the pair's scalar is
  //   phi = a1 y + P3 y^3 + P5 y^5,    a1 = w_u q,    P3 = mu (w_u dn + nw) - q B,    P5 = -3 mu dn B
  //   grad_d = -y^3 (a1 + y^2 (3 P3 + 5 P5 y^2)) d + y^3 (w_u mu n - q w_g) - 3 mu y^5 (B n + dn w_g)
  //   grad_n = mu y^3 (w_u d + w_g) - 3 mu B y^5 d
  template <class R, int MODE, bool MASKED, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[K0], const R (&w)[K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y3 = y2 * y;
    const R q = f[0], mu = f[1], wu = w[0];
    const R* wg = w + 1;
    const R dn = dot3(d, n), B = dot3(d, wg), nw = dot3(n, wg);
    const R h0 = -(y2 * K.c3);                               // -3 y^2: the y^5 terms inside the y^3 bracket
    const R h = mu * h0;
    const R P3 = fma_(mu, fma_(wu, dn, nw), -(q * B));
    const R P5 = (mu * K.c3) * (-dn * B);
    const R cd = -y3 * fma_(y2, fma_(P5 * R(5), y2, P3 * K.c3), wu * q);
    const R cn = fma_(h, B, wu * mu), cw = fma_(h, dn, -q);
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(cd, d[j], fma_(y3, fma_(cn, n[j], cw * wg[j]), G[j]));
    if constexpr (WANT_N) {
      const R mu3 = mu * y3, e = fma_(h0, B, wu);
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(mu3, fma_(e, d[j], wg[j]), N[j]);
    }
  }
  // tangent: with q = f[0], mu = f[1], dn = d.n, eps = d.e, t = e.n + d.m and h = 3 y^2 the potential u = q y + mu dn y^3 and the gradient
  // g = y^3 (mu n - q d) - mu dn h y^3 d move by
  //   du = y^3 (mu (t - dn eps h) - q eps)
  //   dg = y^3 (mu m - (q + mu h dn) e - mu eps h n + h (q eps - mu t + 5 mu dn eps y^2) d)
  template <class R, int MODE, bool MASKED> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&n)[ND ? 3 : 1], const R (&m)[ND ? 3 : 1], const R (&f)[K0], const KerCtx&, const Consts<R>& K) {
    R y2, y3;
    if constexpr (std::is_same<R, float>::value) {
      // fp32: this tangent rises to y^7 = y^3 (y^2)^2, and one close pair can hold half of a sum, so the rounding of a Newton-refined fp32 y (about one
      // ulp) arrived seven-fold in the result (measured, 1100 x 513 points: rel-L2 7.5e-7 where the same formula in torch float32 has 1.0e-7).  r^2 (d is
      // exact), the Newton step from the masked fp32 seed and the two powers are taken in fp64 (full rate on this device) and rounded once each: ten
      // fp64 instructions, modes 0 and 1 alike.  A masked seed of 0 stays 0; an unmasked inf gives NaN, which the tile's compare finds.
      const double r2 = __builtin_fma((double)d[2], (double)d[2], __builtin_fma((double)d[1], (double)d[1], (double)d[0] * (double)d[0]));
      double yd = (double)rsqrt_masked<0, MASKED>((float)r2, K.rsq);
      yd = __builtin_fma(yd * __builtin_fma(-(r2 * yd), yd, 1.0), 0.5, yd);
      const double y2d = yd * yd;
      y2 = (float)y2d;
      y3 = (float)(y2d * yd);
    } else {
      const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
      y2 = y * y;
      y3 = y2 * y;
    }
    const R q = f[0], mu = f[1];
    const R dn = dot3(d, n), eps = dot3(d, e), t = dot3(e, n) + dot3(d, m);
    const R h = y2 * K.c3;
    const R dne = dn * eps;
    acc[0] = fma_(y3, fma_(mu, fma_(-dne, h, t), -(q * eps)), acc[0]);
    const R ce = -fma_(mu * h, dn, q), cn = -((eps * h) * mu);
    const R cd = h * fma_(mu, fma_(dne * R(5), y2, -t), q * eps);
#pragma unroll
    for (int j = 0; j < 3; j++) acc[1 + j] = fma_(y3, fma_(mu, m[j], fma_(ce, e[j], fma_(cn, n[j], cd * d[j]))), acc[1 + j]);
  }
  // gradient, several rows: the 2 x 4 block C = sum_m (q, mu)_m (x) (w_u, w_g)_m (8 M instructions): c_q = C[0][0], c_m = C[1][0], the 3-vectors gq = C[0][1..3]
  // and gm = C[1][1..3].  With dn = d.n, Bq = d.gq, Bm = d.gm the sums of pair_g's terms are
  //   P3 = c_m dn + n.gm - Bq,    P5 = -3 dn Bm
  //   grad_d = -y^3 (c_q + y^2 (3 P3 + 5 P5 y^2)) d + y^3 ((c_m - 3 y^2 Bm) n - 3 y^2 dn gm - gq)
  //   grad_n = y^3 ((c_m - 3 y^2 Bm) d + gm)
  template <class R, int MODE, bool MASKED, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&N)[ND ? 3 : 1], const R (&d)[3], const R (&n)[ND ? 3 : 1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx&, const Consts<R>& K) {
    const R y = rsqrt_grad<MODE, MASKED>(len2(d), K.rsq);
    const R y2 = y * y;
    const R y3 = y2 * y;
    R C[2][4];
    contract_rows(C, f, w);
    const R* gq = C[0] + 1;
    const R* gm = C[1] + 1;
    const R dn = dot3(d, n), Bq = dot3(d, gq), Bm = dot3(d, gm), nw = dot3(n, gm);
    const R h0 = -(y2 * K.c3);                               // -3 y^2
    const R P3 = fma_(C[1][0], dn, nw) - Bq;
    const R P5 = K.c3 * (-dn * Bm);
    const R cd = -y3 * fma_(y2, fma_(P5 * R(5), y2, P3 * K.c3), C[0][0]);
    const R cn = fma_(h0, Bm, C[1][0]), cw = h0 * dn;
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(cd, d[j], fma_(y3, fma_(cn, n[j], fma_(cw, gm[j], -gq[j])), G[j]));
    if constexpr (WANT_N) {
#pragma unroll
      for (int j = 0; j < 3; j++) N[j] = fma_(y3, fma_(cn, d[j], gm[j]), N[j]);
    }
  }
  template <class R, int MODE> static __device__ __forceinline__ void finish_t_mode(R (&acc)[K0]) { acc[0] *= R(rsqrt_scaled_c2(MODE)); }
};

static_assert(helmholtz_dist_factor(2) == rsqrt_scaled_factor(2, 1) && helmholtz_dist_factor(0) == 1, "HelmholtzConsts' distance factor is the cubic step's A");
// ---- NEW: Helmholtz single layer G = exp(ikr)/r, complex k = ctx.v[0] + i ctx.v[1] (config 5)
//   (u_re, u_im) += G (f_re, f_im) as complex numbers, scale 1/(4 pi), G = 0 at r = 0.
struct Helmholtz3D_FxU {
  static constexpr int ID = 9, K0 = 2, K1 = 2, ND = 0, NREC = 6, FLOPS = 16;
  static constexpr const char* NAME = "Helmholtz3D-FxU";
  template <class R> using Consts = HelmholtzConsts<R>;
  static constexpr double scale() { return 1 / (4 * kPi); }
  static constexpr double acc_factor(int mode) { return rsqrt_scaled_factor(mode, 1); }   // the amplitude is the mode's C / r
  template <class R> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* f) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = f[0]; rec[4] = f[1]; rec[5] = 0;
  }
  // VARIANT (launch-uniform, Consts::variant): bit 0 = real wavenumber (no decay factor), bit 1 = the one-reduction form (fp64 all-pairs only)
  template <class R, int MODE, bool MASKED, int VARIANT = 0> static __device__ __forceinline__ void pair(R (&acc)[K1], const R (&d)[3], const R* rec, const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);   // C / r: the amplitude, its C in the scale
    const R rs = r2 * rinv;                                  // C r
    if constexpr ((VARIANT & 2) != 0) {
      R gr, gi;
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);        // reduces C r with the constants of k / C (HelmholtzConsts)
      acc[0] = fma_(gr, rec[3], fma_(-gi, rec[4], acc[0]));
      acc[1] = fma_(gi, rec[3], fma_(gr, rec[4], acc[1]));
      return;
    }
    const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);   // fp64: the table forms reduce C r with the constants of k / C; fp32 (hardware sine / cosine / exp2) takes r
    R sn, cs;
    sincos_<MASKED>(r, ctx, sn, cs, K);
    R amp = rinv;
    if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
    const R gr = amp * cs, gi = amp * sn;
    acc[0] = fma_(gr, rec[3], fma_(-gi, rec[4], acc[0]));
    acc[1] = fma_(gi, rec[3], fma_(gr, rec[4], acc[1]));
  }
  // multi: G = e^{ikr} / r as pair() forms it, once; 4 FMAs per density
  SCTL_AMD_MULTI_RECORD
  template <class R, int MODE, bool MASKED, int M, int VARIANT = 0> static __device__ __forceinline__ void pair_m(R (&acc)[M][K1], const R (&d)[3], const R* rec, const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R fr = rec[3 + 2 * m], fi = rec[4 + 2 * m];
      acc[m][0] = fma_(gr, fr, fma_(-gi, fi, acc[m][0]));
      acc[m][1] = fma_(gi, fr, fma_(gr, fi, acc[m][1]));
    }
  }
  // transposed: the same G = e^{ikr} / r from the same tables and variants; the 2 x 2 block [[gr, gi], [-gi, gr]] changes the sign of its off-diagonal:
  // g_re += gr w_re + gi w_im, g_im += gr w_im - gi w_re (the real 2 x 2 block transposed, i.e. conj(G) w as complex numbers: G itself is not conjugated,
  // only the roles of its imaginary part change).
  // record x_t, w_re, w_im
  static constexpr int NREC_T = 6;
  template <class R> static __device__ __forceinline__ void pack_t(R* rec, const R* x, const R* w) {
    rec[0] = x[0]; rec[1] = x[1]; rec[2] = x[2]; rec[3] = w[0]; rec[4] = w[1]; rec[5] = 0;
  }
  template <class R, int MODE, bool MASKED, int VARIANT = 0> static __device__ __forceinline__ void pair_t(R (&acc)[K0], const R (&d)[3], const R (&)[1], const R* rec, const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
    acc[0] = fma_(gr, rec[3], fma_(gi, rec[4], acc[0]));
    acc[1] = fma_(gr, rec[4], fma_(-gi, rec[3], acc[1]));
  }
  // transposed, several weights: G once, as pair_t() forms it; 4 FMAs per weight vector
  SCTL_AMD_MULTI_T_RECORD
  template <class R, int MODE, bool MASKED, int M, int VARIANT = 0> static __device__ __forceinline__ void pair_tm(R (&acc)[M][K0], const R (&d)[3], const R (&)[1], const R* rec, const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
      const R wr = rec[3 + 2 * m], wi = rec[4 + 2 * m];
      acc[m][0] = fma_(gr, wr, fma_(gi, wi, acc[m][0]));
      acc[m][1] = fma_(gr, wi, fma_(-gi, wr, acc[m][1]));
    }
  }
  // gradient: with c = conj(w) f and G = e^{ikr} / r the pair's scalar is phi = Re(c G), and dG/dr = (ik - 1/r) G, so
  //   grad_d = Re((ik - y) c G) y d,    Re((ik - y) H) = -(Im k + y) H_re - (Re k) H_im,    y = 1/r
  // G comes from the same tables and variants as pair(), i.e. as C G on the mode's unnormalised C / r: grad_factor carries the C, and y = (C / r) / C.
  static constexpr double grad_factor(int mode) { return rsqrt_scaled_factor(mode, 1); }
  template <class R, int MODE, bool MASKED, int VARIANT, bool WANT_N> static __device__ __forceinline__ void pair_g(R (&G)[3], R (&)[1], const R (&d)[3], const R (&)[1], const R (&f)[K0], const R (&w)[K1], const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
    const R y = rinv * R(K.cinv);
    const R cr = fma_(w[1], f[1], w[0] * f[0]), ci = fma_(-w[1], f[0], w[0] * f[1]);
    const R hr = fma_(-ci, gi, cr * gr), hi = fma_(ci, gr, cr * gi);
    const R a = REAL_K ? y : y + R(ctx.v[1]);
    const R t = -fma_(R(ctx.v[0]), hi, a * hr) * y;
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(t, d[j], G[j]);
  }
  // tangent: u = G f as complex numbers and dG/dr = (ik - 1/r) G, dr = (d.e) y: du = (ik - y) y (d.e) H with H = G f,
  //   Re((ik - y) H) = -(Im k + y) H_re - (Re k) H_im,    Im((ik - y) H) = (Re k) H_re - (Im k + y) H_im
  // G from the same tables and variants as pair() and pair_g, with the same grad_factor.
  template <class R, int MODE, bool MASKED, int VARIANT> static __device__ __forceinline__ void pair_j(R (&acc)[K1], const R (&d)[3], const R (&e)[3], const R (&)[1], const R (&)[1], const R (&f)[K0], const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
    const R y = rinv * R(K.cinv);
    const R hr = fma_(-gi, f[1], gr * f[0]), hi = fma_(gr, f[1], gi * f[0]);
    const R a = REAL_K ? y : y + R(ctx.v[1]);
    const R t = y * dot3(d, e);
    acc[0] = fma_(t, -fma_(R(ctx.v[0]), hi, a * hr), acc[0]);
    acc[1] = fma_(t, fma_(R(ctx.v[0]), hr, -(a * hi)), acc[1]);
  }
  // gradient, several rows: the complex c = sum_m conj(w_m) f_m (4 M instructions), then pair_g's form on it; G and grad_factor as there
  template <class R, int MODE, bool MASKED, int VARIANT, bool WANT_N, int M> static __device__ __forceinline__ void pair_gm(R (&G)[3], R (&)[1], const R (&d)[3], const R (&)[1], const R (&f)[M][K0], const R (&w)[M][K1], const KerCtx& ctx, const Consts<R>& K) {
    constexpr bool REAL_K = (VARIANT & 1) != 0;
    const R r2 = len2(d);
    const R rinv = rsqrt_scaled<MODE, MASKED>(r2, K.rsq);
    const R rs = r2 * rinv;
    R gr, gi;
    if constexpr ((VARIANT & 2) != 0) {
      cexp_<MASKED, REAL_K>(rs, rinv, ctx, gr, gi, K);
    } else {
      const R r = std::is_same<R, double>::value ? rs : rs * R(K.cinv);
      R sn, cs;
      sincos_<MASKED>(r, ctx, sn, cs, K);
      R amp = rinv;
      if (!REAL_K) amp *= exp_<MASKED>(r, ctx, K);
      gr = amp * cs; gi = amp * sn;
    }
    const R y = rinv * R(K.cinv);
    R cr = fma_(w[0][1], f[0][1], w[0][0] * f[0][0]), ci = fma_(-w[0][1], f[0][0], w[0][0] * f[0][1]);
#pragma unroll
    for (int m = 1; m < M; m++) {
      cr = fma_(w[m][1], f[m][1], fma_(w[m][0], f[m][0], cr));
      ci = fma_(-w[m][1], f[m][0], fma_(w[m][0], f[m][1], ci));
    }
    const R hr = fma_(-ci, gi, cr * gr), hi = fma_(ci, gr, cr * gi);
    const R a = REAL_K ? y : y + R(ctx.v[1]);
    const R t = -fma_(R(ctx.v[0]), hi, a * hr) * y;
#pragma unroll
    for (int j = 0; j < 3; j++) G[j] = fma_(t, d[j], G[j]);
  }
  // fp64, one reduction of r for the whole factor e^{ikr} (fastmath.hpp: cexp_tab_k); returns G = e^{ikr} / r.  The speculative pass runs it
  // unconditionally and records the largest distance; the careful pass branches per pair to libm beyond the table's range.
  // (r is C r and rinv C / r here, C = K.cdist)
  template <bool MASKED, bool REAL_K> static __device__ __forceinline__ void cexp_(double r, double rinv, const KerCtx& ctx, double& gr, double& gi, const HelmholtzConsts<double>& K) {
    if (MASKED && __builtin_expect(!(ctx.v[0] * r <= fastmath::kCexpMaxPhase * K.cdist), 0)) {
      double s, c;
      const double rt = r * K.cinv;
      ::sincos(ctx.v[0] * rt, &s, &c);
      const double amp = REAL_K ? rinv : rinv * ::exp(-ctx.v[1] * rt);
      gr = amp * c; gi = amp * s;
      return;
    }
    if (!MASKED) K.note_distance(r);
    double re, im;
    if (REAL_K) {
      fastmath::cexp_tab_k_real(r, re, im, K.ck, K.table);
      gr = rinv * re; gi = rinv * im;
    } else {
      double dm;
      fastmath::cexp_tab_k(r, re, im, dm, K.ck, K.table);
      const double amp = rinv * dm;
      gr = amp * re; gi = amp * im;
    }
  }
  template <bool MASKED, bool REAL_K> static __device__ __forceinline__ void cexp_(float, float, const KerCtx&, float&, float&, const HelmholtzConsts<float>&) {}   // fp32 has no such variant
  // fp64: Cody-Waite reduction to the nearest node of an LDS table + a short polynomial (fastmath.hpp).  The speculative pass
  // (MASKED = false) runs the forms with the wavenumber folded in, unconditionally, as straight-line code, and only records the
  // largest distance (one v_max_f64) for the end-of-tile check; a tile with |Re k| r > 1.2e4 (two thousand wavelengths) or
  // |Im k| r > 700 is re-run by the careful pass, which branches per pair (libm beyond the table's range).
  template <bool MASKED> static __device__ __forceinline__ void sincos_(double r, const KerCtx& ctx, double& s, double& c, const HelmholtzConsts<double>& K) {
    if (!MASKED) {
      K.note_distance(r);
      fastmath::sincos_tab_k(r, s, c, K.tk, K.table);
      return;
    }
    const double x = ctx.v[0] * r;                       // (r is C r here: HelmholtzConsts)
    if (__builtin_expect(__builtin_fabs(x) > fastmath::kSincosTabMaxArg * K.cdist, 0)) ::sincos(x * K.cinv, &s, &c);
    else fastmath::sincos_tab_k(r, s, c, K.tk, K.table);
  }
  // fp32: the hardware's sine / cosine / exp2 (v_sin_f32, v_cos_f32, v_exp_f32: ~1e-6 absolute, inputs in revolutions / powers of
  // two) behind a two-piece reduction, so that the reduced argument keeps 24 bits however many periods x spans.  The phase
  // error that remains is the rounding of x itself (|x| 6e-8), which libm's exact reduction cannot remove either.
  template <bool MASKED> static __device__ __forceinline__ void sincos_(float r, const KerCtx& ctx, float& s, float& c, const HelmholtzConsts<float>&) {
    const float x = float(ctx.v[0]) * r;
    const float c_hi = 0.15915494f, c_lo = 6.4206383e-9f;       // 1/(2 pi) = c_hi + c_lo
    const float n = __builtin_rintf(x * c_hi);
    float fr = __builtin_fmaf(x, c_hi, -n);
    fr = __builtin_fmaf(x, c_lo, fr);
    s = __builtin_amdgcn_sinf(fr);
    c = __builtin_amdgcn_cosf(fr);
  }
  // exp(-Im k r): r >= 0 is clamped to 800/|Im k| (one v_min_f64; a NaN distance turns into the cap, but then rinv is NaN
  // too and the product stays NaN), so the argument handed to the table code is within its +-800 range
  template <bool MASKED> static __device__ __forceinline__ double exp_(double r, const KerCtx& ctx, const HelmholtzConsts<double>& K) {
    if (!MASKED) return fastmath::exp_tab_k(r, K.tk, K.table);   // range checked at the end of the tile (tile_bad)
    // careful pass: r >= 0 clamped to kExpTabMaxArg / |Im k| — the value there is 0 or inf already (a NaN distance turns into the cap, but
    // then rinv is NaN too and the product stays NaN)
    return fastmath::exp_tab_k(__builtin_fmin(r, fastmath::kExpTabMaxArg * K.cdist / __builtin_fabs(ctx.v[1])), K.tk, K.table);
  }
  template <bool MASKED> static __device__ __forceinline__ float exp_(float r, const KerCtx& ctx, const HelmholtzConsts<float>&) {
    const float x = -float(ctx.v[1]) * r;
    const float l_hi = 1.4426950f, l_lo = 1.9259630e-8f;        // log2(e) = l_hi + l_lo
    const float n = __builtin_fminf(__builtin_fmaxf(__builtin_rintf(x * l_hi), -300.0f), 300.0f);
    float fr = __builtin_fmaf(x, l_hi, -n);
    fr = __builtin_fmaf(x, l_lo, fr);
    return __builtin_ldexpf(__builtin_amdgcn_exp2f(fr), (int)n);   // |x| beyond the clamp: fr is huge, exp2 gives 0 / inf as it should
  }
};

}  // namespace sctl_amd
