// The direction of a kernel sum, as the policy `Dir` of the P2P list walkers (lists_kernel.hpp: lists_item, lists_packed_item) and the base of the several-row policies:
//   forward     v[t,k1] += scale * sum_s sum_k0 U(x_t - x_s, n_s)[k0][k1] * f[s,k0]     the OWNERS of the sums are the targets, the sources are STREAMED
//   transposed  g[s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[t,k1]     the owners are the sources, the targets are streamed
// A policy holds what follows from the direction alone: which of K0 / K1 is the width of the output and of the input, who carries the normal, the streamed
// record and its pack hook (ukernels.hpp: NREC / pack, NREC_T / pack_t), the pair (the sign of d, pair / pair_t), the finish hook, and which field of an
// argument struct belongs to the owners and which to the streamed points.  The argument structs of a direction name their fields alike (EvalArgs / ListArgs: xt,
// xs, xn, f, v_trg; EvalTArgs / ListTArgs: xt, xs, xn, w, g_src), so the accessors are templates over the struct.  (The single-row all-pairs kernels keep a body
// each, eval_kernel.hpp and eval_transpose_kernel.hpp: DESIGN.md §4.11.)
// Every member is a template over the functor: DirTrans is instantiated only for a functor that has pair_t (HasPairT), a functor without it never meets it.
// The several-row policies (RowsFwd / RowsTrans, ListFwd / ListTrans) derive from these and replace only the record, pack and pair by their M-row forms.
#pragma once
#include "ukernels.hpp"

namespace sctl_amd {

// Forward: sources are streamed with their normal and a density of K0 reals; a target gathers K1 sums and holds no normal (the pair takes a dummy).
struct DirFwd {
  template <class Ker> static constexpr int KOUT = Ker::K1;      // reals of the output per owner
  template <class Ker> static constexpr int KIN = Ker::K0;       // reals of the input per streamed point
  template <class Ker> static constexpr int OWN_N = 0;           // reals of the normal an owner holds
  template <class Ker> static constexpr int STR_N = Ker::ND;     // reals of the normal a streamed point brings
  template <class Ker> static constexpr int NREC = Ker::NREC;    // reals of a streamed record
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R* f) {
    pack_record<Ker, R, MODE>(rec, x, n, f);
  }
  template <class Ker, class R, int MODE, bool MASKED, int VARIANT, class KC>
  static __device__ __forceinline__ void pair(R (&tacc)[Ker::K1], const R (&xt)[3], const R (&)[1], const R* rec, const KerCtx& ctx, const KC& K) {
    const R d[3] = {xt[0] - rec[0], xt[1] - rec[1], xt[2] - rec[2]};
    if constexpr (KC::HAS_VARIANT) Ker::template pair<R, MODE, MASKED, VARIANT>(tacc, d, rec, ctx, K);
    else Ker::template pair<R, MODE, MASKED>(tacc, d, rec, ctx, K);
  }
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void finish(R (&acc)[Ker::K1]) { finish_acc<Ker, R, MODE>(acc); }
  // A: ListArgs (or EvalArgs)
  template <class R, template <class> class A> static __device__ __forceinline__ const R* own_x(const A<R>& a) { return a.xt; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* own_n(const A<R>&) { return nullptr; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* str_x(const A<R>& a) { return a.xs; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* str_n(const A<R>& a) { return a.xn; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* in(const A<R>& a) { return a.f; }
  template <class R, template <class> class A> static __device__ __forceinline__ R* out(const A<R>& a) { return a.v_trg; }
};

// Transposed: targets are streamed with a weight vector of K1 reals; a source, with its normal, gathers K0 sums.  d = x_trg - x_src keeps the forward sign.
struct DirTrans {
  template <class Ker> static constexpr int KOUT = Ker::K0;
  template <class Ker> static constexpr int KIN = Ker::K1;
  template <class Ker> static constexpr int OWN_N = Ker::ND ? 3 : 0;
  template <class Ker> static constexpr int STR_N = 0;
  template <class Ker> static constexpr int NREC = Ker::NREC_T;
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R* w) {
    pack_t_record<Ker, R, MODE>(rec, x, w);
  }
  template <class Ker, class R, int MODE, bool MASKED, int VARIANT, class KC>
  static __device__ __forceinline__ void pair(R (&tacc)[Ker::K0], const R (&xs)[3], const R (&xn)[Ker::ND ? 3 : 1], const R* rec, const KerCtx& ctx, const KC& K) {
    const R d[3] = {rec[0] - xs[0], rec[1] - xs[1], rec[2] - xs[2]};
    if constexpr (KC::HAS_VARIANT) Ker::template pair_t<R, MODE, MASKED, VARIANT>(tacc, d, xn, rec, ctx, K);
    else Ker::template pair_t<R, MODE, MASKED>(tacc, d, xn, rec, ctx, K);
  }
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void finish(R (&acc)[Ker::K0]) { finish_t_acc<Ker, R, MODE>(acc); }
  // A: ListTArgs (or EvalTArgs)
  template <class R, template <class> class A> static __device__ __forceinline__ const R* own_x(const A<R>& a) { return a.xs; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* own_n(const A<R>& a) { return a.xn; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* str_x(const A<R>& a) { return a.xt; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* str_n(const A<R>&) { return nullptr; }
  template <class R, template <class> class A> static __device__ __forceinline__ const R* in(const A<R>& a) { return a.w; }
  template <class R, template <class> class A> static __device__ __forceinline__ R* out(const A<R>& a) { return a.g_src; }
};

}  // namespace sctl_amd
