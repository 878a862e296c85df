// The direction of a several-row kernel sum, as the policy `Dir` of the one-body kernels (rows_kernel.hpp: all pairs; lists_rows_kernel.hpp: the P2P lists):
//   forward     v[m][t,k1] += scale * sum_s sum_k0 U(x_t - x_s, n_s)[k0][k1] * f[m][s,k0]     the OWNERS of the sums are the targets, the sources are STREAMED
//   transposed  g[m][s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t,k1]     the owners are the sources, the targets are streamed
// A policy holds what follows from the direction alone: which of K0 / K1 is the width of an output and of an input row, who carries the normal, the streamed
// record of M rows and its pack hook (ukernels.hpp: NREC_M / pack_m, NREC_TM / pack_tm), the pair (the sign of d and pair_m / pair_tm) and the finish hook.  How a
// kernel finds its points — the fields of its arguments — is not here.
#pragma once
#include <sctl_amd/device/eval_transpose_kernel.hpp>

namespace sctl_amd {

// Forward: sources are streamed with their normal and M densities of K0 reals; a target gathers M x K1 sums and holds no normal (the pair takes a dummy).
struct RowsFwd {
  template <class Ker> static constexpr int KOUT = Ker::K1;      // reals of an output row per owner
  template <class Ker> static constexpr int KIN = Ker::K0;       // reals of an input row per streamed point
  template <class Ker> static constexpr int OWN_N = 0;           // reals of the normal an owner holds
  template <class Ker> static constexpr int STR_N = Ker::ND;     // reals of the normal a streamed point brings
  template <class Ker, int M> static constexpr int NREC = Ker::template NREC_M<M>;
  template <class Ker, class R, int M> static __device__ __forceinline__ void pack(R* rec, const R* x, const R* n, const R (&f)[M][Ker::K0]) {
    Ker::template pack_m<R, M>(rec, x, n, f);
  }
  template <class Ker, class R, int MODE, bool MASKED, int M, int VARIANT, class KC>
  static __device__ __forceinline__ void pair(R (&tacc)[M][Ker::K1], const R (&xt)[3], const R (&)[1], const R* rec, const KerCtx& ctx, const KC& K) {
    const R d[3] = {xt[0] - rec[0], xt[1] - rec[1], xt[2] - rec[2]};
    if constexpr (KC::HAS_VARIANT) Ker::template pair_m<R, MODE, MASKED, M, VARIANT>(tacc, d, rec, ctx, K);
    else Ker::template pair_m<R, MODE, MASKED, M>(tacc, d, rec, ctx, K);
  }
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void finish(R (&acc)[Ker::K1]) { finish_acc<Ker, R, MODE>(acc); }
};

// Transposed: targets are streamed with M weight vectors of K1 reals; a source, with its normal, gathers M x K0 sums.
struct RowsTrans {
  template <class Ker> static constexpr int KOUT = Ker::K0;
  template <class Ker> static constexpr int KIN = Ker::K1;
  template <class Ker> static constexpr int OWN_N = Ker::ND ? 3 : 0;
  template <class Ker> static constexpr int STR_N = 0;
  template <class Ker, int M> static constexpr int NREC = Ker::template NREC_TM<M>;
  template <class Ker, class R, int M> static __device__ __forceinline__ void pack(R* rec, const R* x, const R*, const R (&w)[M][Ker::K1]) {
    Ker::template pack_tm<R, M>(rec, x, w);
  }
  template <class Ker, class R, int MODE, bool MASKED, int M, int VARIANT, class KC>
  static __device__ __forceinline__ void pair(R (&tacc)[M][Ker::K0], const R (&xs)[3], const R (&xn)[Ker::ND ? 3 : 1], const R* rec, const KerCtx& ctx, const KC& K) {
    const R d[3] = {rec[0] - xs[0], rec[1] - xs[1], rec[2] - xs[2]};
    if constexpr (KC::HAS_VARIANT) Ker::template pair_tm<R, MODE, MASKED, M, VARIANT>(tacc, d, xn, rec, ctx, K);
    else Ker::template pair_tm<R, MODE, MASKED, M>(tacc, d, xn, rec, ctx, K);
  }
  template <class Ker, class R, int MODE> static __device__ __forceinline__ void finish(R (&acc)[Ker::K0]) { finish_t_acc<Ker, R, MODE>(acc); }
};

}  // namespace sctl_amd
