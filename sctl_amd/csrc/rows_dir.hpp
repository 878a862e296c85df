// The direction of a several-row kernel sum, as the policy `Dir` of the one-body kernels (rows_kernel.hpp: all pairs; lists_rows_kernel.hpp: the P2P lists):
//   forward     v[m][t,k1] += scale * sum_s sum_k0 U(x_t - x_s, n_s)[k0][k1] * f[m][s,k0]     the OWNERS of the sums are the targets, the sources are STREAMED
//   transposed  g[m][s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] * w[m][t,k1]     the owners are the sources, the targets are streamed
// What follows from the direction alone and not from the number of rows — which of K0 / K1 is the width of an output and of an input row, who carries the
// normal, the finish hook, the fields of ListArgs / ListTArgs — is inherited from the single-row policies DirFwd / DirTrans (device/dir.hpp).  Replaced here:
// the streamed record of M rows, its pack hook (ukernels.hpp: NREC_M / pack_m, NREC_TM / pack_tm) and the pair (the sign of d and pair_m / pair_tm).
#pragma once
#include <sctl_amd/device/dir.hpp>
#include <sctl_amd/device/eval_transpose_kernel.hpp>

namespace sctl_amd {

// Forward: sources are streamed with their normal and M densities of K0 reals; a target gathers M x K1 sums and holds no normal (the pair takes a dummy).
struct RowsFwd : DirFwd {
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
};

// Transposed: targets are streamed with M weight vectors of K1 reals; a source, with its normal, gathers M x K0 sums.
struct RowsTrans : DirTrans {
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
};

}  // namespace sctl_amd
