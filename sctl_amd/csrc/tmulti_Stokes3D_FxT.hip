// Transposed forms of Stokes3D_FxT for several weight vectors (multi_transpose_kernel.hpp): sources per lane 2 / 1 for 2 / 4 weight vectors; no form of 8 (its fp64 forms need 274 vector registers: one wave per SIMD).
#include "multi_transpose_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Stokes3D_FxT() {
  static const MultiTEntry e = make_multi_t_entry<Stokes3D_FxT, 2, 1, 0>();
  return e;
}
}  // namespace sctl_amd
