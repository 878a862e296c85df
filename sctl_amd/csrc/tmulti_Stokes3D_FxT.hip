// Transposed forms of Stokes3D_FxT for several weight vectors (rows_kernel.hpp, transposed): sources per lane 2 / 1 for 2 / 4 weight vectors; no form of 8 (its fp64 forms need 274 vector registers: one wave per SIMD).
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Stokes3D_FxT() {
  static const MultiTEntry e = make_rows_entry<RowsTrans, Stokes3D_FxT, 2, 1, 0>();
  return e;
}
}  // namespace sctl_amd
