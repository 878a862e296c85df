// Transposed forms of Stokes3D_FxU for several weight vectors (rows_kernel.hpp, transposed): sources per lane 2 / 1 / 1 for 2 / 4 / 8 weight vectors.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Stokes3D_FxU() {
  static const MultiTEntry e = make_rows_entry<RowsTrans, Stokes3D_FxU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
