// Transposed forms of Laplace3D_FxdU for several weight vectors (rows_kernel.hpp, transposed): sources per lane 2 / 1 / 1 for 2 / 4 / 8 weight vectors.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Laplace3D_FxdU() {
  static const MultiTEntry e = make_rows_entry<RowsTrans, Laplace3D_FxdU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
