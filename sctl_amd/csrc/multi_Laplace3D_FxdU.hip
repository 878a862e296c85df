// Multi-density forms of Laplace3D_FxdU (rows_kernel.hpp, forward): targets per lane 2 / 1 / 1 for 2 / 4 / 8 densities.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Laplace3D_FxdU() {
  static const MultiEntry e = make_rows_entry<RowsFwd, Laplace3D_FxdU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
