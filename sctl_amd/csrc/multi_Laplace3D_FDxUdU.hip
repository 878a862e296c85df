// Multi-density forms of Laplace3D_FDxUdU (rows_kernel.hpp, forward): targets per lane 2 / 1 for 2 / 4 densities.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Laplace3D_FDxUdU() {
  static const MultiEntry e = make_rows_entry<RowsFwd, Laplace3D_FDxUdU, 2, 1, 0>();
  return e;
}
}  // namespace sctl_amd
