// Multi-density forms of Laplace3D_DxU (rows_kernel.hpp, forward): targets per lane 2 / 2 / 2 for 2 / 4 / 8 densities.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Laplace3D_DxU() {
  static const MultiEntry e = make_rows_entry<RowsFwd, Laplace3D_DxU, 2, 2, 2>();
  return e;
}
}  // namespace sctl_amd
