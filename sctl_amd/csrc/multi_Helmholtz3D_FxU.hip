// Multi-density forms of Helmholtz3D_FxU (rows_kernel.hpp, forward): targets per lane 2 / 1 / 1 for 2 / 4 / 8 densities.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Helmholtz3D_FxU() {
  static const MultiEntry e = make_rows_entry<RowsFwd, Helmholtz3D_FxU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
