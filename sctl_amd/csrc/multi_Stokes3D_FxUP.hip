// Multi-density forms of Stokes3D_FxUP (rows_kernel.hpp, forward): targets per lane 2 / 1 for 2 / 4 densities.
#include "rows_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Stokes3D_FxUP() {
  static const MultiEntry e = make_rows_entry<RowsFwd, Stokes3D_FxUP, 2, 1, 0>();
  return e;
}
}  // namespace sctl_amd
