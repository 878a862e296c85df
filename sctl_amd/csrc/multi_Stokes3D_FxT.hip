// Multi-density forms of Stokes3D_FxT (multi_kernel.hpp): targets per lane 1 / 1 for 2 / 4 densities.
#include "multi_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Stokes3D_FxT() {
  static const MultiEntry e = make_multi_entry<Stokes3D_FxT, 1, 1, 0>();
  return e;
}
}  // namespace sctl_amd
