// Multi-density forms of Laplace3D_FxdU (multi_kernel.hpp): targets per lane 2 / 1 / 1 for 2 / 4 / 8 densities.
#include "multi_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Laplace3D_FxdU() {
  static const MultiEntry e = make_multi_entry<Laplace3D_FxdU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
