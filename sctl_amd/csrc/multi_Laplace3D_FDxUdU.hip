// Multi-density forms of Laplace3D_FDxUdU (multi_kernel.hpp): targets per lane 2 / 1 for 2 / 4 densities.
#include "multi_kernel.hpp"
namespace sctl_amd {
const MultiEntry& multi_Laplace3D_FDxUdU() {
  static const MultiEntry e = make_multi_entry<Laplace3D_FDxUdU, 2, 1, 0>();
  return e;
}
}  // namespace sctl_amd
