// Gradient forms of Laplace3D_DxU for several density / weight rows (multi_grad_kernel.hpp): forms of 2 .. 8 rows, both sides.
#include "multi_grad_kernel.hpp"
namespace sctl_amd {
const MultiGEntry& multi_g_Laplace3D_DxU() {
  static const MultiGEntry e = make_multi_g_entry<Laplace3D_DxU, 8>();
  return e;
}
}  // namespace sctl_amd
