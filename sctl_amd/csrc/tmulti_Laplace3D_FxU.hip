// Transposed forms of Laplace3D_FxU for several weight vectors (multi_transpose_kernel.hpp): sources per lane 2 / 2 / 2 for 2 / 4 / 8 weight vectors.
#include "multi_transpose_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Laplace3D_FxU() {
  static const MultiTEntry e = make_multi_t_entry<Laplace3D_FxU, 2, 2, 2>();
  return e;
}
}  // namespace sctl_amd
