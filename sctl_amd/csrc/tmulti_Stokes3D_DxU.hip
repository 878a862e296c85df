// Transposed forms of Stokes3D_DxU for several weight vectors (multi_transpose_kernel.hpp): sources per lane 2 / 1 / 1 for 2 / 4 / 8 weight vectors.
#include "multi_transpose_kernel.hpp"
namespace sctl_amd {
const MultiTEntry& multi_t_Stokes3D_DxU() {
  static const MultiTEntry e = make_multi_t_entry<Stokes3D_DxU, 2, 1, 1>();
  return e;
}
}  // namespace sctl_amd
