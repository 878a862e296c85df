// Tangent (directional-derivative) evaluation kernels of Laplace3D_DxU (jvp_kernel.hpp): fp64 modes 0-2, fp32 modes 0-1.
#include "jvp_kernel.hpp"
namespace sctl_amd {
const JvpEntry& jvp_Laplace3D_DxU() {
  static const JvpEntry e = make_jvp_entry<Laplace3D_DxU>();
  return e;
}
}  // namespace sctl_amd
