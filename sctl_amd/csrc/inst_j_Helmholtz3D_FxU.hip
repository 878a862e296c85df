// Tangent (directional-derivative) evaluation kernels of Helmholtz3D_FxU (jvp_kernel.hpp): fp64 modes 0-2, fp32 modes 0-1.
#include "jvp_kernel.hpp"
namespace sctl_amd {
const JvpEntry& jvp_Helmholtz3D_FxU() {
  static const JvpEntry e = make_jvp_entry<Helmholtz3D_FxU>();
  return e;
}
}  // namespace sctl_amd
