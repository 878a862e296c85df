// Tangent (directional-derivative) evaluation kernels of Stokes3D_FxUP (jvp_kernel.hpp): fp64 modes 0-2, fp32 modes 0-1.
#include "jvp_kernel.hpp"
namespace sctl_amd {
const JvpEntry& jvp_Stokes3D_FxUP() {
  static const JvpEntry e = make_jvp_entry<Stokes3D_FxUP>();
  return e;
}
}  // namespace sctl_amd
