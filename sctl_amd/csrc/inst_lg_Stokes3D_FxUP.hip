// Launch table of the list gradient kernels of Stokes3D_FxUP, both sides (see include/sctl_amd/device/lists_grad_kernel.hpp).
#include <sctl_amd/device/lists_grad_kernel.hpp>
namespace sctl_amd {
const ListsGradEntry& lists_grad_Stokes3D_FxUP() {
  static const ListsGradEntry e = make_lists_grad_entry<Stokes3D_FxUP>();
  return e;
}
}  // namespace sctl_amd
