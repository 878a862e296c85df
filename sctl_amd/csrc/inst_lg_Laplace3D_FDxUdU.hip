// Launch table of the list gradient kernels of Laplace3D_FDxUdU, both sides (see include/sctl_amd/device/lists_grad_kernel.hpp).
#include <sctl_amd/device/lists_grad_kernel.hpp>
namespace sctl_amd {
const ListsGradEntry& lists_grad_Laplace3D_FDxUdU() {
  static const ListsGradEntry e = make_lists_grad_entry<Laplace3D_FDxUdU>();
  return e;
}
}  // namespace sctl_amd
