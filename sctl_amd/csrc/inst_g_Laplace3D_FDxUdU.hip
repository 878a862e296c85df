// Instantiations of the gradient evaluation kernels for Laplace3D_FDxUdU (see launch.hpp, eval_grad_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_G_INSTANCES(, Laplace3D_FDxUdU)
}  // namespace sctl_amd
