// Instantiations of the gradient evaluation kernels for Stokes3D_FSxU (see launch.hpp, eval_grad_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_G_INSTANCES(, Stokes3D_FSxU)
}  // namespace sctl_amd
