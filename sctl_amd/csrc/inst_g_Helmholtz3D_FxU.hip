// Instantiations of the gradient evaluation kernels for Helmholtz3D_FxU (see launch.hpp, eval_grad_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_G_INSTANCES(, Helmholtz3D_FxU)
}  // namespace sctl_amd
