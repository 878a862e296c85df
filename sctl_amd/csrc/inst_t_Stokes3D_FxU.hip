// Instantiations of the transposed evaluation kernels for Stokes3D_FxU (see launch.hpp, eval_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_T_INSTANCES(, Stokes3D_FxU)
}  // namespace sctl_amd
