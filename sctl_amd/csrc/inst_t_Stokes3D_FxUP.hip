// Instantiations of the transposed evaluation kernels for Stokes3D_FxUP (see launch.hpp, eval_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_T_INSTANCES(, Stokes3D_FxUP)
}  // namespace sctl_amd
