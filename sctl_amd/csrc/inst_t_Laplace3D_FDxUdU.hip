// Instantiations of the transposed evaluation kernels for Laplace3D_FDxUdU (see launch.hpp, eval_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_EVAL_T_INSTANCES(, Laplace3D_FDxUdU)
}  // namespace sctl_amd
