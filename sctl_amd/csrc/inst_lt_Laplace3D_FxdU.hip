// Instantiations of the transposed list kernels for Laplace3D_FxdU (see launch.hpp, lists_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_LISTS_T_INSTANCES(, Laplace3D_FxdU)
}  // namespace sctl_amd
