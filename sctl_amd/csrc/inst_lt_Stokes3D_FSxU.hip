// Instantiations of the transposed list kernels for Stokes3D_FSxU (see launch.hpp, lists_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_LISTS_T_INSTANCES(, Stokes3D_FSxU)
}  // namespace sctl_amd
