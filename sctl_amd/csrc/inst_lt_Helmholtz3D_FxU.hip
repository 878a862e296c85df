// Instantiations of the transposed list kernels for Helmholtz3D_FxU (see launch.hpp, lists_transpose_kernel.hpp).
#include <sctl_amd/device/launch.hpp>
namespace sctl_amd {
SCTL_AMD_LISTS_T_INSTANCES(, Helmholtz3D_FxU)
}  // namespace sctl_amd
