// Several-densities list forms of Stokes3D_FxU (lists_multi_kernel, lists_rows_kernel.hpp): widest form 4 densities in fp64, 8 in fp32.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiEntry& lmulti_Stokes3D_FxU() {
  static const ListsMultiEntry e = make_lists_rows_entry<ListFwd, Stokes3D_FxU, 4, 8>();
  return e;
}
}  // namespace sctl_amd
