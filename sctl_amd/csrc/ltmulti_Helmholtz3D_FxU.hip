// Transposed list forms of Helmholtz3D_FxU for several weight vectors (lists_multi_transpose_kernel, lists_rows_kernel.hpp): widest form 4 weight vectors in fp64, 8 in fp32.
// No fp64 form of 8: with the kernel's LDS tables its 64-record tile does not fit the 20 KB that leave two waves per SIMD.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiTEntry& ltmulti_Helmholtz3D_FxU() {
  static const ListsMultiTEntry e = make_lists_rows_entry<ListTrans, Helmholtz3D_FxU, 4, 8>();
  return e;
}
}  // namespace sctl_amd
