// Transposed list forms of Laplace3D_FxU for several weight vectors (lists_multi_transpose_kernel, lists_rows_kernel.hpp): widest form 8 weight vectors in fp64, 8 in fp32.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiTEntry& ltmulti_Laplace3D_FxU() {
  static const ListsMultiTEntry e = make_lists_rows_entry<ListTrans, Laplace3D_FxU, 8, 8>();
  return e;
}
}  // namespace sctl_amd
