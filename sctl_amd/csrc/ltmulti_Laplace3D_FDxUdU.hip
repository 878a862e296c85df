// Transposed list forms of Laplace3D_FDxUdU for several weight vectors (lists_multi_transpose_kernel, lists_rows_kernel.hpp): widest form 4 weight vectors in fp64, 8 in fp32.
// No fp64 form of 8: at 256 vector registers (two waves per SIMD) it spills 28 - 44 bytes of scratch.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiTEntry& ltmulti_Laplace3D_FDxUdU() {
  static const ListsMultiTEntry e = make_lists_rows_entry<ListTrans, Laplace3D_FDxUdU, 4, 8>();
  return e;
}
}  // namespace sctl_amd
