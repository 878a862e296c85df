// Transposed list forms of Stokes3D_DxU for several weight vectors (lists_multi_transpose_kernel, lists_rows_kernel.hpp): widest form 4 weight vectors in fp64, 8 in fp32.
// No fp64 form of 8: at 256 vector registers (two waves per SIMD) it spills 12 bytes of scratch in every mode.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiTEntry& ltmulti_Stokes3D_DxU() {
  static const ListsMultiTEntry e = make_lists_rows_entry<ListTrans, Stokes3D_DxU, 4, 8>();
  return e;
}
}  // namespace sctl_amd
