// Transposed list forms of Stokes3D_FxT for several weight vectors (lists_multi_transpose_kernel, lists_rows_kernel.hpp): widest form 4 weight vectors in fp64, 4 in fp32.
// No fp64 form of 8: its record of 52 doubles makes a 64-record tile of 26.7 KB, more than the 20 KB that leave two waves per SIMD.
// No fp32 form of 8: it compiles (228 vector registers, 13.1 KB of LDS, no scratch; owners in halves, one target per lane and step), but at leaves of ~8
// points it took 1.053 x the time of eight single calls (0.558 and 0.576 x at ~64 and ~512: profiles/r14_lists_transpose_densities.txt), so by the
// shipping rule of DESIGN.md §4.15 it is left out and eight rows run as two passes of 4.
#include "lists_rows_kernel.hpp"
namespace sctl_amd {
const ListsMultiTEntry& ltmulti_Stokes3D_FxT() {
  static const ListsMultiTEntry e = make_lists_rows_entry<ListTrans, Stokes3D_FxT, 4, 4>();
  return e;
}
}  // namespace sctl_amd
