// The launch planners and drivers of the all-pairs evaluators (eval_drivers.hip).  A driver takes `real` and untyped device pointers and enqueues on a
// stream; the typed templates behind it are private to eval_drivers.hip.
#pragma once
#include "internal.hpp"
#include "rows_kernel.hpp"
#include "multi_grad_kernel.hpp"
#include "jvp_kernel.hpp"

namespace sctl_amd {
// centered.hip
template <class R>
hipError_t eval_centered(int kernel_id, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, R* v_trg, double scale, int mode,
                         int cus, hipStream_t st, bool presorted, int64_t density);
void centered_plan(int64_t Nt, int64_t Ns, int cus, int src_bytes, int out_bytes, int* T, int* splits, int64_t* chunk);
int centered_pipe(int kernel_id, int real, int mode);
int centered_targets_per_wave(int kernel_id, int real, int mode, int64_t density);
hipError_t morton_order_device(int real, const void* d_x, int64_t n, void* d_sorted, uint32_t* d_perm, hipStream_t st);
}  // namespace sctl_amd

#pragma GCC visibility push(hidden)
namespace sctl_amd {

int cu_count();   // CUs of the current device; 256 (MI355X) when planning without a device

struct Plan {
  int t_idx;        // index into kTvalues
  int splits;
  int64_t chunk;    // sources per split (multiple of kTile)
  int64_t wg_x;
  int64_t workspace_bytes;
};
Plan make_plan(const KernelEntry& k, int real, int64_t Nt, int64_t Ns);

// The transposed evaluation (eval_transpose_kernel.hpp): make_plan with the roles exchanged — the SOURCES own the output and tile grid.x, the TARGET
// range is split.  The partial sums [splits][owners * K0] are bounded at 2 GB by cutting the owners into several launches of owners_per_launch
// (a multiple of a workgroup's 256 * T owners), never by taking fewer splits: the splits are what keeps a streamed chunk in one XCD's L2.
struct PlanT {
  int t_idx;        // index into kTTvalues
  int splits;
  int64_t chunk;    // targets per split (multiple of kTile)
  int64_t owners_per_launch;
  int64_t workspace_bytes;
};
PlanT make_plan_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns);
// The geometry shared by the owner schemes that stream the other set (the transposed and the gradient evaluators): `owners` points own `out_width` sums
// each, t per lane; the `streamed` points, `streamed_reals` reals each, are split.
struct PlanOwned {
  int splits;
  int64_t chunk, owners_per_launch, workspace_bytes;
};
PlanOwned plan_owned(int64_t owners, int64_t streamed, int t, int64_t streamed_reals, int64_t out_width, int64_t rs);
PlanOwned make_plan_g(const KernelEntry& k, int real, int side, int64_t Nt, int64_t Ns);

// ---- several rows through the all-pairs sum: densities forward (Dir = RowsFwd), weight vectors transposed (RowsTrans); rows_kernel.hpp ----
template <class Dir> const RowsEntry<Dir>* multi_entry(int kernel_id);   // null for a registered plugin kernel: its rows go one at a time through the single-row path
template <> const MultiEntry* multi_entry<RowsFwd>(int kernel_id);
template <> const MultiTEntry* multi_entry<RowsTrans>(int kernel_id);
// the form for `left` rows still to do: the narrowest of 2 / 4 / 8 that takes them all, else the widest
template <class Dir> int multi_form(const RowsEntry<Dir>& me, int left) {
  for (int i = 0; i < kNumRowsM; i++)
    if (me.t[i] && (kRowsM[i] >= left || kRowsM[i] == me.m_max)) return i;
  return 0;
}
// make_plan with M rows in a streamed record, in terms of owners (the targets forward, the sources transposed) and streamed points: the same workgroup target, the
// L2 rule counting all `streamed_reals` of a record in a split's streamed bytes, and the splits always in eights from 8 on (the XCD-owned mapping).  The partial
// sums [M][splits][owners_per_launch * out_width] stay within `cap` bytes by cutting the owners into launches of whole workgroups, never by dropping below the L2
// rule's split count: the splits are what keeps a streamed chunk in one XCD's L2.
struct RowsPlan {
  int form, M, T, splits;
  int64_t chunk, owners_per_launch, launches, wg_x, workspace_bytes;   // wg_x: workgroups along the owners of one launch of owners_per_launch owners
};
RowsPlan make_plan_rows(int form, int T, int64_t owners, int64_t streamed, int64_t streamed_reals, int64_t out_width, int64_t rs, int64_t cap);
// ... of one direction.  Forward: a streamed source brings its normal and M densities, and the bound is a fixed 2 GB.  Transposed: a streamed target brings M
// weight vectors, and SCTL_AMD_TRANSPOSE_WORKSPACE may lower the bound of 2 GB (it never touches the forward plan).
template <class Dir> RowsPlan make_plan_multi(const KernelEntry& k, const RowsEntry<Dir>& me, int form, int real, int64_t Nt, int64_t Ns);

// ---- geometry gradients for several density / weight rows (multi_grad_kernel.hpp) ----
const MultiGEntry* multi_g_entry(int kernel_id);    // null for a registered plugin kernel: its rows go one at a time through the single gradient path
int multi_g_form(const MultiGEntry& me, int left);  // as multi_form
// make_plan_g with M rows in a streamed record: plan_owned with one owner per lane, the L2 rule counting all M rows in a split's streamed bytes, and the
// splits in eights from 8 on.  The partial sums are [splits][owners * 3] (6 with a normal) whatever M is: the bound and its lowering variable are the
// single gradient's.
PlanOwned make_plan_gm(const KernelEntry& k, int M, int real, int side, int64_t Nt, int64_t Ns);

// ---- the tangent of the field along a perturbation of the geometry (jvp_kernel.hpp) ----
const JvpEntry* jvp_entry(int kernel_id);           // null for a registered plugin kernel: the tangent is built for the built-in kernels only
int no_jvp(const KernelEntry& k);                   // sets the error text, returns SCTL_AMD_ERR_UNKNOWN_KERNEL
// plan_owned with the targets as owners of K1 sums each and the sources streamed as {x, dx, n, dn, f}; the owner cut honours the same bound, and the same
// lowering variable, as the transposed and the gradient plans
PlanOwned make_plan_j(const KernelEntry& k, const JvpEntry& je, int real, int64_t Nt, int64_t Ns);

// ---- the tile-centred fast path (centered.hip) ----
// mode < 0: the mode of the default accuracy request (what an operator handle sorts its targets for)
bool has_centered_path(const KernelEntry& k, int real, int mode = -1);
constexpr int64_t kPresortMinTargets = 1 << 17;   // sctl_amd_op_* keeps the targets of such kernels in Morton order from this size on
// nt_whole: size of the target set the Nt targets were cut from as a spatially compact slab (= Nt for a whole set)
bool use_centered(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, int64_t nt_whole = 0, bool presorted = false, int mode = -1);

bool has_transpose(const KernelEntry& k);
int no_transpose(const KernelEntry& k);   // sets the error text, returns SCTL_AMD_ERR_UNKNOWN_KERNEL
bool has_grad(const KernelEntry& k);
int no_grad(const KernelEntry& k);

// ---- drivers: device arrays, enqueued on st; results are accumulated into ----
// v[t,k1] += scale * sum_s U(x_t - x_s, n_s)[k0][k1] f[s,k0]
int eval_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, void* v, int digits,
                const void* ctx, hipStream_t st, int64_t nt_whole = 0, bool presorted = false);
// nd >= 2 densities, density-major (a single density must take eval_device: this one would run it on the 2-density form)
int eval_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, void* v,
                          int digits, const void* ctx, hipStream_t st, int64_t nt_whole = 0, bool presorted = false);
// g[s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] w[t,k1]
int eval_transpose_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* w, void* g,
                          int digits, const void* ctx, hipStream_t st);
// nd >= 2 weight vectors, row-major: g[m] += A^T w[m] (a single row must take eval_transpose_device: this one would run it on the form of 2)
int eval_transpose_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* w,
                                    void* g, int digits, const void* ctx, hipStream_t st);
// g_trg, g_src, g_nrm += the gradients of <w, A f> with respect to the target coordinates, the source coordinates and the source normals; a null output is
// not computed, and a side whose outputs are all null is not launched
int eval_grad_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, const void* w,
                     void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, hipStream_t st);
// nd >= 2 density and weight rows, row-major: the outputs += the gradients of sum_m <w[m], A f[m]> (a single row must take eval_grad_device: this one
// would run it on the form of 2)
int eval_grad_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f,
                               const void* w, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, hipStream_t st);
// dv[t,k1] += the tangent of v = A f along (dxt, dxs, dxn), the densities held fixed; a null tangent is a field of zeros, and with all three null nothing
// is launched.  Built-in kernels only (the caller checks jvp_entry)
int eval_jvp_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, const void* dxt,
                    const void* dxs, const void* dxn, void* dv, int digits, const void* ctx, hipStream_t st);
int matrix_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, void* M, int digits, const void* ctx,
                  hipStream_t st);
void matrix_batch_launch(const KernelEntry& k, int real, const MatTile* tiles, int64_t ntiles, const void* xt, const void* xs, const void* xn, void* M,
                         int digits, const void* ctx, hipStream_t st);

// ---- the operator handle's small pre/post kernels, one launch per density row (rows `stride` reals apart); the caller asks hipGetLastError ----
void scale_density(int real, void* f, const void* w, int64_t Ns, int k0, int nd, hipStream_t st);                     // f[m][s][:] *= w[s]
void normal_dot(int real, const void* v, const void* nrm, void* u, int64_t nt, int k1r, int nd, hipStream_t st);     // u[m][t][k] = sum_l v[m][t][k*3+l] nrm[t][l]
void normal_expand(int real, const void* w, const void* nrm, void* wf, int64_t nt, int k1r, int nd, hipStream_t st); // its adjoint: wf[m][t][k*3+l] = w[m][t][k] nrm[t][l]

}  // namespace sctl_amd
#pragma GCC visibility pop
