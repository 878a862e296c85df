// Launch planning and the typed launch drivers of the all-pairs evaluators, behind the untyped functions of eval_drivers.hpp: the forward sum, several
// densities, the transposed sum, several weight vectors through it, the geometry gradients, the tangent along a perturbation of the geometry and the kernel
// matrix.  All arithmetic lives in eval_kernel.hpp / rows_kernel.hpp (several rows, both directions) / multi_grad_kernel.hpp / jvp_kernel.hpp / ukernels.hpp.
#include "eval_drivers.hpp"
#include "workspace.hpp"

#include <cstdlib>
#include <mutex>
#include <string>

namespace sctl_amd {
namespace {
template <class R> EvalLaunch<R> pick_eval(const KernelEntry& k, int mode, int t);
template <> EvalLaunch<double> pick_eval<double>(const KernelEntry& k, int mode, int t) { return k.eval_f64[mode][t]; }
template <> EvalLaunch<float> pick_eval<float>(const KernelEntry& k, int mode, int t) { return k.eval_f32[mode][t]; }
template <class R> EvalTLaunch<R> pick_eval_t(const KernelEntry& k, int mode, int t);
template <> EvalTLaunch<double> pick_eval_t<double>(const KernelEntry& k, int mode, int t) { return k.eval_t_f64[mode][t]; }
template <> EvalTLaunch<float> pick_eval_t<float>(const KernelEntry& k, int mode, int t) { return k.eval_t_f32[mode][t]; }
template <class R> MatrixLaunch<R> pick_matrix(const KernelEntry& k, int mode);
template <> MatrixLaunch<double> pick_matrix<double>(const KernelEntry& k, int mode) { return k.matrix_f64[mode]; }
template <> MatrixLaunch<float> pick_matrix<float>(const KernelEntry& k, int mode) { return k.matrix_f32[mode]; }

template <class R> EvalGLaunch<R> pick_eval_g(const KernelEntry& k, int mode, int side);
template <> EvalGLaunch<double> pick_eval_g<double>(const KernelEntry& k, int mode, int side) { return k.eval_g_f64[mode][side]; }
template <> EvalGLaunch<float> pick_eval_g<float>(const KernelEntry& k, int mode, int side) { return k.eval_g_f32[mode][side]; }
}  // namespace

int cu_count() {   // CUs of the current device; 256 (MI355X) when planning without a device
  static std::once_flag once;
  static int cus = 256;
  std::call_once(once, [] {
    int dev = 0, n = 0;
    if (device_count_quiet() > 0 && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
  });
  return cus;
}

// Geometry: targets per lane from the target count, then split the source range until there are enough workgroups
// (SURVEY.md §8e sizes: 2^14 .. 2^23).
Plan make_plan(const KernelEntry& k, int real, int64_t Nt, int64_t Ns) {
  // workgroups wanted: 8 per CU (32 waves) — measured +4 % over 4 per CU at Nt = 2^17, Ns = 2^20 and on the Stokeslet at
  // 2^18 — except for tiny problems, which are launch-bound and lose time to the extra partial sums
  // (2 / 4 / 6 / 8 per CU for small problems, and two targets per lane from other sizes on: profiles/r02_small_problem_plans.txt)
  const int64_t want = (int64_t)cu_count() * ((double)Nt * (double)Ns < 2147483648.0 ? 4 : 8);
  Plan p{};
  // Two targets per lane halve the LDS reads per pair and double the independent chains: 5-7 % faster than one target
  // per lane from Nt = 2^16 up on every kernel (Stokeslet 2^18: 56.2 vs 59.7 ms; traction kernel 72.5 vs 77.9 ms), with
  // the source range split further to keep the chip full; at Nt <= 2^14 one target per lane wins (0.18 vs 0.20 ms).
  (void)k;
  const int t = (Nt >= 32768) ? 2 : 1;
  p.t_idx = (t == 1) ? 0 : 1;
  p.wg_x = (Nt + (int64_t)kBlock * t - 1) / ((int64_t)kBlock * t);
  if (p.wg_x < 1) p.wg_x = 1;
  const int64_t ntile = (Ns + kTile - 1) / kTile;
  int64_t s = (want + p.wg_x - 1) / p.wg_x;
  if (s > ntile) s = ntile;
  if (s > 1024) s = 1024;
  if (s < 1) s = 1;
  // Splits sized for the L2, in eights (round 3; A/B on one box, profiles/r03_ab_eval_l2_splits.txt): large problems used to get ONE split
  // and exactly one round of workgroups (2^20 targets, two per lane: 2048 workgroups = 8 per CU), every XCD streaming the whole source set
  // past its 4 MB L2 and nothing left to even out the CUs.  With one split's source data <= 2 MB, the splits a multiple of 8 and each split
  // owned by one XCD (eval_kernel.hpp) the launch has 8-32 x more workgroups than the chip holds at once: 1.3-2.8 % faster (Stokeslet 2^18,
  // SL+DL 2^20, Helmholtz 2^20).  Bounded: at most 64 splits, at most 4 GB of partial sums; problems under 2^34 pairs keep the old plan.
  if ((double)Nt * (double)Ns >= 17179869184.0) {
    const int64_t rs = (int64_t)real_size(real);
    const int64_t src_bytes = Ns * (3 + k.nd + k.k0) * rs;
    int64_t s2 = (src_bytes + (2 << 20) - 1) / (2 << 20);
    s2 = (s2 + 7) / 8 * 8;
    if (s2 > 64) s2 = 64;
    const int64_t ws_cap = ((int64_t)4 << 30) / (Nt * k.k1 * rs) / 8 * 8;
    if (s2 > ws_cap) s2 = ws_cap;
    if (s2 > s) s = s2;
    if (s >= 8) s = (s + 7) / 8 * 8;      // in eights also when the workgroup count, not the L2, asked for the splits (the XCD mapping needs it)
    if (s > ntile) s = ntile;
  }
  int64_t tiles_per = (ntile + s - 1) / s;
  if (tiles_per < 1) tiles_per = 1;
  p.chunk = tiles_per * kTile;
  p.splits = (int)((Ns + p.chunk - 1) / p.chunk);
  if (p.splits < 1) p.splits = 1;
  p.workspace_bytes = (p.splits > 1) ? (int64_t)p.splits * Nt * k.k1 * (int64_t)real_size(real) : 0;
  return p;
}

namespace {
constexpr int64_t kTransposeWorkspaceCap = (int64_t)2 << 30;
// SCTL_AMD_TRANSPOSE_WORKSPACE=<bytes> lowers the bound (never raises it), read per call as SCTL_AMD_CENTERED is: a test runs the several-launch
// cut of the owners on a small shape with it
int64_t transpose_workspace_cap() {
  const char* e = std::getenv("SCTL_AMD_TRANSPOSE_WORKSPACE");
  if (!e || !e[0]) return kTransposeWorkspaceCap;
  const long long v = std::atoll(e);
  return (v >= 1 && v < kTransposeWorkspaceCap) ? (int64_t)v : kTransposeWorkspaceCap;
}
}  // namespace
PlanOwned plan_owned(int64_t owners, int64_t streamed, int t, int64_t streamed_reals, int64_t out_width, int64_t rs) {
  const int64_t want = (int64_t)cu_count() * ((double)owners * (double)streamed < 2147483648.0 ? 4 : 8);
  PlanOwned p{};
  int64_t wg_x = (owners + (int64_t)kBlock * t - 1) / ((int64_t)kBlock * t);
  if (wg_x < 1) wg_x = 1;
  const int64_t ntile = (streamed + kTile - 1) / kTile;
  int64_t s = (want + wg_x - 1) / wg_x;
  if (s > ntile) s = ntile;
  if (s > 1024) s = 1024;
  if (s < 1) s = 1;
  if ((double)owners * (double)streamed >= 17179869184.0) {   // one split's streamed data <= 2 MB, splits in eights, at most 64 (make_plan)
    const int64_t bytes = streamed * streamed_reals * rs;
    int64_t s2 = (bytes + (2 << 20) - 1) / (2 << 20);
    s2 = (s2 + 7) / 8 * 8;
    if (s2 > 64) s2 = 64;
    if (s2 > s) s = s2;
    if (s >= 8) s = (s + 7) / 8 * 8;
    if (s > ntile) s = ntile;
  }
  int64_t tiles_per = (ntile + s - 1) / s;
  if (tiles_per < 1) tiles_per = 1;
  p.chunk = tiles_per * kTile;
  p.splits = (int)((streamed + p.chunk - 1) / p.chunk);
  if (p.splits < 1) p.splits = 1;
  p.owners_per_launch = owners > 0 ? owners : 1;
  if (p.splits > 1) {
    const int64_t group = (int64_t)kBlock * t;
    int64_t cap = transpose_workspace_cap() / ((int64_t)p.splits * out_width * rs) / group * group;   // >= 2^31 / (1024 * 32 * 8) = 8192 owners
    if (cap < group) cap = group;
    if (p.owners_per_launch > cap) p.owners_per_launch = cap;
  }
  p.workspace_bytes = (p.splits > 1) ? (int64_t)p.splits * p.owners_per_launch * out_width * rs : 0;
  return p;
}
PlanT make_plan_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns) {
  const int t = (Ns >= 32768) ? 2 : 1;
  const PlanOwned o = plan_owned(Ns, Nt, t, 3 + k.k1, k.k0, (int64_t)real_size(real));
  PlanT p{};
  p.t_idx = (t == 1) ? 0 : 1;
  p.splits = o.splits; p.chunk = o.chunk; p.owners_per_launch = o.owners_per_launch; p.workspace_bytes = o.workspace_bytes;
  return p;
}
// The gradient evaluation (eval_grad_kernel.hpp).  side 0: the targets own 3 sums each and the sources stream as {x, n, f}; side 1: the sources own 3
// sums, 6 with a normal, and the targets stream as {x, w}.  The owner cut honours the same bound, and the same lowering variable, as the transposed plan.
static int grad_out_width(const KernelEntry& k, int side) { return (side == 1 && k.nd > 0) ? 6 : 3; }
PlanOwned make_plan_g(const KernelEntry& k, int real, int side, int64_t Nt, int64_t Ns) {
  const int64_t rs = (int64_t)real_size(real);
  if (side == 0) return plan_owned(Nt, Ns, k.grad_t[0], 3 + k.nd + k.k0, 3, rs);
  return plan_owned(Ns, Nt, k.grad_t[1], 3 + k.k1, grad_out_width(k, 1), rs);
}
PlanOwned make_plan_gm(const KernelEntry& k, int M, int real, int side, int64_t Nt, int64_t Ns) {
  const int64_t rs = (int64_t)real_size(real), owners = side == 0 ? Nt : Ns, width = grad_out_width(k, side);
  PlanOwned p = side == 0 ? plan_owned(Nt, Ns, 1, 3 + k.nd + (int64_t)M * k.k0, width, rs) : plan_owned(Ns, Nt, 1, 3 + (int64_t)M * k.k1, width, rs);
  if (p.splits >= 8 && (p.splits & 7)) {   // in eights (the splits past the streamed set have no work): the XCD-owned mapping; the owner cut follows
    p.splits = (p.splits + 7) / 8 * 8;
    int64_t cap = transpose_workspace_cap() / ((int64_t)p.splits * width * rs) / kBlock * kBlock;
    if (cap < kBlock) cap = kBlock;
    p.owners_per_launch = owners > 0 ? owners : 1;
    if (p.owners_per_launch > cap) p.owners_per_launch = cap;
    p.workspace_bytes = (int64_t)p.splits * p.owners_per_launch * width * rs;
  }
  return p;
}

// Tile-centred fast path (centered_kernel.hpp): Laplace single layer (fp64 and fp32) on problems large enough to amortise the
// Morton sort of the targets.  SCTL_AMD_CENTERED=0 in the environment forces the exact kernel (used for A/B checks).
// nt_whole: size of the target set the Nt targets were cut from as a spatially compact slab (= Nt for a whole set).
// Laplace single and double layer (fp64 and fp32) and, fp64 only, the gradient of the single layer and the Stokes velocity + pressure kernel (round 4: far sources
// summed as moments)
// mode < 0: the mode of the default accuracy request (what an operator handle sorts its targets for)
bool has_centered_path(const KernelEntry& k, int real, int mode) {
  if (mode < 0) mode = mode_for(real, -1);
  if (k.id == SCTL_AMD_LAPLACE3D_FXU || k.id == SCTL_AMD_LAPLACE3D_DXU) return true;
  if (real == SCTL_AMD_F64) return k.id == SCTL_AMD_LAPLACE3D_FXDU || k.id == SCTL_AMD_STOKES3D_FXUP;
  // fp32: the Stokeslet family and the stresslet at the seed's accuracy, r2 and the dot products on the matrix cores (centered_mfma_kernel.hpp); more digits: the exact kernel
  return (k.id == SCTL_AMD_STOKES3D_FXU || k.id == SCTL_AMD_STOKES3D_FSXU || k.id == SCTL_AMD_STOKES3D_FXUP || k.id == SCTL_AMD_STOKES3D_DXU || k.id == SCTL_AMD_STOKES3D_FXT || k.id == SCTL_AMD_LAPLACE3D_FXDU || k.id == SCTL_AMD_LAPLACE3D_FDXUDU) && centered_pipe(k.id, real, mode) == 2;
}
bool use_centered(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, int64_t nt_whole, bool presorted, int mode) {
  const char* e = std::getenv("SCTL_AMD_CENTERED");   // read per call so that a test can A/B both paths in one process
  const bool enabled = !(e && e[0] == '0'), forced = (e && e[0] == '1');
  if (!enabled || !has_centered_path(k, real, mode) || Nt >= (int64_t(1) << 32)) return false;
  if (forced) return Nt >= 128 && Ns >= 64;
  // (targets already in Morton order — `presorted`, no per-call sort/gather/scatter — do not move the crossover: at 2^17 x 2^17 the
  // centred kernel itself is level with the exact one, 8.14 vs 8.05 ms, because ~10 % of the sources are near; tools/presorted_threshold.py)
  (void)presorted;
  // What decides is the target DENSITY: with too few targets in the domain the 128 targets of a wave span so much of it
  // that many sources are "near" and the exact kernel wins.  Measured with the near threshold 4 Rt^2 (tools/centred_threshold.py,
  // profiles/r01d_centred_threshold.txt; fp64, exact vs centred): 2^18 x 2^18 34.4 vs 32.1 ms, 2^20 x 2^14 8.69 vs 8.38 ms,
  // 2^17 x 2^20 67.7 vs 65.6 ms, but 2^17 x 2^17 8.51 vs 8.88 ms and 2^16 x 2^20 34.96 vs 35.15 ms.  A compact slab of 2^17 out
  // of 2^20 has the density of the whole set and gains like it (59.4 ms against 64.7 ms exact, tools/slab_locality.py).
  const int64_t dens = Nt > nt_whole ? Nt : nt_whole;
  if (dens >= (1 << 18)) return Nt >= (1 << 17) && Ns >= (Nt >= (1 << 18) ? (1 << 14) : (1 << 16));
  return Nt >= (1 << 17) && Ns >= (1 << 20);
}

bool has_transpose(const KernelEntry& k) { return k.nrec_t > 0 && k.eval_t_f64[0][0] != nullptr; }
int no_transpose(const KernelEntry& k) {
  return fail(SCTL_AMD_ERR_UNKNOWN_KERNEL, std::string("kernel '") + k.name + "' has no transposed form: its functor supplies no pair_t (device/kernel_plugin.hpp)");
}
bool has_grad(const KernelEntry& k) { return k.grad_t[0] > 0 && k.eval_g_f64[0][0] != nullptr; }
int no_grad(const KernelEntry& k) {
  return fail(SCTL_AMD_ERR_UNKNOWN_KERNEL, std::string("kernel '") + k.name + "' has no gradient form: its functor supplies no pair_g (device/kernel_plugin.hpp)");
}

namespace {
template <class R>
int run_centered(const KernelEntry& k, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, R* v, int mode, hipStream_t st, bool presorted,
                 int64_t nt_whole) {
  // density of the target set: the size of the set these targets were cut from as a compact slab (the whole set for a plain call)
  HIP_TRY(eval_centered<R>(k.id, Nt, Ns, xt, xs, xn, f, v, k.scale / k.acc_factor[mode], mode, cu_count(), st, presorted, Nt > nt_whole ? Nt : nt_whole));
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}

template <class R>
int eval_device_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, R* v, int digits,
                  const void* ctx, hipStream_t st, int64_t nt_whole = 0, bool presorted = false) {
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;   // nothing to add (generic-kernel.txx:153-186 degenerates to v_trg += 0)
  (void)hipGetLastError();                      // drop a stale error of an earlier, unrelated runtime call on this thread
  const Plan p = make_plan(k, real, Nt, Ns);
  const int mode = mode_for(real, digits);
  if (use_centered(k, real, Nt, Ns, nt_whole, presorted, mode)) return run_centered<R>(k, Nt, Ns, xt, xs, xn, f, v, mode, st, presorted, nt_whole);
  EvalArgs<R> a{};
  a.Nt = Nt; a.Ns = Ns; a.xt = xt; a.xs = xs; a.xn = xn; a.f = f; a.v_trg = v; a.partial = nullptr;
  a.chunk = p.chunk; a.scale = (R)(k.scale / k.acc_factor[mode]); a.ctx = make_ctx(k, ctx);   // pair() of this mode may accumulate a multiple (launch.hpp)
  if (p.splits > 1) {
    void* ws = nullptr;
    HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));   // the block of this stream (workspace.hpp), not the HIP pool
    a.partial = (R*)ws;
  }
  const dim3 grid((unsigned)p.wg_x, (unsigned)p.splits);
  pick_eval<R>(k, mode, p.t_idx)(a, grid, st);
  HIP_TRY(hipGetLastError());
  if (p.splits > 1) {
    const int64_t n = Nt * k.k1;
    hipLaunchKernelGGL((reduce_splits_kernel<R>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, v, (const R*)a.partial, n,
                       p.splits, (R)(k.scale / k.acc_factor[mode]));
    HIP_TRY(hipGetLastError());
  }
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}

// g[s,k0] += scale * sum_t sum_k1 U(x_t - x_s, n_s)[k0][k1] w[t,k1] on device arrays, enqueued on st
template <class R>
int eval_transpose_device_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* w, R* g, int digits,
                            const void* ctx, hipStream_t st) {
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  (void)hipGetLastError();
  const PlanT p = make_plan_t(k, real, Nt, Ns);
  const int mode = mode_for(real, digits);
  const R scale = (R)(k.scale / k.acc_factor[mode]);
  void* ws = nullptr;
  if (p.splits > 1) HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));
  const int64_t group = (int64_t)kBlock * kTTvalues[p.t_idx];
  for (int64_t s0 = 0; s0 < Ns; s0 += p.owners_per_launch) {   // one launch unless the partial sums of all owners would pass 2 GB
    const int64_t n = (Ns - s0 < p.owners_per_launch) ? Ns - s0 : p.owners_per_launch;
    EvalTArgs<R> a{};
    a.Nt = Nt; a.Ns = n; a.xt = xt; a.xs = xs + s0 * 3; a.xn = xn ? xn + s0 * k.nd : nullptr; a.w = w; a.g_src = g + s0 * k.k0; a.partial = (R*)ws;
    a.chunk = p.chunk; a.scale = scale; a.ctx = make_ctx(k, ctx);
    const dim3 grid((unsigned)((n + group - 1) / group), (unsigned)p.splits);
    pick_eval_t<R>(k, mode, p.t_idx)(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (p.splits > 1) {
      const int64_t m = n * k.k0;
      hipLaunchKernelGGL((reduce_splits_kernel<R>), dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.g_src, (const R*)a.partial, m, p.splits, scale);
      HIP_TRY(hipGetLastError());
    }
  }
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}

// One side of the gradient on device arrays, enqueued on st: `owners` points at xo own g (and gn), the other set streams
template <class R>
int eval_grad_side(const KernelEntry& k, int real, int side, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, const R* w, R* g, R* gn,
                   int mode, const void* ctx, hipStream_t st) {
  const PlanOwned p = make_plan_g(k, real, side, Nt, Ns);
  const R scale = (R)(k.scale / k.grad_factor[mode]);
  const int64_t owners = side == 0 ? Nt : Ns;
  const bool normal = (side == 1 && k.nd > 0);
  void* ws = nullptr;
  if (p.splits > 1) HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));
  const int64_t group = (int64_t)kBlock * k.grad_t[side];
  for (int64_t o0 = 0; o0 < owners; o0 += p.owners_per_launch) {   // one launch unless the partial sums of all owners would pass 2 GB
    const int64_t n = (owners - o0 < p.owners_per_launch) ? owners - o0 : p.owners_per_launch;
    EvalGArgs<R> a{};
    a.No = n; a.partial = (R*)ws; a.chunk = p.chunk; a.scale = scale; a.ctx = make_ctx(k, ctx);
    a.g = g ? g + o0 * 3 : nullptr;
    a.gn = (normal && gn) ? gn + o0 * 3 : nullptr;
    if (side == 0) { a.Nst = Ns; a.xo = xt + o0 * 3; a.xst = xs; a.xn = xn; a.f = f; a.w = w + o0 * k.k1; }
    else { a.Nst = Nt; a.xo = xs + o0 * 3; a.xst = xt; a.xn = xn ? xn + o0 * k.nd : nullptr; a.f = f + o0 * k.k0; a.w = w; }
    const dim3 grid((unsigned)((n + group - 1) / group), (unsigned)p.splits);
    pick_eval_g<R>(k, mode, side)(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (p.splits > 1) {
      const int64_t m = n * 3;
      const dim3 rgrid((unsigned)((m + kBlock - 1) / kBlock));
      if (a.g) hipLaunchKernelGGL((reduce_splits_kernel<R>), rgrid, dim3(kBlock), 0, st, a.g, (const R*)a.partial, m, p.splits, scale);
      if (a.gn) hipLaunchKernelGGL((reduce_splits_kernel<R>), rgrid, dim3(kBlock), 0, st, a.gn, (const R*)a.partial + (int64_t)p.splits * m, m, p.splits, scale);
      HIP_TRY(hipGetLastError());
    }
  }
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}

// g_trg, g_src, g_nrm += the gradients of <w, A f> with respect to the target coordinates, the source coordinates and the source normals; a null output is
// not computed, and a side whose outputs are all null is not launched
template <class R>
int eval_grad_device_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, const R* w, R* g_trg, R* g_src,
                       R* g_nrm, int digits, const void* ctx, hipStream_t st) {
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  (void)hipGetLastError();
  const int mode = mode_for(real, digits);
  if (g_trg) {
    const int rc = eval_grad_side<R>(k, real, 0, Nt, Ns, xt, xs, xn, f, w, g_trg, nullptr, mode, ctx, st);
    if (rc) return rc;
  }
  if (g_src || g_nrm) return eval_grad_side<R>(k, real, 1, Nt, Ns, xt, xs, xn, f, w, g_src, g_nrm, mode, ctx, st);
  return SCTL_AMD_OK;
}

template <class R>
int matrix_device_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, R* M, int digits,
                    const void* ctx, hipStream_t st) {
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  (void)hipGetLastError();
  const int mode = mode_for(real, digits);
  const dim3 grid((unsigned)((Nt + kBlock - 1) / kBlock), (unsigned)(Ns < 65535 ? Ns : 65535));
  pick_matrix<R>(k, mode)(Nt, Ns, xt, xs, xn, M, (R)(k.scale / k.acc_factor[mode]), make_ctx(k, ctx), grid, st);
  HIP_TRY(hipGetLastError());
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}
}  // namespace

// ---- several rows through the all-pairs sum, forward and transposed (sctl_amd_eval_densities_*, sctl_amd_eval_transpose_densities_*, rows_kernel.hpp) --------
// Launch tables of the several-row forms: the built-in kernels only; a registered plugin kernel has none (null) and is evaluated one row at a time.
template <> const MultiEntry* multi_entry<RowsFwd>(int kernel_id) {
  static const MultiEntry* tab[SCTL_AMD_NUM_KERNELS] = {
      &multi_Laplace3D_FxU(), &multi_Laplace3D_DxU(), &multi_Laplace3D_FxdU(),  &multi_Stokes3D_FxU(),      &multi_Stokes3D_DxU(),
      &multi_Stokes3D_FxT(),  &multi_Stokes3D_FSxU(), &multi_Stokes3D_FxUP(), &multi_Laplace3D_FDxUdU(), &multi_Helmholtz3D_FxU()};
  return (kernel_id >= 0 && kernel_id < SCTL_AMD_NUM_KERNELS) ? tab[kernel_id] : nullptr;
}
template <> const MultiTEntry* multi_entry<RowsTrans>(int kernel_id) {
  static const MultiTEntry* tab[SCTL_AMD_NUM_KERNELS] = {
      &multi_t_Laplace3D_FxU(), &multi_t_Laplace3D_DxU(), &multi_t_Laplace3D_FxdU(),  &multi_t_Stokes3D_FxU(),      &multi_t_Stokes3D_DxU(),
      &multi_t_Stokes3D_FxT(),  &multi_t_Stokes3D_FSxU(), &multi_t_Stokes3D_FxUP(), &multi_t_Laplace3D_FDxUdU(), &multi_t_Helmholtz3D_FxU()};
  return (kernel_id >= 0 && kernel_id < SCTL_AMD_NUM_KERNELS) ? tab[kernel_id] : nullptr;
}

RowsPlan make_plan_rows(int form, int T, int64_t owners, int64_t streamed, int64_t streamed_reals, int64_t out_width, int64_t rs, int64_t cap) {
  RowsPlan p{};
  p.form = form; p.M = kRowsM[form]; p.T = T;
  const int64_t per_wg = (int64_t)kBlock * p.T;
  const int64_t ntile = (streamed + kTile - 1) / kTile;
  int64_t l2 = 1;
  if ((double)owners * (double)streamed >= 17179869184.0) {   // one split's streamed data, all M rows of a point with it, <= 2 MB
    const int64_t bytes = streamed * streamed_reals * rs;
    l2 = (bytes + (2 << 20) - 1) / (2 << 20);
    l2 = (l2 + 7) / 8 * 8;
    if (l2 > 64) l2 = 64;
  }
  auto geometry = [&](int64_t n) {
    p.owners_per_launch = n;
    p.wg_x = (n + per_wg - 1) / per_wg;
    const int64_t want = (int64_t)cu_count() * ((double)n * (double)streamed < 2147483648.0 ? 4 : 8);
    int64_t s = (want + p.wg_x - 1) / p.wg_x;
    if (s > 1024) s = 1024;
    if (s < l2) s = l2;
    if (s > ntile) s = ntile;
    if (s < 1) s = 1;
    const int64_t tiles_per = (ntile + s - 1) / s;
    p.chunk = (tiles_per > 0 ? tiles_per : 1) * kTile;
    int64_t splits = (streamed + p.chunk - 1) / p.chunk;
    if (splits >= 8) splits = (splits + 7) / 8 * 8;   // (the splits past the streamed points have no work)
    p.splits = (int)(splits < 1 ? 1 : splits);
    p.workspace_bytes = p.splits > 1 ? (int64_t)p.M * p.splits * n * out_width * rs : 0;
  };
  p.launches = 1;
  for (;;) {
    int64_t n = (owners + p.launches - 1) / p.launches;
    n = (n + per_wg - 1) / per_wg * per_wg;
    if (n > owners) n = owners;
    geometry(n);
    if (p.workspace_bytes <= cap || n <= per_wg) break;
    const int64_t more = (p.workspace_bytes + cap - 1) / cap * p.launches;   // (at least one more launch)
    p.launches = more > p.launches ? more : p.launches + 1;
  }
  p.launches = (owners + p.owners_per_launch - 1) / p.owners_per_launch;
  return p;
}
constexpr int64_t kMultiWorkspaceCap = (int64_t)2 << 30;   // partial sums of one forward launch, [M][splits][nt*K1]: fixed, no variable lowers it
template <class Dir> RowsPlan make_plan_multi(const KernelEntry& k, const RowsEntry<Dir>& me, int form, int real, int64_t Nt, int64_t Ns) {
  const int64_t M = kRowsM[form], rs = (int64_t)real_size(real);
  if constexpr (std::is_same<Dir, RowsFwd>::value) return make_plan_rows(form, me.t[form], Nt, Ns, 3 + k.nd + M * k.k0, k.k1, rs, kMultiWorkspaceCap);
  else return make_plan_rows(form, me.t[form], Ns, Nt, 3 + M * k.k1, k.k0, rs, transpose_workspace_cap());
}
template RowsPlan make_plan_multi<RowsFwd>(const KernelEntry&, const MultiEntry&, int, int, int64_t, int64_t);
template RowsPlan make_plan_multi<RowsTrans>(const KernelEntry&, const MultiTEntry&, int, int, int64_t, int64_t);

namespace {
// nd >= 2 rows, row-major, on the device, in either direction (in: the densities f forward, the weights w transposed; out: v and g): passes of the widest form,
// the last pass on the narrowest form that takes what is left (a single row left over runs on the form of 2, so that every pass keeps this planner's bound).  out
// is accumulated into.  A plugin kernel has no several-row form: `single(in_row, out_row)` sends its rows one at a time through the single-row driver.
template <class Dir, class R, class Single>
int eval_rows_device_t(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* in, R* out, int digits,
                       const void* ctx, hipStream_t st, Single single) {
  if (nd == 0 || Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  constexpr bool FWD = std::is_same<Dir, RowsFwd>::value;
  const int64_t owners = FWD ? Nt : Ns, kout = FWD ? k.k1 : k.k0;
  const int64_t in_stride = FWD ? Ns * k.k0 : Nt * k.k1, out_stride = owners * kout;
  const RowsEntry<Dir>* me = multi_entry<Dir>(k.id);
  const int mode = mode_for(real, digits);
  for (int m0 = 0; m0 < nd;) {
    const int left = nd - m0;
    if (!me) {
      const int rc = single(in + m0 * in_stride, out + m0 * out_stride);
      if (rc) return rc;
      m0++;
      continue;
    }
    (void)hipGetLastError();
    const RowsPlan p = make_plan_multi(k, *me, multi_form(*me, left), real, Nt, Ns);
    const int nact = left < p.M ? left : p.M;
    RowsArgs<R> a{};
    a.n_str = FWD ? Ns : Nt; a.x_str = FWD ? xs : xt; a.in = in + m0 * in_stride; a.in_stride = in_stride; a.out_stride = out_stride;
    a.chunk = p.chunk; a.nact = nact; a.scale = (R)(k.scale / k.acc_factor[mode]); a.ctx = make_ctx(k, ctx);
    if (p.splits > 1) {
      void* ws = nullptr;
      HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));
      a.partial = (R*)ws;
    }
    RowsLaunch<R> launch;
    if constexpr (std::is_same<R, double>::value) launch = me->f64[mode][p.form];
    else launch = me->f32[mode][p.form];
    for (int64_t o0 = 0; o0 < owners; o0 += p.owners_per_launch) {   // one launch unless the partial sums of all owners would pass the bound
      const int64_t no = (owners - o0 < p.owners_per_launch) ? owners - o0 : p.owners_per_launch;
      a.n_own = no; a.x_own = (FWD ? xt : xs) + o0 * 3; a.out = out + m0 * out_stride + o0 * kout;
      a.nrm = (FWD || !xn) ? xn : xn + o0 * k.nd;   // the normals are the sources': they advance with the owner cut only where the sources own
      const dim3 grid((unsigned)((no + (int64_t)kBlock * p.T - 1) / ((int64_t)kBlock * p.T)), (unsigned)p.splits);
      launch(a, grid, st);
      HIP_TRY(hipGetLastError());
      if (p.splits > 1) {
        const int64_t n = no * kout;
        for (int m = 0; m < nact; m++)
          hipLaunchKernelGGL((reduce_splits_kernel<R>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.out + m * out_stride,
                             (const R*)(a.partial + (int64_t)m * p.splits * n), n, p.splits, a.scale);
        HIP_TRY(hipGetLastError());
      }
    }
    count_work((int64_t)nact * Nt * Ns, k);
    m0 += nact;
  }
  return SCTL_AMD_OK;
}
template <class R>
int eval_densities_device_t(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, R* v, int digits,
                            const void* ctx, hipStream_t st, int64_t nt_whole = 0, bool presorted = false) {
  return eval_rows_device_t<RowsFwd, R>(k, real, nd, Nt, Ns, xt, xs, xn, f, v, digits, ctx, st, [&](const R* fm, R* vm) {
    return eval_device_t<R>(k, real, Nt, Ns, xt, xs, xn, fm, vm, digits, ctx, st, nt_whole, presorted);
  });
}
template <class R>
int eval_transpose_densities_device_t(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* w, R* g,
                                      int digits, const void* ctx, hipStream_t st) {
  return eval_rows_device_t<RowsTrans, R>(k, real, nd, Nt, Ns, xt, xs, xn, w, g, digits, ctx, st, [&](const R* wm, R* gm) {
    return eval_transpose_device_t<R>(k, real, Nt, Ns, xt, xs, xn, wm, gm, digits, ctx, st);
  });
}
}  // namespace

// ---- geometry gradients for several density / weight rows (sctl_amd_eval_grad_densities_*, multi_grad_kernel.hpp) ------------------------------
const MultiGEntry* multi_g_entry(int kernel_id) {
  static const MultiGEntry* tab[SCTL_AMD_NUM_KERNELS] = {
      &multi_g_Laplace3D_FxU(), &multi_g_Laplace3D_DxU(), &multi_g_Laplace3D_FxdU(),  &multi_g_Stokes3D_FxU(),      &multi_g_Stokes3D_DxU(),
      &multi_g_Stokes3D_FxT(),  &multi_g_Stokes3D_FSxU(), &multi_g_Stokes3D_FxUP(), &multi_g_Laplace3D_FDxUdU(), &multi_g_Helmholtz3D_FxU()};
  return (kernel_id >= 0 && kernel_id < SCTL_AMD_NUM_KERNELS) ? tab[kernel_id] : nullptr;
}
int multi_g_form(const MultiGEntry& me, int left) {
  for (int i = 0; i < kNumMultiGM; i++)
    if (kMultiGM[i] >= left || kMultiGM[i] == me.m_max) return i;
  return 0;
}

namespace {
// One side of one pass of `nact` rows on the form of kMultiGM[form] rows.  A form that is not in the table is served by the single kernel, one row at a time
// into the same outputs.
template <class R>
int eval_grad_multi_side(const KernelEntry& k, const MultiGEntry& me, int form, int real, int side, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn,
                         const R* f, const R* w, int nact, R* g, R* gn, int mode, const void* ctx, hipStream_t st) {
  const int64_t f_stride = Ns * k.k0, w_stride = Nt * k.k1;
  MultiGLaunch<R> launch;
  if constexpr (std::is_same<R, double>::value) launch = me.f64[mode][side][form];
  else launch = me.f32[mode][side][form];
  if (!launch) {
    for (int m = 0; m < nact; m++)
      if (const int rc = eval_grad_side<R>(k, real, side, Nt, Ns, xt, xs, xn, f + m * f_stride, w + m * w_stride, g, gn, mode, ctx, st)) return rc;
    return SCTL_AMD_OK;
  }
  const PlanOwned p = make_plan_gm(k, kMultiGM[form], real, side, Nt, Ns);
  const R scale = (R)(k.scale / k.grad_factor[mode]);
  const int64_t owners = side == 0 ? Nt : Ns;
  const bool normal = (side == 1 && k.nd > 0);
  void* ws = nullptr;
  if (p.splits > 1) HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));
  for (int64_t o0 = 0; o0 < owners; o0 += p.owners_per_launch) {   // one launch unless the partial sums of all owners would pass 2 GB
    const int64_t n = (owners - o0 < p.owners_per_launch) ? owners - o0 : p.owners_per_launch;
    MultiGArgs<R> a{};
    a.No = n; a.partial = (R*)ws; a.chunk = p.chunk; a.nact = nact; a.scale = scale; a.ctx = make_ctx(k, ctx);
    a.f_stride = f_stride; a.w_stride = w_stride;
    a.g = g ? g + o0 * 3 : nullptr;
    a.gn = (normal && gn) ? gn + o0 * 3 : nullptr;
    if (side == 0) { a.Nst = Ns; a.xo = xt + o0 * 3; a.xst = xs; a.xn = xn; a.f = f; a.w = w + o0 * k.k1; }
    else { a.Nst = Nt; a.xo = xs + o0 * 3; a.xst = xt; a.xn = xn ? xn + o0 * k.nd : nullptr; a.f = f + o0 * k.k0; a.w = w; }
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock), (unsigned)p.splits);
    launch(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (p.splits > 1) {
      const int64_t m = n * 3;
      const dim3 rgrid((unsigned)((m + kBlock - 1) / kBlock));
      if (a.g) hipLaunchKernelGGL((reduce_splits_kernel<R>), rgrid, dim3(kBlock), 0, st, a.g, (const R*)a.partial, m, p.splits, scale);
      if (a.gn) hipLaunchKernelGGL((reduce_splits_kernel<R>), rgrid, dim3(kBlock), 0, st, a.gn, (const R*)a.partial + (int64_t)p.splits * m, m, p.splits, scale);
      HIP_TRY(hipGetLastError());
    }
  }
  count_work((int64_t)nact * Nt * Ns, k);
  return SCTL_AMD_OK;
}

// nd >= 2 rows, row-major, on the device: passes of the widest form, the last pass on the narrowest form that takes what is left, every pass accumulating
// into the same outputs.  A plugin kernel with pair_g has no pair_gm: its rows go one at a time through the single path, which is exact (the outputs are sums).
template <class R>
int eval_grad_densities_device_t(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, const R* w,
                                 R* g_trg, R* g_src, R* g_nrm, int digits, const void* ctx, hipStream_t st) {
  if (nd == 0 || Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  const int64_t f_stride = Ns * k.k0, w_stride = Nt * k.k1;
  const MultiGEntry* me = multi_g_entry(k.id);
  const int mode = mode_for(real, digits);
  for (int m0 = 0; m0 < nd;) {
    const R* fm = f + m0 * f_stride;
    const R* wm = w + m0 * w_stride;
    if (!me) {
      if (const int rc = eval_grad_device_t<R>(k, real, Nt, Ns, xt, xs, xn, fm, wm, g_trg, g_src, g_nrm, digits, ctx, st)) return rc;
      m0++;
      continue;
    }
    (void)hipGetLastError();
    const int left = nd - m0, form = multi_g_form(*me, left);
    const int nact = left < kMultiGM[form] ? left : kMultiGM[form];
    if (g_trg)
      if (const int rc = eval_grad_multi_side<R>(k, *me, form, real, 0, Nt, Ns, xt, xs, xn, fm, wm, nact, g_trg, nullptr, mode, ctx, st)) return rc;
    if (g_src || g_nrm)
      if (const int rc = eval_grad_multi_side<R>(k, *me, form, real, 1, Nt, Ns, xt, xs, xn, fm, wm, nact, g_src, g_nrm, mode, ctx, st)) return rc;
    m0 += nact;
  }
  return SCTL_AMD_OK;
}
}  // namespace

// ---- the tangent of the field along a perturbation of the geometry (sctl_amd_eval_jvp_*, jvp_kernel.hpp) -----------------------------------------
const JvpEntry* jvp_entry(int kernel_id) {
  static const JvpEntry* tab[SCTL_AMD_NUM_KERNELS] = {&jvp_Laplace3D_FxU(), &jvp_Laplace3D_DxU(), &jvp_Laplace3D_FxdU(),   &jvp_Stokes3D_FxU(),
                                                      &jvp_Stokes3D_DxU(),  &jvp_Stokes3D_FxT(),  &jvp_Stokes3D_FSxU(),    &jvp_Stokes3D_FxUP(),
                                                      &jvp_Laplace3D_FDxUdU(), &jvp_Helmholtz3D_FxU()};
  return (kernel_id >= 0 && kernel_id < SCTL_AMD_NUM_KERNELS) ? tab[kernel_id] : nullptr;
}
int no_jvp(const KernelEntry& k) {
  return fail(SCTL_AMD_ERR_UNKNOWN_KERNEL, std::string("kernel '") + k.name + "' has no tangent form: sctl_amd_eval_jvp_* is built for the built-in kernels only");
}
PlanOwned make_plan_j(const KernelEntry& k, const JvpEntry& je, int real, int64_t Nt, int64_t Ns) {
  return plan_owned(Nt, Ns, je.t, 6 + 2 * k.nd + k.k0, k.k1, (int64_t)real_size(real));
}

namespace {
template <class R>
int eval_jvp_device_t(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const R* xt, const R* xs, const R* xn, const R* f, const R* dxt, const R* dxs,
                      const R* dxn, R* dv, int digits, const void* ctx, hipStream_t st) {
  if (Nt == 0 || Ns == 0 || (!dxt && !dxs && !dxn)) return SCTL_AMD_OK;   // nothing to add: the tangent along a zero perturbation is zero
  (void)hipGetLastError();
  const JvpEntry& je = *jvp_entry(k.id);
  const PlanOwned p = make_plan_j(k, je, real, Nt, Ns);
  const int mode = mode_for(real, digits);
  const R scale = (R)(k.scale / k.grad_factor[mode]);   // pair_j accumulates the multiple pair_g does
  EvalJLaunch<R> launch;
  if constexpr (std::is_same<R, double>::value) launch = je.f64[mode];
  else launch = je.f32[mode];
  void* ws = nullptr;
  if (p.splits > 1) HIP_TRY(workspace_acquire(st, (size_t)p.workspace_bytes, &ws));
  const int64_t group = (int64_t)kBlock * je.t;
  for (int64_t t0 = 0; t0 < Nt; t0 += p.owners_per_launch) {   // one launch unless the partial sums of all targets would pass 2 GB
    const int64_t n = (Nt - t0 < p.owners_per_launch) ? Nt - t0 : p.owners_per_launch;
    EvalJArgs<R> a{};
    a.Nt = n; a.Ns = Ns; a.xt = xt + t0 * 3; a.dxt = dxt ? dxt + t0 * 3 : nullptr; a.xs = xs; a.dxs = dxs; a.xn = xn; a.dxn = k.nd ? dxn : nullptr; a.f = f;
    a.dv = dv + t0 * k.k1; a.partial = (R*)ws; a.chunk = p.chunk; a.scale = scale; a.ctx = make_ctx(k, ctx);
    const dim3 grid((unsigned)((n + group - 1) / group), (unsigned)p.splits);
    launch(a, grid, st);
    HIP_TRY(hipGetLastError());
    if (p.splits > 1) {
      const int64_t m = n * k.k1;
      hipLaunchKernelGGL((reduce_splits_kernel<R>), dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.dv, (const R*)a.partial, m, p.splits, scale);
      HIP_TRY(hipGetLastError());
    }
  }
  count_work(Nt * Ns, k);
  return SCTL_AMD_OK;
}
}  // namespace

// ---- the untyped seam: `real` picks the template here and nowhere else ----------------------------------------------------------------------------
int eval_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, void* v, int digits,
                const void* ctx, hipStream_t st, int64_t nt_whole, bool presorted) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_device_t<R>(k, real, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)f, (R*)v, digits, ctx, st, nt_whole, presorted); });
}
int eval_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, void* v,
                          int digits, const void* ctx, hipStream_t st, int64_t nt_whole, bool presorted) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_densities_device_t<R>(k, real, nd, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)f, (R*)v, digits, ctx, st, nt_whole, presorted); });
}
int eval_transpose_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* w, void* g,
                          int digits, const void* ctx, hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_transpose_device_t<R>(k, real, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)w, (R*)g, digits, ctx, st); });
}
int eval_transpose_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* w,
                                    void* g, int digits, const void* ctx, hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_transpose_densities_device_t<R>(k, real, nd, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)w, (R*)g, digits, ctx, st); });
}
int eval_grad_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, const void* w,
                     void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_grad_device_t<R>(k, real, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)f, (const R*)w, (R*)g_trg, (R*)g_src, (R*)g_nrm, digits, ctx, st); });
}
int eval_grad_densities_device(const KernelEntry& k, int real, int nd, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f,
                               const void* w, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_grad_densities_device_t<R>(k, real, nd, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)f, (const R*)w, (R*)g_trg, (R*)g_src, (R*)g_nrm, digits, ctx, st); });
}
int eval_jvp_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, const void* f, const void* dxt,
                    const void* dxs, const void* dxn, void* dv, int digits, const void* ctx, hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return eval_jvp_device_t<R>(k, real, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (const R*)f, (const R*)dxt, (const R*)dxs, (const R*)dxn, (R*)dv, digits, ctx, st); });
}
int matrix_device(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* xt, const void* xs, const void* xn, void* M, int digits, const void* ctx,
                  hipStream_t st) {
  return with_real(real, [&](auto zero) { using R = decltype(zero); return matrix_device_t<R>(k, real, Nt, Ns, (const R*)xt, (const R*)xs, (const R*)xn, (R*)M, digits, ctx, st); });
}
void matrix_batch_launch(const KernelEntry& k, int real, const MatTile* tiles, int64_t ntiles, const void* xt, const void* xs, const void* xn, void* M,
                         int digits, const void* ctx, hipStream_t st) {
  const int mode = mode_for(real, digits);
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    MatrixBatchLaunch<R> launch;
    if constexpr (std::is_same<R, double>::value) launch = k.matrix_batch_f64[mode];
    else launch = k.matrix_batch_f32[mode];
    launch(tiles, ntiles, (const R*)xt, (const R*)xs, (const R*)xn, (R*)M, (R)(k.scale / k.acc_factor[mode]), make_ctx(k, ctx), st);
    return 0;
  });
}

void scale_density(int real, void* f, const void* w, int64_t Ns, int k0, int nd, hipStream_t st) {
  const unsigned nb = (unsigned)((Ns * k0 + kBlock - 1) / kBlock);
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    for (int m = 0; m < nd; m++) hipLaunchKernelGGL((scale_density_kernel<R>), dim3(nb), dim3(kBlock), 0, st, (R*)f + (int64_t)m * Ns * k0, (const R*)w, Ns, k0);
    return 0;
  });
}
void normal_dot(int real, const void* v, const void* nrm, void* u, int64_t nt, int k1r, int nd, hipStream_t st) {
  const unsigned nb = (unsigned)((nt * k1r + kBlock - 1) / kBlock);
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    for (int m = 0; m < nd; m++)
      hipLaunchKernelGGL((normal_dot_kernel<R>), dim3(nb), dim3(kBlock), 0, st, (const R*)v + (int64_t)m * nt * k1r * 3, (const R*)nrm, (R*)u + (int64_t)m * nt * k1r, nt, k1r);
    return 0;
  });
}
void normal_expand(int real, const void* w, const void* nrm, void* wf, int64_t nt, int k1r, int nd, hipStream_t st) {
  const unsigned nb = (unsigned)((nt * k1r * 3 + kBlock - 1) / kBlock);
  with_real(real, [&](auto zero) {
    using R = decltype(zero);
    for (int m = 0; m < nd; m++)
      hipLaunchKernelGGL((normal_expand_kernel<R>), dim3(nb), dim3(kBlock), 0, st, (const R*)w + (int64_t)m * nt * k1r, (const R*)nrm, (R*)wf + (int64_t)m * nt * k1r * 3, nt, k1r);
    return 0;
  });
}

}  // namespace sctl_amd
