// C ABI of libsctl_amd.so (include/sctl_amd.h): the kernel registry and plugin loading, the error text, the shared argument checks, init / finalize,
// the info and plan queries, and the device-pointer entries (checks + one driver call of eval_drivers.hpp).  The host-buffer entries are in
// host_entries.hip, the operator handle in op.hip.  All arithmetic lives in eval_kernel.hpp / rows_kernel.hpp /
// ukernels.hpp.
#include "eval_drivers.hpp"
#include "workspace.hpp"

#include <dlfcn.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>

namespace sctl_amd {
namespace {
thread_local std::string g_err;
}  // namespace
int set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
std::string& error_text() { return g_err; }

// ---- kernel registry: the ten built-in functors, then whatever plugins register (sctl_amd_register_kernel) --------------------
namespace {
constexpr int kMaxKernels = 256;
struct Registry {
  const KernelEntry* tab[kMaxKernels] = {};
  std::atomic<int> n{0};
  std::mutex mu;
  Registry() {
    const KernelEntry* builtin[SCTL_AMD_NUM_KERNELS] = {
        &entry_Laplace3D_FxU(),  &entry_Laplace3D_DxU(),  &entry_Laplace3D_FxdU(),   &entry_Stokes3D_FxU(),   &entry_Stokes3D_DxU(),
        &entry_Stokes3D_FxT(),   &entry_Stokes3D_FSxU(),  &entry_Stokes3D_FxUP(),    &entry_Laplace3D_FDxUdU(), &entry_Helmholtz3D_FxU()};
    for (int i = 0; i < SCTL_AMD_NUM_KERNELS; i++) tab[i] = builtin[i];
    n = SCTL_AMD_NUM_KERNELS;
  }
};
Registry& reg() {
  static Registry* r = new Registry;   // leaked on purpose: plugins may register from static initialisers in any order
  return *r;
}
}  // namespace
const KernelEntry* registry(int id) { return (id >= 0 && id < reg().n.load()) ? reg().tab[id] : nullptr; }
int registry_size() { return reg().n.load(); }
int registry_find(const char* name) {
  if (!name) return SCTL_AMD_ERR_UNKNOWN_KERNEL;
  const int n = reg().n.load();
  for (int i = 0; i < n; i++)
    if (!std::strcmp(reg().tab[i]->name, name)) return i;
  return SCTL_AMD_ERR_UNKNOWN_KERNEL;
}
int registry_add(const KernelEntry& e, std::string* why) {
  Registry& r = reg();
  std::lock_guard<std::mutex> lock(r.mu);
  const int n = r.n.load();
  for (int i = 0; i < n; i++)
    if (!std::strcmp(r.tab[i]->name, e.name)) { *why = std::string("a kernel called '") + e.name + "' is already registered"; return SCTL_AMD_ERR_BAD_ARGUMENT; }
  if (n >= kMaxKernels) { *why = "kernel registry is full"; return SCTL_AMD_ERR_BAD_ARGUMENT; }
  KernelEntry* copy = new KernelEntry(e);          // lives as long as the process (ids are never recycled)
  char* name = new char[std::strlen(e.name) + 1];
  std::strcpy(name, e.name);
  copy->name = name;
  copy->id = n;
  r.tab[n] = copy;
  r.n.store(n + 1);
  return n;
}
namespace {
std::atomic<int64_t> g_pairs{0}, g_flops{0};
}  // namespace
void count_work(int64_t pairs, const KernelEntry& k) { g_pairs += pairs; g_flops += pairs * k.flops; }
int device_count_quiet() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

// digits -> refinement mode of ukernels.hpp rsqrt_masked (the reference maps digits to Newton iteration
// counts at compile time, intrin-wrapper.hpp:3025-3050; -1 and >= 16 mean full precision, generic-kernel.txx:46-77)
int mode_for(int real, int digits) {
  if (real == SCTL_AMD_F64) {
    if (digits < 0 || digits > 14) return 2;
    return digits <= 7 ? 0 : 1;
  }
  return (digits < 0 || digits <= 7) ? 0 : 1;
}
KerCtx make_ctx(const KernelEntry& k, const void* ctx) {
  KerCtx c{};
  if (k.ctx_bytes > 0) std::memcpy(c.v, ctx, (size_t)k.ctx_bytes);
  return c;
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------------
int check_ctx(const KernelEntry& k, const void* ctx, int ctx_bytes) {
  if (k.ctx_bytes != 0 && (ctx_bytes != k.ctx_bytes || !ctx))
    return fail(SCTL_AMD_ERR_BAD_CONTEXT, std::string(k.name) + " needs a context blob of " + std::to_string(k.ctx_bytes) + " bytes");
  return SCTL_AMD_OK;
}
int check_real_sizes(const KernelEntry* k, int real, int64_t Nt, int64_t Ns) {
  if (!k) return fail(SCTL_AMD_ERR_UNKNOWN_KERNEL, "unknown kernel id");
  if (real != SCTL_AMD_F64 && real != SCTL_AMD_F32) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "real must be SCTL_AMD_F64 or SCTL_AMD_F32");
  if (Nt < 0 || Ns < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative size");
  return SCTL_AMD_OK;
}
int check_common(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                 int ctx_bytes, const void* ctx) {
  const int rc = check_real_sizes(k, real, Nt, Ns);
  if (rc) return rc;
  if ((Nt > 0 && !r_trg) || (Ns > 0 && !r_src)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate array");
  if (Ns > 0 && k->nd > 0 && !n_src) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k->name) + " needs source normals (n_src is null)");
  return check_ctx(*k, ctx, ctx_bytes);
}
int no_device() { return fail(SCTL_AMD_ERR_NO_DEVICE, "no HIP device: libsctl_amd has no CPU fallback"); }
int check_device(int device) {
  const int avail = device_count_quiet();
  if (avail <= 0) return no_device();
  if (device < 0 || device >= avail) return fail(SCTL_AMD_ERR_NO_DEVICE, "device index out of range");
  return SCTL_AMD_OK;
}
int check_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                    const void* v_src, const void* v_trg, int ctx_bytes, const void* ctx) {
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd > 0 && ((Ns > 0 && !v_src) || (Nt > 0 && !v_trg))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  return SCTL_AMD_OK;
}
int check_transpose(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                    const void* w_trg, const void* g_src, int ctx_bytes, const void* ctx) {
  const int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((Nt > 0 && !w_trg) || (Ns > 0 && !g_src)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null weight or result array");
  if (!has_transpose(*k)) return no_transpose(*k);
  return SCTL_AMD_OK;
}
int check_transpose_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                              const void* w_trg, const void* g_src, int ctx_bytes, const void* ctx) {
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of weight vectors");
  const int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd > 0 && ((Nt > 0 && !w_trg) || (Ns > 0 && !g_src))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null weight or result array");
  if (!has_transpose(*k)) return no_transpose(*k);
  return SCTL_AMD_OK;
}
int check_grad(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
               const void* w_trg, const void* g_nrm, int ctx_bytes, const void* ctx) {
  const int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((Ns > 0 && !v_src) || (Nt > 0 && !w_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or weight array");
  if (g_nrm && k->nd == 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k->name) + " has no source normal: g_nrm must be null");
  if (!has_grad(*k)) return no_grad(*k);
  return SCTL_AMD_OK;
}
int check_jvp(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
              const void* d_nrm, const void* dv_trg, int ctx_bytes, const void* ctx) {
  const int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((Ns > 0 && !v_src) || (Nt > 0 && !dv_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or tangent result array");
  if (d_nrm && k->nd == 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k->name) + " has no source normal: d_nrm must be null");
  if (!jvp_entry(k->id)) return no_jvp(*k);
  return SCTL_AMD_OK;
}
int check_grad_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                         const void* v_src, const void* w_trg, const void* g_nrm, int ctx_bytes, const void* ctx) {
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of density and weight rows");
  const int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd > 0 && ((Ns > 0 && !v_src) || (Nt > 0 && !w_trg))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or weight array");
  if (g_nrm && k->nd == 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k->name) + " has no source normal: g_nrm must be null");
  if (!has_grad(*k)) return no_grad(*k);
  return SCTL_AMD_OK;
}
// The passes of a call of nd >= 2 rows as the driver makes them (eval_drivers.hip): the first pass is the widest and gives the rows per pass, the owners per
// lane, the splits and the workgroups of all its owner launches; the workspace is the largest any pass asks for.
template <class Dir>
void rows_passes_plan(const KernelEntry& k, const RowsEntry<Dir>& me, int real, int nd, int64_t Nt, int64_t Ns, int* rows_per_pass, int* passes, int* own_per_lane,
                      int* splits, int64_t* workgroups, int64_t* workspace_bytes) {
  constexpr bool FWD = std::is_same<Dir, RowsFwd>::value;
  for (int m0 = 0; m0 < nd;) {
    const int left = nd - m0;
    const RowsPlan p = make_plan_multi(k, me, multi_form(me, left), real, FWD && Nt <= 0 ? 1 : Nt, !FWD && Ns <= 0 ? 1 : Ns);   // (an owner set is never planned empty)
    if (*passes == 0) {
      *rows_per_pass = p.M; *own_per_lane = p.T; *splits = p.splits;
      const int64_t owners = FWD ? Nt : Ns, per_wg = (int64_t)kBlock * p.T;
      for (int64_t o0 = 0; o0 < owners; o0 += p.owners_per_launch) {
        const int64_t n = (owners - o0 < p.owners_per_launch) ? owners - o0 : p.owners_per_launch;
        *workgroups += (n + per_wg - 1) / per_wg * p.splits;
      }
    }
    *workspace_bytes = p.workspace_bytes > *workspace_bytes ? p.workspace_bytes : *workspace_bytes;
    (*passes)++;
    m0 += left < p.M ? left : p.M;
  }
}
}  // namespace sctl_amd

using namespace sctl_amd;

extern "C" {

int sctl_amd_version(void) { return SCTL_AMD_VERSION; }
const char* sctl_amd_last_error(void) { return g_err.c_str(); }
int sctl_amd_device_count(void) { return device_count_quiet(); }

// init / finalise.  Everything in this library initialises lazily, so neither call is required: init() takes the HIP
// runtime's and every device's first-touch cost (context, code-object load: tens to hundreds of ms) out of the first evaluation and
// reports how many GPUs there are; finalize() gives back what the library keeps between calls — the scratch blocks, the operators of the
// host-buffer entry, the calling thread's cached streams / buffers / staging — and leaves it usable (the next call initialises again).
int sctl_amd_init(void) {
  const int n = device_count_quiet();
  if (n <= 0) return 0;
  RestoreDevice restore;
  for (int d = 0; d < n; d++) {
    if (hipSetDevice(d) != hipSuccess || hipFree(nullptr) != hipSuccess) { (void)hipGetLastError(); return fail(SCTL_AMD_ERR_HIP, "cannot initialise device " + std::to_string(d)); }
  }
  return n;
}
void sctl_amd_finalize(void) {
  sctl_amd_trim();
  host_slots_release();
}

int sctl_amd_kernel_id(const char* name) { return registry_find(name); }
int sctl_amd_num_kernels(void) { return registry_size(); }

int sctl_amd_register_kernel(const sctl_amd_kernel_desc* d) {
  if (!d) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null kernel descriptor");
  if (d->abi_version != SCTL_AMD_DEVICE_ABI || d->desc_bytes != (int)sizeof(sctl_amd_kernel_desc) || d->entry_bytes != (int)sizeof(KernelEntry))
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "kernel plugin was compiled with other device headers (ABI " + std::to_string(d->abi_version) + ", library " +
                                              std::to_string(SCTL_AMD_DEVICE_ABI) + "): rebuild it against this library's include/sctl_amd/device");
  const KernelEntry* e = (const KernelEntry*)d->launch_table;
  if (!e || !d->name || !e->name || std::strcmp(e->name, d->name) != 0 || !d->name[0]) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "kernel descriptor without a name or launch table");
  if (e->k0 != d->src_dim || e->k1 != d->trg_dim || e->nd != d->normal_dim || e->flops != d->flops || e->ctx_bytes != d->ctx_bytes || e->scale != d->scale)
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("descriptor of '") + d->name + "' disagrees with its launch table");
  if (e->k0 < 1 || e->k1 < 1 || (e->nd != 0 && e->nd != 3) || e->ctx_bytes < 0 || e->ctx_bytes > (int)sizeof(KerCtx))
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': dimensions or context size out of range");
  for (int m = 0; m < kNumMode; m++) {
    if (!(e->acc_factor[m] > 0) || !e->matrix_f64[m] || !e->matrix_f32[m] || !e->matrix_batch_f64[m] || !e->matrix_batch_f32[m] || !e->lists_f64[m] || !e->lists_f32[m])
      return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': incomplete launch table");
    for (int t = 0; t < kNumT; t++)
      if (!e->eval_f64[m][t] || !e->eval_f32[m][t]) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': incomplete launch table");
  }
  {   // the transposed launchers are optional (a functor without pair_t), but all or none
    int have = 0;
    for (int m = 0; m < kNumMode; m++)
      for (int t = 0; t < kNumTT; t++) have += (e->eval_t_f64[m][t] != nullptr) + (e->eval_t_f32[m][t] != nullptr);
    if ((have != 0 && have != 2 * kNumMode * kNumTT) || (have != 0) != (e->nrec_t > 0))
      return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': incomplete transposed launch table");
  }
  {   // ... and so are the gradient launchers (a functor without pair_g)
    int have = 0;
    for (int m = 0; m < kNumMode; m++)
      for (int side = 0; side < 2; side++) have += (e->eval_g_f64[m][side] != nullptr) + (e->eval_g_f32[m][side] != nullptr);
    const bool named = e->grad_t[0] > 0 && e->grad_t[1] > 0;
    if ((have != 0 && have != 2 * kNumMode * 2) || (have != 0) != named || (e->grad_t[0] > 0) != (e->grad_t[1] > 0))
      return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': incomplete gradient launch table");
    for (int m = 0; m < kNumMode && have; m++)
      if (!(e->grad_factor[m] > 0)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel '") + d->name + "': incomplete gradient launch table");
  }
  std::string why;
  const int id = registry_add(*e, &why);
  return id >= 0 ? id : fail(id, why);
}

int sctl_amd_load_plugin(const char* path) {
  if (!path || !path[0]) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "empty plugin path");
  if (void* loaded = dlopen(path, RTLD_NOW | RTLD_NOLOAD)) {   // already in the process: its initialisers ran when it was first loaded
    (void)loaded;
    return 0;
  }
  const int before = registry_size();
  g_err.clear();                     // the plugin's static registration runs on this thread: a refusal leaves its reason here
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) { const char* e = dlerror(); return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("cannot load kernel plugin: ") + (e ? e : path)); }
  const int added = registry_size() - before;   // the handle is kept open on purpose: registered launch pointers point into the plugin
  if (added == 0) dlclose(h);                   // nothing points into it
  if (added == 0)
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("kernel plugin ") + path + " was loaded but registered no kernel: " +
                                               (g_err.empty() ? std::string("it contains no SCTL_AMD_REGISTER_KERNEL") : std::string(g_err)));
  return added;
}
const char* sctl_amd_kernel_name(int kernel) {
  const KernelEntry* k = registry(kernel);
  return k ? k->name : nullptr;
}
int sctl_amd_kernel_info(int kernel, int* src_dim, int* trg_dim, int* normal_dim, int* flops, double* scale, int* ctx_bytes) {
  const KernelEntry* k = registry(kernel);
  if (!k) return fail(SCTL_AMD_ERR_UNKNOWN_KERNEL, "unknown kernel id");
  if (src_dim) *src_dim = k->k0;
  if (trg_dim) *trg_dim = k->k1;
  if (normal_dim) *normal_dim = k->nd;
  if (flops) *flops = k->flops;
  if (scale) *scale = k->scale;
  if (ctx_bytes) *ctx_bytes = k->ctx_bytes;
  return SCTL_AMD_OK;
}
int sctl_amd_flops_per_pair(int kernel) {
  const KernelEntry* k = registry(kernel);
  return k ? 3 + k->flops + 2 * k->k0 * k->k1 : SCTL_AMD_ERR_UNKNOWN_KERNEL;
}

static int eval_device_entry(int kernel, int real, int64_t Nt, int64_t Ns, int64_t nt_whole, const void* r_trg, const void* r_src, const void* n_src,
                             const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((Ns > 0 && !v_src) || (Nt > 0 && !v_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  if (nt_whole < Nt) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "a slab cannot hold more targets than the set it was cut from");
  // A proper slab IS a run of the space-filling-curve order (the entry's contract): the tile-centred path then needs no sort, gather or
  // scatter of its own.  (Targets in any other order are still evaluated correctly — only slowly: their clusters are large, so most
  // sources take the exact near path.)
  const bool slab_sorted = nt_whole > Nt;
  if (device_count_quiet() <= 0) return no_device();
  return eval_device(*k, real, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, (hipStream_t)stream, nt_whole, slab_sorted);
}

int sctl_amd_eval_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                         const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  return eval_device_entry(kernel, real, Nt, Ns, Nt, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, stream);
}

int sctl_amd_eval_device_slab(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, const void* r_trg, const void* r_src,
                              const void* n_src, const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  return eval_device_entry(kernel, real, Nt, Ns, Nt_whole, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, stream);
}

int sctl_amd_kernel_matrix_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                  void* M, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (Nt > 0 && Ns > 0 && !M) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null matrix");
  if (device_count_quiet() <= 0) return no_device();
  return matrix_device(*k, real, Nt, Ns, r_trg, r_src, n_src, M, digits, ctx, (hipStream_t)stream);
}

// ---- several densities against one geometry ----------------------------------------------------------------------------------------------
// nd == 1 goes through the single-density entry (bit-identical results); nd == 0 is a no-op after the argument checks.
int sctl_amd_eval_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                   const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_device(kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, stream);
  if (device_count_quiet() <= 0) return no_device();
  return eval_densities_device(*k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* densities_per_pass, int* passes, int* trg_per_lane,
                                 int* src_splits, int64_t* workgroups, int64_t* workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  int dpp = 0, np = 0, t = 0, s = 0;
  int64_t wg = 0, ws = 0;
  const MultiEntry* me = multi_entry<RowsFwd>(k->id);
  if (nd == 1 || (nd > 1 && !me)) {   // the single-density plan, once per density
    const int rc = sctl_amd_eval_plan(kernel, real, Nt, Ns, Nt, digits, &t, &s, &wg, &ws);
    if (rc) return rc;
    dpp = 1; np = nd;
  } else if (nd > 1) {
    rows_passes_plan(*k, *me, real, nd, Nt, Ns, &dpp, &np, &t, &s, &wg, &ws);
  }
  if (densities_per_pass) *densities_per_pass = dpp;
  if (passes) *passes = np;
  if (trg_per_lane) *trg_per_lane = t;
  if (src_splits) *src_splits = s;
  if (workgroups) *workgroups = wg;
  if (workspace_bytes) *workspace_bytes = ws;
  return SCTL_AMD_OK;
}

// ---- transposed evaluation: g_src += A^T w_trg --------------------------------------------------------------------------------------
int sctl_amd_eval_transpose_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                   const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_transpose(k, real, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (device_count_quiet() <= 0) return no_device();
  return eval_transpose_device(*k, real, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_transpose_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* src_per_lane, int* splits, int64_t* workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (!has_transpose(*k)) return no_transpose(*k);
  (void)digits;   // every accuracy mode runs the same launch geometry
  const PlanT p = make_plan_t(*k, real, Nt, Ns);
  if (src_per_lane) *src_per_lane = kTTvalues[p.t_idx];
  if (splits) *splits = p.splits;
  if (workspace_bytes) *workspace_bytes = p.workspace_bytes;
  return SCTL_AMD_OK;
}

// ---- several weight vectors through the transposed sum: g_src[m] += A^T w_trg[m] ------------------------------------------------------------
// nd == 1 goes through the single transposed entry (bit-identical results); nd == 0 is a no-op after the argument checks.
int sctl_amd_eval_transpose_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                             const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_transpose_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_transpose_device(kernel, real, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes, stream);
  if (device_count_quiet() <= 0) return no_device();
  return eval_transpose_densities_device(*k, real, nd, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_transpose_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* vectors_per_pass, int* passes,
                                           int* src_per_lane, int* splits, int64_t* workgroups, int64_t* workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of weight vectors");
  if (!has_transpose(*k)) return no_transpose(*k);
  (void)digits;   // every accuracy mode runs the same launch geometry
  int vpp = 0, np = 0, t = 0, s = 0;
  int64_t wg = 0, ws = 0;
  const MultiTEntry* me = multi_entry<RowsTrans>(k->id);
  if (nd == 1 || (nd > 1 && !me)) {   // the single transposed plan, once per weight vector
    const PlanT p = make_plan_t(*k, real, Nt, Ns);
    const int64_t group = (int64_t)kBlock * kTTvalues[p.t_idx];
    vpp = 1; np = nd; t = kTTvalues[p.t_idx]; s = p.splits; ws = p.workspace_bytes;
    for (int64_t s0 = 0; s0 < Ns; s0 += p.owners_per_launch) {
      const int64_t n = (Ns - s0 < p.owners_per_launch) ? Ns - s0 : p.owners_per_launch;
      wg += (n + group - 1) / group * p.splits;
    }
  } else if (nd > 1) {
    rows_passes_plan(*k, *me, real, nd, Nt, Ns, &vpp, &np, &t, &s, &wg, &ws);
  }
  if (vectors_per_pass) *vectors_per_pass = vpp;
  if (passes) *passes = np;
  if (src_per_lane) *src_per_lane = t;
  if (splits) *splits = s;
  if (workgroups) *workgroups = wg;
  if (workspace_bytes) *workspace_bytes = ws;
  return SCTL_AMD_OK;
}

// ---- gradients of <w_trg, A v_src> with respect to the geometry ------------------------------------------------------------------------
int sctl_amd_eval_grad_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                              const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_grad(k, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_nrm, ctx_bytes, ctx);
  if (rc) return rc;
  if (device_count_quiet() <= 0) return no_device();
  return eval_grad_device(*k, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_grad_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* trg_per_lane, int* trg_splits, int64_t* trg_workspace_bytes,
                            int* src_per_lane, int* src_splits, int64_t* src_workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (!has_grad(*k)) return no_grad(*k);
  (void)digits;   // every accuracy mode runs the same launch geometry
  const PlanOwned pt = make_plan_g(*k, real, 0, Nt, Ns), ps = make_plan_g(*k, real, 1, Nt, Ns);
  if (trg_per_lane) *trg_per_lane = k->grad_t[0];
  if (trg_splits) *trg_splits = pt.splits;
  if (trg_workspace_bytes) *trg_workspace_bytes = pt.workspace_bytes;
  if (src_per_lane) *src_per_lane = k->grad_t[1];
  if (src_splits) *src_splits = ps.splits;
  if (src_workspace_bytes) *src_workspace_bytes = ps.workspace_bytes;
  return SCTL_AMD_OK;
}

// ---- the tangent of v_trg = A v_src along a perturbation of the geometry ----------------------------------------------------------------------
int sctl_amd_eval_jvp_device(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                             const void* d_trg, const void* d_src, const void* d_nrm, void* dv_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_jvp(k, real, Nt, Ns, r_trg, r_src, n_src, v_src, d_nrm, dv_trg, ctx_bytes, ctx);
  if (rc) return rc;
  if (device_count_quiet() <= 0) return no_device();
  return eval_jvp_device(*k, real, Nt, Ns, r_trg, r_src, n_src, v_src, d_trg, d_src, d_nrm, dv_trg, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_jvp_plan(int kernel, int real, int64_t Nt, int64_t Ns, int digits, int* trg_per_lane, int* splits, int64_t* workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  const JvpEntry* je = jvp_entry(k->id);
  if (!je) return no_jvp(*k);
  (void)digits;   // every accuracy mode runs the same launch geometry
  const PlanOwned p = make_plan_j(*k, *je, real, Nt, Ns);
  if (trg_per_lane) *trg_per_lane = je->t;
  if (splits) *splits = p.splits;
  if (workspace_bytes) *workspace_bytes = p.workspace_bytes;
  return SCTL_AMD_OK;
}

// ---- the same for several density / weight rows: the gradients of sum_m <w_trg[m], A v_src[m]> -------------------------------------------------
// nd == 1 goes through the single gradient entry (bit-identical results); nd == 0 is a no-op after the argument checks.
int sctl_amd_eval_grad_densities_device(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                        const void* v_src, const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes,
                                        void* stream) {
  const KernelEntry* k = registry(kernel);
  const int rc = check_grad_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_nrm, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_grad_device(kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits, ctx, ctx_bytes, stream);
  if (device_count_quiet() <= 0) return no_device();
  return eval_grad_densities_device(*k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits, ctx, (hipStream_t)stream);
}

int sctl_amd_eval_grad_densities_plan(int kernel, int real, int nd, int64_t Nt, int64_t Ns, int digits, int* rows_per_pass, int* passes, int* trg_splits,
                                      int64_t* trg_workspace_bytes, int* src_splits, int64_t* src_workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of density and weight rows");
  if (!has_grad(*k)) return no_grad(*k);
  (void)digits;   // every accuracy mode runs the same launch geometry
  int rpp = 0, np = 0, s[2] = {0, 0};
  int64_t ws[2] = {0, 0};
  const MultiGEntry* me = multi_g_entry(k->id);
  if (nd == 1 || (nd > 1 && !me)) {   // the single gradient plan, once per row
    rpp = 1; np = nd;
    for (int side = 0; side < 2; side++) {
      const PlanOwned p = make_plan_g(*k, real, side, Nt, Ns);
      s[side] = p.splits; ws[side] = p.workspace_bytes;
    }
  } else if (nd > 1) {
    // the first pass is the widest; the workspace is the largest any pass asks for
    for (int m0 = 0; m0 < nd;) {
      const int left = nd - m0, M = kMultiGM[multi_g_form(*me, left)];
      for (int side = 0; side < 2; side++) {
        const PlanOwned p = make_plan_gm(*k, M, real, side, Nt, Ns);
        if (np == 0) s[side] = p.splits;
        ws[side] = p.workspace_bytes > ws[side] ? p.workspace_bytes : ws[side];
      }
      if (np == 0) rpp = M;
      np++;
      m0 += left < M ? left : M;
    }
  }
  if (rows_per_pass) *rows_per_pass = rpp;
  if (passes) *passes = np;
  if (trg_splits) *trg_splits = s[0];
  if (trg_workspace_bytes) *trg_workspace_bytes = ws[0];
  if (src_splits) *src_splits = s[1];
  if (src_workspace_bytes) *src_workspace_bytes = ws[1];
  return SCTL_AMD_OK;
}

void sctl_amd_counters(int64_t* pair_interactions, int64_t* sctl_flops) {
  if (pair_interactions) *pair_interactions = g_pairs.load();
  if (sctl_flops) *sctl_flops = g_flops.load();
}
void sctl_amd_reset_counters(void) { g_pairs = 0; g_flops = 0; }
void sctl_amd_trim(void) {
  op_cache_trim();            // operators the host-buffer entry over a device list keeps between calls
  workspace_release_all();
}
int sctl_amd_set_debug(int flags) {
  static std::atomic<int> cur{0};
  workspace_poison((flags & SCTL_AMD_DEBUG_POISON_SCRATCH) != 0);
  return cur.exchange(flags);
}

int sctl_amd_eval_plan(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, int digits, int* trg_per_lane, int* src_splits,
                       int64_t* workgroups, int64_t* workspace_bytes) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, Nt, Ns)) return rc;
  if (use_centered(*k, real, Nt, Ns, Nt_whole, false, mode_for(real, digits))) {
    int T, splits;
    int64_t chunk;
    centered_plan(Nt, Ns, cu_count(), (int)real_size(real) * (3 + k->nd + k->k0), (int)real_size(real) * k->k1, &T, &splits, &chunk);
    const int64_t per_wave = centered_targets_per_wave(k->id, real, mode_for(real, digits), Nt > Nt_whole ? Nt : Nt_whole);   // (centered.hip)
    (void)T;
    if (trg_per_lane) *trg_per_lane = (int)(per_wave / 64);
    if (src_splits) *src_splits = splits;
    if (workgroups) *workgroups = ((Nt + per_wave - 1) / per_wave) * splits;   // one wave64 per workgroup
    if (workspace_bytes) *workspace_bytes = (splits > 1) ? (int64_t)splits * Nt * k->k1 * (int)real_size(real) : 0;
    return SCTL_AMD_OK;
  }
  const Plan p = make_plan(*k, real, Nt, Ns);
  if (trg_per_lane) *trg_per_lane = kTvalues[p.t_idx];
  if (src_splits) *src_splits = p.splits;
  if (workgroups) *workgroups = p.wg_x * p.splits;
  if (workspace_bytes) *workspace_bytes = p.workspace_bytes;
  return SCTL_AMD_OK;
}

int sctl_amd_eval_path(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, 0, 0)) return rc;
  return use_centered(*k, real, Nt, Ns, Nt_whole) ? 1 : 0;
}

int sctl_amd_eval_pipe(int kernel, int real, int64_t Nt, int64_t Ns, int64_t Nt_whole, int digits) {
  const int path = sctl_amd_eval_path(kernel, real, Nt, Ns, Nt_whole);
  if (path < 0) return path;
  const KernelEntry* k = registry(kernel);
  if (!use_centered(*k, real, Nt, Ns, Nt_whole, false, mode_for(real, digits))) return 0;   // (a kernel may have its tile-centred form at some accuracies only)
  return centered_pipe(k->id, real, mode_for(real, digits));
}

}  // extern "C"
