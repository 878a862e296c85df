// The device-resident operator (sctl_amd_op_*): geometry, weights, normals and an attached near field kept on one or several devices between
// evaluations; its forward and transposed evaluation, the rank-parallel form, and the cache of operators that the host-buffer entry over a device list
// keeps between calls.
#include "eval_drivers.hpp"
#include "workspace.hpp"

#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace sctl_amd {
// comm.hip
int comm_gather_to_device(sctl_amd_comm* c, const void* local, int64_t nbytes, void** dbuf, size_t* dcap, std::vector<int64_t>* bytes_of_rank,
                          char* (*stage_take)(void*, size_t), void* stage, hipStream_t st);
namespace {
struct OpDevice {
  int device = 0;
  hipStream_t st = nullptr;
  int64_t t0 = 0, t1 = 0;                 // target slab of this device
  void *xt = nullptr, *xs = nullptr, *xn = nullptr, *f = nullptr, *v = nullptr;
  size_t cap_xt = 0, cap_xs = 0, cap_xn = 0, cap_f = 0, cap_v = 0;
  void *w = nullptr, *nt = nullptr, *u = nullptr;   // source weights, target normals (this slab), contracted potential
  size_t cap_w = 0, cap_nt = 0, cap_u = 0;
  void *m_x = nullptr, *m_sorted = nullptr, *m_perm = nullptr;   // first device only: all targets, their Morton order (sctl_amd_op_set_targets)
  size_t cap_m_x = 0, cap_m_sorted = 0, cap_m_perm = 0;
  PinnedBuf stage;                        // pinned staging for uploads and for the slab of the potential
};

hipError_t grow(void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return hipSuccess;
  if (*p) { hipError_t e = hipFree(*p); if (e != hipSuccess) return e; *p = nullptr; *cap = 0; }
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) *cap = bytes;
  return e;
}
}  // namespace
}  // namespace sctl_amd

struct sctl_amd_op {
  const sctl_amd::KernelEntry* k = nullptr;
  int real = 0;
  int64_t Nt = 0, Ns = 0;
  std::vector<sctl_amd::OpDevice> devs;
  // several devices: the slabs are cut from the Morton order of the targets, so that a device's targets keep the
  // density of the whole set (what the tile-centred path needs); perm[i] = caller's index of sorted target i
  std::vector<int64_t> perm;
  bool have_weights = false, have_trg_normals = false;   // far-field pre/post steps on the device (sctl_amd_op_set_source_weights / _target_normals)
  // BoundaryIntegralOp near field attached to this operator (sctl_amd_op_set_near): one sub-operator per device, holding the columns
  // (near targets) of every element block that fall into that device's target slab, so far + near are added ON the device
  std::vector<sctl_amd_near*> near;
  std::vector<void*> near_f;      // device copy of the near density (element nodes x SrcDim), one per device
  std::vector<size_t> near_f_cap; // its bytes: one density after set_near, nd of them after a several-densities evaluation
  int64_t near_f_len = 0;
  int near_trg_dim = 0;
};

namespace sctl_amd {
namespace {

int op_for_each_device(sctl_amd_op* op, const std::function<int(OpDevice&)>& fn) {
  const int n = (int)op->devs.size();
  if (n == 1) return fn(op->devs[0]);
  std::vector<int> rcs(n, SCTL_AMD_OK);
  std::vector<std::string> msgs(n);
  std::vector<std::thread> th;
  for (int g = 0; g < n; g++) th.emplace_back([&, g] { rcs[g] = fn(op->devs[g]); if (rcs[g]) msgs[g] = error_text(); });
  for (auto& t : th) t.join();
  for (int g = 0; g < n; g++)
    if (rcs[g]) return fail(rcs[g], "device " + std::to_string(op->devs[g].device) + ": " + msgs[g]);
  return SCTL_AMD_OK;
}
}  // namespace
}  // namespace sctl_amd

// ---- operators kept between calls of the host-buffer entry over a device list --------------------------------------------------------
// A small process-wide pool keyed by (kernel, precision, device list).  A call takes a free operator with its key (or creates one; two
// threads with the same key get two), uses it and hands it back; at most kOpCacheMax stay (the least recently used free one goes when a
// new one is kept), sctl_amd_trim() destroys the free ones, and an operator whose call failed is destroyed rather than kept.  Like the
// other process-lifetime state of this library the pool is never torn down at exit (the HIP runtime may already be gone by then).
namespace sctl_amd {
namespace {
constexpr size_t kOpCacheMax = 8;
struct CachedOp { int kernel, real; std::vector<int> devs; sctl_amd_op* op; bool busy; uint64_t stamp; };
struct OpCache { std::mutex mu; std::vector<CachedOp> ops; uint64_t clock = 0; };
OpCache& op_cache() { static OpCache* c = new OpCache; return *c; }
}  // namespace
int op_cache_acquire(int kernel, int real, const std::vector<int>& devs, sctl_amd_op** out) {
  OpCache& c = op_cache();
  {
    std::lock_guard<std::mutex> lock(c.mu);
    for (CachedOp& e : c.ops)
      if (!e.busy && e.kernel == kernel && e.real == real && e.devs == devs) { e.busy = true; e.stamp = ++c.clock; *out = e.op; return SCTL_AMD_OK; }
  }
  sctl_amd_op* op = nullptr;
  const int rc = sctl_amd_op_create(kernel, real, devs.data(), (int)devs.size(), &op);
  if (rc != SCTL_AMD_OK) return rc;
  sctl_amd_op* evict = nullptr;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    if (c.ops.size() >= kOpCacheMax) {   // make room: the least recently used FREE operator goes (all busy: this one is simply not kept)
      size_t lru = c.ops.size();
      for (size_t i = 0; i < c.ops.size(); i++)
        if (!c.ops[i].busy && (lru == c.ops.size() || c.ops[i].stamp < c.ops[lru].stamp)) lru = i;
      if (lru < c.ops.size()) { evict = c.ops[lru].op; c.ops.erase(c.ops.begin() + (long)lru); }
    }
    if (c.ops.size() < kOpCacheMax) c.ops.push_back(CachedOp{kernel, real, devs, op, true, ++c.clock});
  }
  if (evict) sctl_amd_op_destroy(evict);
  *out = op;
  return SCTL_AMD_OK;
}
void op_cache_release(sctl_amd_op* op, bool failed) {
  if (!op) return;
  OpCache& c = op_cache();
  bool kept = false;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    for (size_t i = 0; i < c.ops.size(); i++)
      if (c.ops[i].op == op) {
        if (failed) c.ops.erase(c.ops.begin() + (long)i);
        else { c.ops[i].busy = false; kept = true; }
        break;
      }
  }
  if (!kept) sctl_amd_op_destroy(op);
}
void op_cache_trim() {
  OpCache& c = op_cache();
  std::vector<sctl_amd_op*> gone;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    for (size_t i = c.ops.size(); i-- > 0;)
      if (!c.ops[i].busy) { gone.push_back(c.ops[i].op); c.ops.erase(c.ops.begin() + (long)i); }
  }
  for (sctl_amd_op* op : gone) sctl_amd_op_destroy(op);
}
}  // namespace sctl_amd

using namespace sctl_amd;

extern "C" {

int sctl_amd_op_create(int kernel, int real, const int* devices, int n_devices, sctl_amd_op** out) {
  const KernelEntry* k = registry(kernel);
  if (const int rc = check_real_sizes(k, real, 0, 0)) return rc;
  if (!out || n_devices <= 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle pointer or no devices");
  const int avail = device_count_quiet();
  if (avail <= 0) return no_device();
  RestoreDevice restore;
  sctl_amd_op* op = new sctl_amd_op;
  op->k = k; op->real = real;
  op->devs.resize(n_devices);
  for (int g = 0; g < n_devices; g++) {
    OpDevice& d = op->devs[g];
    d.device = devices ? devices[g] : g;
    if (d.device < 0 || d.device >= avail) { sctl_amd_op_destroy(op); return fail(SCTL_AMD_ERR_NO_DEVICE, "device index out of range"); }
    if (hipSetDevice(d.device) != hipSuccess || hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) {
      sctl_amd_op_destroy(op);
      return fail(SCTL_AMD_ERR_HIP, "cannot create a stream on device " + std::to_string(d.device));
    }
  }
  *out = op;
  return SCTL_AMD_OK;
}

static void op_release_near(sctl_amd_op* op);
void sctl_amd_op_destroy(sctl_amd_op* op) {
  if (!op) return;
  op_release_near(op);
  RestoreDevice restore;
  const int avail = device_count_quiet();
  for (OpDevice& d : op->devs) {
    if (d.device < 0 || d.device >= avail || !d.st) continue;   // never initialised (create failed on this entry)
    if (hipSetDevice(d.device) != hipSuccess) { (void)hipGetLastError(); continue; }
    for (void* p : {d.xt, d.xs, d.xn, d.f, d.v, d.w, d.nt, d.u, d.m_x, d.m_sorted, d.m_perm})
      if (p) (void)hipFree(p);
    if (d.st) { workspace_forget(d.st); (void)hipStreamDestroy(d.st); }
  }
  delete op;
}

int sctl_amd_op_set_targets(sctl_amd_op* op, int64_t Nt, const void* r_trg) {
  if (!op || Nt < 0 || (Nt > 0 && !r_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "bad target arguments");
  const size_t rs = real_size(op->real);
  const int G = (int)op->devs.size();
  op->Nt = Nt;
  op->have_trg_normals = false;   // normals belong to a target set: set them again after new targets
  op_release_near(op);            // and so does an attached near-field operator (its columns are target slabs)
  int g = 0;
  for (OpDevice& d : op->devs) { d.t0 = Nt * g / G; d.t1 = Nt * (g + 1) / G; g++; }   // fmm-wrapper.txx:507
  // several devices, or a kernel with a tile-centred path: the targets are kept in Morton order (coordinates gathered into sorted
  // order once, here), so that slabs are compact and an evaluation needs no sort of its own
  std::vector<char> sorted;
  op->perm.clear();
  if ((G > 1 || (has_centered_path(*op->k, op->real) && Nt >= kPresortMinTargets)) && Nt > 0) {
    // The order is computed on the FIRST device (upload all targets, bbox -> keys -> radix sort -> gather, download order and sorted
    // coordinates): ~10 ms at 2^20 points, where the host sort this replaces (round 3) took 70-90 ms on one core — more than a GPU's whole
    // share of a 2^20 x 2^20 evaluation on an 8-GPU node, and paid per call by the host-buffer entry over a device list.
    if (Nt > 0xfffffff0ll) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "more than 2^32 targets in one operator");
    OpDevice& d0 = op->devs[0];
    const size_t xbytes = (size_t)Nt * 3 * rs, pbytes = (size_t)Nt * sizeof(uint32_t);
    DeviceScope scope0(d0.device);
    HIP_TRY(scope0.err);
    HIP_TRY(grow(&d0.m_x, &d0.cap_m_x, xbytes));
    HIP_TRY(grow(&d0.m_sorted, &d0.cap_m_sorted, xbytes));
    HIP_TRY(grow(&d0.m_perm, &d0.cap_m_perm, pbytes));
    HIP_TRY(d0.stage.reserve(pad256(xbytes) + pad256(pbytes)));
    HIP_TRY(upload(d0.m_x, r_trg, xbytes, d0.stage, d0.st));
    HIP_TRY(morton_order_device(op->real, d0.m_x, Nt, d0.m_sorted, (uint32_t*)d0.m_perm, d0.st));
    HIP_TRY(hipStreamSynchronize(d0.st));       // the upload's staging slice is free again
    d0.stage.used = 0;
    char* hs = d0.stage.take(xbytes);
    char* hp = d0.stage.take(pbytes);
    HIP_TRY(hipMemcpyAsync(hs, d0.m_sorted, xbytes, hipMemcpyDeviceToHost, d0.st));
    HIP_TRY(hipMemcpyAsync(hp, d0.m_perm, pbytes, hipMemcpyDeviceToHost, d0.st));
    HIP_TRY(hipStreamSynchronize(d0.st));
    sorted.assign(hs, hs + xbytes);
    op->perm.resize((size_t)Nt);
    const uint32_t* p32 = (const uint32_t*)hp;
    for (int64_t i = 0; i < Nt; i++) op->perm[(size_t)i] = (int64_t)p32[i];
    d0.stage.used = 0;
  }
  const char* src = sorted.empty() ? (const char*)r_trg : sorted.data();
  return op_for_each_device(op, [&](OpDevice& d) -> int {
    const size_t bytes = (size_t)(d.t1 - d.t0) * 3 * rs;
    DeviceScope dev_scope_4(d.device);
    HIP_TRY(dev_scope_4.err);
    HIP_TRY(grow(&d.xt, &d.cap_xt, bytes));
    HIP_TRY(d.stage.reserve(pad256(bytes)));
    HIP_TRY(upload(d.xt, src + (size_t)d.t0 * 3 * rs, bytes, d.stage, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    return SCTL_AMD_OK;
  });
}

int sctl_amd_op_set_sources(sctl_amd_op* op, int64_t Ns, const void* r_src, const void* n_src) {
  if (!op || Ns < 0 || (Ns > 0 && !r_src)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "bad source arguments");
  if (Ns > 0 && op->k->nd > 0 && !n_src) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(op->k->name) + " needs source normals (n_src is null)");
  const size_t rs = real_size(op->real);
  op->Ns = Ns;
  op->have_weights = false;       // weights belong to a source set
  return op_for_each_device(op, [&](OpDevice& d) -> int {
    DeviceScope dev_scope_5(d.device);
    HIP_TRY(dev_scope_5.err);
    HIP_TRY(grow(&d.xs, &d.cap_xs, (size_t)Ns * 3 * rs));
    HIP_TRY(grow(&d.xn, &d.cap_xn, (size_t)Ns * op->k->nd * rs));
    HIP_TRY(d.stage.reserve(pad256((size_t)Ns * 3 * rs) + pad256((size_t)Ns * op->k->nd * rs)));
    HIP_TRY(upload(d.xs, r_src, (size_t)Ns * 3 * rs, d.stage, d.st));
    if (op->k->nd) HIP_TRY(upload(d.xn, n_src, (size_t)Ns * op->k->nd * rs, d.stage, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    return SCTL_AMD_OK;
  });
}

int sctl_amd_op_set_source_weights(sctl_amd_op* op, const void* wts) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!wts) { op->have_weights = false; return SCTL_AMD_OK; }
  const size_t rs = real_size(op->real);
  const int64_t Ns = op->Ns;
  const int rc = op_for_each_device(op, [&](OpDevice& d) -> int {
    DeviceScope dev_scope_6(d.device);
    HIP_TRY(dev_scope_6.err);
    HIP_TRY(grow(&d.w, &d.cap_w, (size_t)Ns * rs));
    HIP_TRY(d.stage.reserve(pad256((size_t)Ns * rs)));
    HIP_TRY(upload(d.w, wts, (size_t)Ns * rs, d.stage, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    return SCTL_AMD_OK;
  });
  op->have_weights = (rc == SCTL_AMD_OK);
  return rc;
}

int sctl_amd_op_set_target_normals(sctl_amd_op* op, const void* n_trg) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!n_trg) { op->have_trg_normals = false; return SCTL_AMD_OK; }
  if (op->k->k1 % 3 != 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(op->k->name) + ": TrgDim is not a multiple of 3, nothing to contract with a normal");
  const size_t rs = real_size(op->real);
  std::vector<char> sorted;   // several devices: the targets live in Morton order
  if (!op->perm.empty()) {
    sorted.resize((size_t)op->Nt * 3 * rs);
    for (int64_t i = 0; i < op->Nt; i++) std::memcpy(&sorted[(size_t)i * 3 * rs], (const char*)n_trg + (size_t)op->perm[(size_t)i] * 3 * rs, 3 * rs);
  }
  const char* src = sorted.empty() ? (const char*)n_trg : sorted.data();
  const int rc = op_for_each_device(op, [&](OpDevice& d) -> int {
    const size_t bytes = (size_t)(d.t1 - d.t0) * 3 * rs;
    DeviceScope dev_scope_7(d.device);
    HIP_TRY(dev_scope_7.err);
    HIP_TRY(grow(&d.nt, &d.cap_nt, bytes));
    HIP_TRY(d.stage.reserve(pad256(bytes)));
    HIP_TRY(upload(d.nt, src + (size_t)d.t0 * 3 * rs, bytes, d.stage, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    return SCTL_AMD_OK;
  });
  op->have_trg_normals = (rc == SCTL_AMD_OK);
  return rc;
}

}  // extern "C"

namespace {
// the checks of an evaluation that adds the attached near field
int check_near_attached(const sctl_amd_op* op) {
  if (op->near.empty()) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "no near-field operator attached: call sctl_amd_op_set_near first");
  if (op->near_trg_dim != (op->have_trg_normals ? op->k->k1 / 3 : op->k->k1))
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "the attached near-field operator has another potential dimension than the far field delivers");
  return SCTL_AMD_OK;
}
// An operator without element nodes still takes the near path (which then adds nothing): a near density that is not null
const void* near_density(const sctl_amd_op* op, const void* f_near) {
  static const char nothing = 0;
  return op->near_f_len == 0 ? (const void*)&nothing : f_near;
}
// the argument checks of the single-density evaluations, in their order.  comm != nullptr: v_src is this rank's share of ns_local sources.
int check_op_eval(const sctl_amd_op* op, const void* v_src, const void* f_near, const void* v_trg, const void* ctx, int ctx_bytes, sctl_amd_comm* comm = nullptr,
                  int64_t ns_local = 0) {
  int rc = f_near ? check_near_attached(op) : SCTL_AMD_OK;
  if (rc == SCTL_AMD_OK) rc = check_ctx(*op->k, ctx, ctx_bytes);
  if (rc) return rc;
  if ((!comm && op->Ns > 0 && !v_src) || (comm && ns_local > 0 && !v_src) || (op->Nt > 0 && !v_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  return SCTL_AMD_OK;
}

// Far field (+ the attached near field when f_near != nullptr) of nd >= 1 densities, density-major, all rows of the potential back to the host once: the
// per-device body of every forward evaluation (arguments checked by the callers).  One density takes the single-density driver and near apply, several
// take the several-densities forms: that is what keeps nd == 1 bit-identical to the single-density entries.
// comm != nullptr (nd == 1 only): v_src is this rank's share of the density; all ranks' shares are gathered on the device (rank order).
int op_eval_body(sctl_amd_op* op, int nd, const void* v_src, const void* f_near, void* v_trg, int accumulate, int digits, const void* ctx,
                 sctl_amd_comm* comm = nullptr, int64_t ns_local = 0) {
  const KernelEntry& k = *op->k;
  const int real = op->real;
  const size_t rs = real_size(real);
  const int64_t Ns = op->Ns, Nt = op->Nt;
  const size_t near_bytes = f_near ? (size_t)nd * op->near_f_len * rs : 0;
  const int k1 = op->have_trg_normals ? k.k1 / 3 : k.k1;   // components per target that go back to the host
  return op_for_each_device(op, [&](OpDevice& d) -> int {
    const int64_t nt = d.t1 - d.t0;
    if (nt == 0 && !comm) return SCTL_AMD_OK;      // (a rank without targets still takes part in the gather)
    const size_t g = (size_t)(&d - op->devs.data());
    const size_t fbytes = (size_t)nd * Ns * k.k0 * rs, vbytes = (size_t)nd * nt * k.k1 * rs, obytes = (size_t)nd * nt * k1 * rs;
    DeviceScope dev_scope(d.device);
    auto reserve = [&]() -> int {
      HIP_TRY(dev_scope.err);
      HIP_TRY(grow(&d.f, &d.cap_f, fbytes));
      HIP_TRY(grow(&d.v, &d.cap_v, vbytes));
      return SCTL_AMD_OK;
    };
    const int reserve_rc = comm ? comm_agree(comm, reserve(), "sctl_amd_op_eval_dist") : reserve();
    if (reserve_rc) return reserve_rc;
    if (comm) {   // every rank's density into d.f, in the rank order the sources were gathered in
      std::vector<int64_t> got;
      const int rc = comm_gather_to_device(comm, v_src, ns_local * k.k0 * (int64_t)rs, &d.f, &d.cap_f, &got, &PinnedBuf::reserve_and_take, &d.stage, d.st);
      if (rc) return rc;
      int64_t tot = 0;
      for (int64_t b : got) tot += b;
      if (tot != Ns * k.k0 * (int64_t)rs) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "the ranks' densities do not match the sources gathered by sctl_amd_op_set_sources_dist");
      HIP_TRY(hipStreamSynchronize(d.st));   // the staging slice is reused below
      if (nt == 0) return SCTL_AMD_OK;       // took part in the gather; owns no targets
    }
    HIP_TRY(d.stage.reserve(pad256(comm ? 0 : fbytes) + pad256(near_bytes) + pad256(nd == 1 ? vbytes : obytes)));
    if (!comm) HIP_TRY(upload(d.f, v_src, fbytes, d.stage, d.st));
    if (near_bytes) {   // (one density fits what sctl_amd_op_set_near allocated)
      HIP_TRY(grow(&op->near_f[g], &op->near_f_cap[g], near_bytes));
      HIP_TRY(upload(op->near_f[g], f_near, near_bytes, d.stage, d.st));
    }
    if (op->have_weights && Ns > 0) {   // every density x the quadrature weights (boundary_integral.txx:1040-1052)
      scale_density(real, d.f, d.w, Ns, k.k0, nd, d.st);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(d.v, 0, vbytes, d.st));
    const int64_t nt_whole = op->perm.empty() ? 0 : Nt;
    int rc = SCTL_AMD_OK;
    if (Ns == 0) {}           // no far-field sources: the potential is the near field alone
    else if (nd == 1) rc = eval_device(k, real, nt, Ns, d.xt, d.xs, d.xn, d.f, d.v, digits, ctx, d.st, nt_whole, !op->perm.empty());
    else rc = eval_densities_device(k, real, nd, nt, Ns, d.xt, d.xs, d.xn, d.f, d.v, digits, ctx, d.st, nt_whole, !op->perm.empty());
    if (rc) return rc;
    void* result = d.v;
    if (op->have_trg_normals) {   // contract each density's last index with the target normal (boundary_integral.txx:1060-1071): 3x less D2H
      HIP_TRY(grow(&d.u, &d.cap_u, obytes));
      normal_dot(real, d.v, d.nt, d.u, nt, k1, nd, d.st);
      HIP_TRY(hipGetLastError());
      result = d.u;
    }
    if (f_near && op->near[g]) {   // the near-zone correction of this slab's targets, every row added where its far field lies (boundary_integral.txx:608-614)
      rc = nd == 1 ? sctl_amd_near_apply_device(op->near[g], op->near_f[g], result, d.st)
                   : sctl_amd_near_apply_densities_device(op->near[g], nd, op->near_f[g], result, d.st);
      if (rc) return rc;
    }
    const char* out = d.stage.take(obytes);
    HIP_TRY(hipMemcpyAsync((void*)out, result, obytes, hipMemcpyDeviceToHost, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    // this slab of every density row, into the caller's target order (Morton slab -> perm when the targets are kept sorted)
    scatter_slab(real, v_trg, out, nd, Nt, nt, d.t0, k1, op->perm.empty() ? nullptr : op->perm.data() + d.t0, accumulate != 0);
    return SCTL_AMD_OK;
  });
}
}  // namespace

extern "C" {

int sctl_amd_op_eval(sctl_amd_op* op, const void* v_src, void* v_trg, int accumulate, int digits, const void* ctx, int ctx_bytes) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  const int rc = check_op_eval(op, v_src, nullptr, v_trg, ctx, ctx_bytes);
  return rc ? rc : op_eval_body(op, 1, v_src, nullptr, v_trg, accumulate, digits, ctx);
}

int sctl_amd_op_eval_potential(sctl_amd_op* op, const void* v_src_far, const void* f_near, void* v_trg, int accumulate, int digits, const void* ctx,
                               int ctx_bytes) {
  if (op && op->near_f_len > 0 && !f_near) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field density");
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  f_near = near_density(op, f_near);
  const int rc = check_op_eval(op, v_src_far, f_near, v_trg, ctx, ctx_bytes);
  return rc ? rc : op_eval_body(op, 1, v_src_far, f_near, v_trg, accumulate, digits, ctx);
}

// nd == 1 goes through the single-density entry; nd == 0 is a no-op after the argument checks.
int sctl_amd_op_eval_densities(sctl_amd_op* op, int nd, const void* v_src, void* v_trg, int accumulate, int digits, const void* ctx, int ctx_bytes) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  const int rc = check_ctx(*op->k, ctx, ctx_bytes);
  if (rc) return rc;
  if (nd > 0 && ((op->Ns > 0 && !v_src) || (op->Nt > 0 && !v_trg))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  if (nd == 0) return SCTL_AMD_OK;
  if (nd == 1) return sctl_amd_op_eval(op, v_src, v_trg, accumulate, digits, ctx, ctx_bytes);
  return op_eval_body(op, nd, v_src, nullptr, v_trg, accumulate, digits, ctx);
}

int sctl_amd_op_eval_potential_densities(sctl_amd_op* op, int nd, const void* v_src_far, const void* f_near, void* v_trg, int accumulate, int digits,
                                         const void* ctx, int ctx_bytes) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  int rc = check_near_attached(op);
  if (rc == SCTL_AMD_OK) rc = check_ctx(*op->k, ctx, ctx_bytes);
  if (rc) return rc;
  if (nd > 0 && ((op->Ns > 0 && !v_src_far) || (op->Nt > 0 && !v_trg))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  if (nd > 0 && op->near_f_len > 0 && !f_near) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null near-field density");
  if (nd == 0) return SCTL_AMD_OK;
  if (nd == 1) return sctl_amd_op_eval_potential(op, v_src_far, f_near, v_trg, accumulate, digits, ctx, ctx_bytes);
  return op_eval_body(op, nd, v_src_far, near_density(op, f_near), v_trg, accumulate, digits, ctx);
}
// ---- rank-parallel form: every rank owns some targets and some sources (ParticleFMM::EvalDirect under MPI, fmm-wrapper.txx:504-561) ----
int sctl_amd_op_set_sources_dist(sctl_amd_op* op, sctl_amd_comm* comm, int64_t Ns_local, const void* r_src, const void* n_src) {
  if (!op || !comm) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle or communicator");
  const size_t rs = real_size(op->real);
  OpDevice& d = op->devs[0];
  DeviceScope scope(d.device);
  auto check_arguments = [&]() -> int {
    if (Ns_local < 0 || (Ns_local > 0 && !r_src)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "bad source arguments");
    if (op->devs.size() != 1) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "a rank-parallel operator lives on ONE device per rank");
    if (Ns_local > 0 && op->k->nd > 0 && !n_src) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(op->k->name) + " needs source normals (n_src is null)");
    HIP_TRY(scope.err);
    return SCTL_AMD_OK;
  };
  const int arg_rc = comm_agree(comm, check_arguments(), "sctl_amd_op_set_sources_dist");   // all ranks, before the first collective
  if (arg_rc) return arg_rc;
  op->have_weights = false;
  std::vector<int64_t> got, gotn;
  int rc = comm_gather_to_device(comm, r_src, Ns_local * 3 * (int64_t)rs, &d.xs, &d.cap_xs, &got, &PinnedBuf::reserve_and_take, &d.stage, d.st);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(d.st));
  int64_t tot = 0;
  for (int64_t b : got) tot += b;
  op->Ns = tot / (3 * (int64_t)rs);
  if (op->k->nd) {
    rc = comm_gather_to_device(comm, n_src, Ns_local * op->k->nd * (int64_t)rs, &d.xn, &d.cap_xn, &gotn, &PinnedBuf::reserve_and_take, &d.stage, d.st);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(d.st));
  }
  return SCTL_AMD_OK;
}

int sctl_amd_op_eval_dist(sctl_amd_op* op, sctl_amd_comm* comm, int64_t Ns_local, const void* v_src_local, void* v_trg, int accumulate, int digits,
                          const void* ctx, int ctx_bytes) {
  if (!op || !comm) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle or communicator");
  const int shape_rc = comm_agree(comm, (Ns_local < 0 || op->devs.size() != 1) ? fail(SCTL_AMD_ERR_BAD_ARGUMENT, "a rank-parallel operator lives on ONE device per rank and takes Ns_local >= 0")
                                                                                : SCTL_AMD_OK, "sctl_amd_op_eval_dist");
  if (shape_rc) return shape_rc;
  // the ranks agree on their argument checks BEFORE the first collective, so that a rank with a bad argument does not leave the others waiting inside
  // the gather (they get SCTL_AMD_ERR_PEER)
  const int arg_rc = comm_agree(comm, check_op_eval(op, v_src_local, nullptr, v_trg, ctx, ctx_bytes, comm, Ns_local), "sctl_amd_op_eval_dist");
  return arg_rc ? arg_rc : op_eval_body(op, 1, v_src_local, nullptr, v_trg, accumulate, digits, ctx, comm, Ns_local);
}
// The adjoint of op_eval_body for nd >= 1 weight vectors, row-major: g_far[m] = D_w A^T C_n^T w[m] and, with_near, g_near[m] = N^T w[m].  Every device
// works on its target slab of every row; the partial results wait in the devices' staging buffers and are added on the host in device order, row by row.
// One row takes the single transposed driver and near apply, several take the several-vectors forms: that keeps nd == 1 bit-identical to what it was.
static int op_eval_transpose_impl(sctl_amd_op* op, int nd, const void* w_trg, void* g_far, void* g_near, bool with_near, int accumulate, int digits,
                                  const void* ctx, int ctx_bytes) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (nd < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of weight vectors");
  const KernelEntry& k = *op->k;
  int rc0 = with_near ? check_near_attached(op) : SCTL_AMD_OK;
  if (rc0 == SCTL_AMD_OK) rc0 = check_ctx(k, ctx, ctx_bytes);
  if (rc0) return rc0;
  if (nd > 0 && ((op->Nt > 0 && !w_trg) || (op->Ns > 0 && !g_far) || (with_near && op->near_f_len > 0 && !g_near)))
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null weight or density-gradient array");
  if (!has_transpose(k)) return no_transpose(k);
  if (nd == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(op->real);
  const int64_t Ns = op->Ns;
  const int k1w = op->have_trg_normals ? k.k1 / 3 : k.k1;   // components of w per target
  const size_t frow = (size_t)Ns * k.k0 * rs, nrow = with_near ? (size_t)op->near_f_len * rs : 0, wrow = (size_t)k1w * rs;
  const size_t fbytes = (size_t)nd * frow, nbytes = (size_t)nd * nrow;
  std::vector<char> sorted;   // every row of w in the operator's own (Morton) target order
  if (!op->perm.empty()) {
    sorted.resize((size_t)nd * op->Nt * wrow);
    for (int m = 0; m < nd; m++)
      for (int64_t i = 0; i < op->Nt; i++)
        std::memcpy(&sorted[((size_t)m * op->Nt + (size_t)i) * wrow], (const char*)w_trg + ((size_t)m * op->Nt + (size_t)op->perm[(size_t)i]) * wrow, wrow);
  }
  const char* wsrc = sorted.empty() ? (const char*)w_trg : sorted.data();
  std::vector<const char*> part_far(op->devs.size(), nullptr), part_near(op->devs.size(), nullptr);
  const int rc_all = op_for_each_device(op, [&](OpDevice& d) -> int {
    const int64_t nt = d.t1 - d.t0;
    if (nt == 0) return SCTL_AMD_OK;
    const size_t g = (size_t)(&d - op->devs.data());
    const size_t wslab = (size_t)nt * wrow, wbytes = (size_t)nd * wslab;
    DeviceScope dev_scope(d.device);
    HIP_TRY(dev_scope.err);
    HIP_TRY(grow(&d.f, &d.cap_f, fbytes));
    HIP_TRY(grow(&d.v, &d.cap_v, (size_t)nd * nt * k.k1 * rs));
    if (op->have_trg_normals) HIP_TRY(grow(&d.u, &d.cap_u, wbytes));
    HIP_TRY(d.stage.reserve(pad256(wbytes) + pad256(fbytes) + pad256(nbytes)));
    void* w_dev = op->have_trg_normals ? d.u : d.v;   // the slab of every row of w as the caller gave it: what the near field takes
    {   // this slab of every row, rows back to back, down once
      char* q = d.stage.take(wbytes);
      for (int m = 0; m < nd; m++) std::memcpy(q + (size_t)m * wslab, wsrc + ((size_t)m * op->Nt + (size_t)d.t0) * wrow, wslab);
      HIP_TRY(hipMemcpyAsync(w_dev, q, wbytes, hipMemcpyHostToDevice, d.st));
    }
    if (op->have_trg_normals) {   // w_full[m][t][k*3+l] = w[m][t][k] n_trg[t][l]: the adjoint of the contraction with the target normal
      normal_expand(op->real, d.u, d.nt, d.v, nt, k1w, nd, d.st);
      HIP_TRY(hipGetLastError());
    }
    if (fbytes) HIP_TRY(hipMemsetAsync(d.f, 0, fbytes, d.st));
    int rc = SCTL_AMD_OK;
    if (Ns == 0) {}
    else if (nd == 1) rc = eval_transpose_device(k, op->real, nt, Ns, d.xt, d.xs, d.xn, d.v, d.f, digits, ctx, d.st);
    else rc = eval_transpose_densities_device(k, op->real, nd, nt, Ns, d.xt, d.xs, d.xn, d.v, d.f, digits, ctx, d.st);
    if (rc) return rc;
    if (op->have_weights && Ns > 0) {   // the adjoint of density x quadrature weights is the same scaling
      scale_density(op->real, d.f, d.w, Ns, k.k0, nd, d.st);
      HIP_TRY(hipGetLastError());
    }
    const bool near_here = nbytes && op->near[g];
    if (near_here) {
      HIP_TRY(grow(&op->near_f[g], &op->near_f_cap[g], nbytes));   // (one row fits what sctl_amd_op_set_near allocated)
      HIP_TRY(hipMemsetAsync(op->near_f[g], 0, nbytes, d.st));
      rc = nd == 1 ? sctl_amd_near_apply_transpose_device(op->near[g], w_dev, op->near_f[g], d.st)
                   : sctl_amd_near_apply_transpose_densities_device(op->near[g], nd, w_dev, op->near_f[g], d.st);
      if (rc) return rc;
    }
    char* out_f = d.stage.take(fbytes);
    if (fbytes) HIP_TRY(hipMemcpyAsync(out_f, d.f, fbytes, hipMemcpyDeviceToHost, d.st));
    char* out_n = d.stage.take(nbytes);
    if (near_here) HIP_TRY(hipMemcpyAsync(out_n, op->near_f[g], nbytes, hipMemcpyDeviceToHost, d.st));
    HIP_TRY(hipStreamSynchronize(d.st));
    part_far[g] = out_f;
    if (near_here) part_near[g] = out_n;
    return SCTL_AMD_OK;
  });
  if (rc_all) return rc_all;
  auto combine = [&](void* out, const std::vector<const char*>& parts, size_t bytes) {   // device order: a fixed order (the rows lie back to back)
    if (!bytes) return;
    if (!accumulate) std::memset(out, 0, bytes);
    for (const char* p : parts)
      if (p) add_into(op->real, out, p, (int64_t)(bytes / rs));
  };
  combine(g_far, part_far, fbytes);
  if (with_near) combine(g_near, part_near, nbytes);
  return SCTL_AMD_OK;
}

int sctl_amd_op_eval_transpose(sctl_amd_op* op, const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes) {
  return op_eval_transpose_impl(op, 1, w_trg, g_src, nullptr, false, accumulate, digits, ctx, ctx_bytes);
}

int sctl_amd_op_eval_potential_transpose(sctl_amd_op* op, const void* w_trg, void* g_src_far, void* g_near, int accumulate, int digits, const void* ctx,
                                         int ctx_bytes) {
  return op_eval_transpose_impl(op, 1, w_trg, g_src_far, g_near, true, accumulate, digits, ctx, ctx_bytes);
}

// nd rows in one pass; nd == 1 is the single entry (op_eval_transpose_impl takes the single drivers for it), nd == 0 a no-op after the argument checks.
int sctl_amd_op_eval_transpose_densities(sctl_amd_op* op, int nd, const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx,
                                         int ctx_bytes) {
  return op_eval_transpose_impl(op, nd, w_trg, g_src, nullptr, false, accumulate, digits, ctx, ctx_bytes);
}

int sctl_amd_op_eval_potential_transpose_densities(sctl_amd_op* op, int nd, const void* w_trg, void* g_src_far, void* g_near, int accumulate, int digits,
                                                   const void* ctx, int ctx_bytes) {
  return op_eval_transpose_impl(op, nd, w_trg, g_src_far, g_near, true, accumulate, digits, ctx, ctx_bytes);
}

static void op_release_near(sctl_amd_op* op) {
  RestoreDevice restore;
  for (size_t g = 0; g < op->near.size(); g++) {
    if (op->near[g]) sctl_amd_near_destroy(op->near[g]);
    if (g < op->near_f.size() && op->near_f[g] && hipSetDevice(op->devs[g].device) == hipSuccess) (void)hipFree(op->near_f[g]);
  }
  op->near.clear();
  op->near_f.clear();
  op->near_f_cap.clear();
  op->near_f_len = 0;
  op->near_trg_dim = 0;
}

int sctl_amd_op_set_near(sctl_amd_op* op, int src_dim, int trg_dim, int64_t Nelem, const int64_t* elem_nds_cnt, const int64_t* near_elem_cnt,
                         const int64_t* K_near_cnt, const void* K_near, const int64_t* near_scatter_index, const int64_t* near_trg_cnt,
                         const int64_t* near_trg_dsp) {
  if (!op) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  op_release_near(op);
  if (Nelem == 0 && !elem_nds_cnt) return SCTL_AMD_OK;   // detach
  if (src_dim != op->k->k0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "near-field operator: src_dim differs from the kernel's SrcDim");
  if (Nelem < 0 || trg_dim < 1 || (Nelem > 0 && (!elem_nds_cnt || !near_elem_cnt)) || (op->Nt > 0 && (!near_trg_cnt || !near_trg_dsp)))
    return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "near-field operator: bad sizes or null count arrays");
  const int64_t Nt = op->Nt;
  const size_t rs = real_size(op->real);
  const int G = (int)op->devs.size();
  // per-element displacements, and for every near entry (element-major) the target it belongs to
  std::vector<int64_t> near_dsp((size_t)Nelem + 1, 0), k_dsp((size_t)Nelem + 1, 0);
  int64_t f_len = 0;
  for (int64_t e = 0; e < Nelem; e++) {
    if (elem_nds_cnt[e] < 0 || near_elem_cnt[e] < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative element count");
    const int64_t kc = K_near_cnt ? K_near_cnt[e] : elem_nds_cnt[e] * near_elem_cnt[e];
    if (kc != 0 && kc != elem_nds_cnt[e] * near_elem_cnt[e]) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "K_near_cnt[e] must be 0 or elem_nds_cnt[e] * near_elem_cnt[e]");
    near_dsp[(size_t)e + 1] = near_dsp[(size_t)e] + near_elem_cnt[e];
    k_dsp[(size_t)e + 1] = k_dsp[(size_t)e] + kc;
    f_len += elem_nds_cnt[e] * src_dim;
  }
  const int64_t n_near = near_dsp[(size_t)Nelem];
  if (n_near > 0 && !near_scatter_index) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null near_scatter_index");
  if (k_dsp[(size_t)Nelem] > 0 && !K_near) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null K_near");
  std::vector<int64_t> trg_of_entry((size_t)n_near, -1);
  for (int64_t i = 0; i < Nt; i++) {
    if (near_trg_cnt[i] < 0 || near_trg_dsp[i] < 0 || near_trg_dsp[i] + near_trg_cnt[i] > n_near) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "near_trg_dsp/cnt outside the near list");
    for (int64_t p = near_trg_dsp[i]; p < near_trg_dsp[i] + near_trg_cnt[i]; p++) {
      const int64_t entry = near_scatter_index[p];
      if (entry < 0 || entry >= n_near || trg_of_entry[(size_t)entry] >= 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "near_scatter_index is not a permutation of the near list");
      trg_of_entry[(size_t)entry] = i;
    }
  }
  for (int64_t q = 0; q < n_near; q++)
    if (trg_of_entry[(size_t)q] < 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "a near-list entry belongs to no target");
  // slot of every caller target in the operator's own (Morton) target order
  std::vector<int64_t> slot((size_t)Nt);
  for (int64_t i = 0; i < Nt; i++) slot[op->perm.empty() ? (size_t)i : (size_t)op->perm[(size_t)i]] = i;
  op->near.assign((size_t)G, nullptr);
  op->near_f.assign((size_t)G, nullptr);
  op->near_f_cap.assign((size_t)G, 0);
  op->near_f_len = f_len;
  op->near_trg_dim = trg_dim;
  const char* Kh = (const char*)K_near;
  for (int g = 0; g < G; g++) {
    const OpDevice& d = op->devs[(size_t)g];
    const int64_t nt_g = d.t1 - d.t0;
    // this device's share: per element the columns (near targets) whose target lies in [t0, t1), in their original order
    std::vector<int64_t> cnt_g((size_t)Nelem, 0), kcnt_g((size_t)Nelem, 0), new_id((size_t)n_near, -1);
    std::vector<char> Kg;
    int64_t n_g = 0;
    for (int64_t e = 0; e < Nelem; e++) {
      const int64_t c0 = near_dsp[(size_t)e], nc = near_elem_cnt[e], rows = elem_nds_cnt[e] * src_dim;
      const bool has_matrix = (k_dsp[(size_t)e + 1] > k_dsp[(size_t)e]);
      std::vector<int64_t> cols;
      for (int64_t j = 0; j < nc; j++) {
        const int64_t s = slot[(size_t)trg_of_entry[(size_t)(c0 + j)]];
        if (s >= d.t0 && s < d.t1) { cols.push_back(j); new_id[(size_t)(c0 + j)] = n_g++; }
      }
      cnt_g[(size_t)e] = (int64_t)cols.size();
      if (!has_matrix || cols.empty() || rows == 0) continue;
      kcnt_g[(size_t)e] = elem_nds_cnt[e] * (int64_t)cols.size();
      const size_t row_in = (size_t)nc * trg_dim * rs, piece = (size_t)trg_dim * rs;
      const char* blk = Kh + (size_t)k_dsp[(size_t)e] * src_dim * trg_dim * rs;
      const size_t at = Kg.size();
      Kg.resize(at + (size_t)rows * cols.size() * piece);
      char* out = Kg.data() + at;
      if ((int64_t)cols.size() == nc) { std::memcpy(out, blk, (size_t)rows * row_in); continue; }   // the whole block lives here
      for (int64_t r = 0; r < rows; r++)
        for (int64_t j : cols) { std::memcpy(out, blk + (size_t)r * row_in + (size_t)j * piece, piece); out += piece; }
    }
    std::vector<int64_t> sc_g((size_t)n_g), tc_g((size_t)nt_g, 0), td_g((size_t)nt_g, 0);
    int64_t p_g = 0;
    for (int64_t s = d.t0; s < d.t1; s++) {   // targets in slab order, their entries in the caller's order
      const int64_t i = op->perm.empty() ? s : op->perm[(size_t)s];
      td_g[(size_t)(s - d.t0)] = p_g;
      tc_g[(size_t)(s - d.t0)] = near_trg_cnt[i];
      for (int64_t p = near_trg_dsp[i]; p < near_trg_dsp[i] + near_trg_cnt[i]; p++) sc_g[(size_t)p_g++] = new_id[(size_t)near_scatter_index[p]];
    }
    if (nt_g == 0) continue;
    int rc = sctl_amd_near_create(op->real, d.device, Nelem, src_dim, trg_dim, elem_nds_cnt, cnt_g.data(), kcnt_g.data(), Kg.empty() ? nullptr : Kg.data(), nt_g,
                                  sc_g.empty() ? nullptr : sc_g.data(), tc_g.data(), td_g.data(), &op->near[(size_t)g]);
    if (rc == SCTL_AMD_OK && f_len > 0) {
      DeviceScope scope(d.device);
      if (scope.err != hipSuccess || grow(&op->near_f[(size_t)g], &op->near_f_cap[(size_t)g], (size_t)f_len * rs) != hipSuccess) rc = fail(SCTL_AMD_ERR_HIP, "cannot allocate the near-field density on device " + std::to_string(d.device));
    }
    if (rc != SCTL_AMD_OK) { const std::string msg = error_text(); op_release_near(op); error_text() = msg; return rc; }
  }
  return SCTL_AMD_OK;
}

}  // extern "C"
