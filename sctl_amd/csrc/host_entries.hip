// The host-buffer entries of include/sctl_amd.h that make one call on one device: upload through pinned staging, one driver call (eval_drivers.hpp),
// download, add into the caller's arrays.  Over a device list the forward entry hands the work to an operator handle (op.hip).
#include "eval_drivers.hpp"
#include "workspace.hpp"

#include <climits>
#include <memory>
#include <string>
#include <vector>

namespace sctl_amd {
namespace {

struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) { workspace_forget(s); (void)hipStreamDestroy(s); } }
};
// grow-only device buffer and the per-(thread, device) cache of the one-shot host entries
struct CachedDevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
    if (e == hipSuccess) cap = bytes ? bytes : 8;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// Stream, device buffers and pinned staging are kept per (calling thread, device) between calls: at 2^14 points the
// five hipMalloc/hipFree pairs and the stream creation cost 2.9 of the 3.1 ms a call took.  The reference's SetupNear calls KernelMatrix once per
// element from every thread of an OpenMP loop (boundary_integral.txx:949-986), thousands of small blocks, which cost less than those would.
struct HostSlot {
  int device = -1;
  StreamGuard st;
  CachedDevBuf buf[8];
  PinnedBuf stage;
  void trim(size_t keep) {
    size_t tot = stage.cap;
    for (auto& b : buf) tot += b.cap;
    if (tot <= keep) return;
    for (auto& b : buf) b.release();
    stage.release();
  }
  ~HostSlot() { for (auto& b : buf) b.release(); }
};
std::vector<std::unique_ptr<HostSlot>>& host_slots() {
  static thread_local std::vector<std::unique_ptr<HostSlot>> slots;
  return slots;
}
HostSlot& host_slot(int device) {
  auto& slots = host_slots();
  for (auto& s : slots) if (s->device == device) return *s;
  slots.emplace_back(new HostSlot);
  slots.back()->device = device;
  return *slots.back();
}

// One host-buffer call on the calling thread's slot for a device (a thread makes one call at a time).  Declare the inputs, then the outputs, each with
// the slot's device buffer it lives in; start() reserves the buffers and the staging for all of them, uploads and zeroes; the caller launches on st with
// dev(); finish() brings the outputs back and, after the one synchronise, stores or adds them.  Anything above 64 MB is released when the call returns.
struct HostCall {
  enum { kZero = 1, kStaged = 2, kAccumulate = 4 };   // an output that is neither zeroed nor staged is written once, straight into the caller's array
  struct Io { int buf; const void* src; void* dst; size_t bytes; int flags; };
  DeviceScope scope;
  HostSlot& hs;
  const int real;
  hipStream_t st = nullptr;
  Io io[8];
  int n_in = 0, n = 0;
  HostCall(int device, int real_) : scope(device), hs(host_slot(device)), real(real_) {}
  ~HostCall() { if (st) hs.trim((size_t)64 << 20); }
  void in(int buf, const void* src, size_t bytes) { io[n++] = Io{buf, src, nullptr, bytes, kStaged}; n_in = n; }
  void out(int buf, void* dst, size_t bytes, int flags) { io[n++] = Io{buf, nullptr, dst, bytes, flags}; }
  void* dev(int buf) const { return hs.buf[buf].p; }
  int start() {
    HIP_TRY(scope.err);
    if (!hs.st.s) HIP_TRY(hipStreamCreateWithFlags(&hs.st.s, hipStreamNonBlocking));
    st = hs.st.s;
    size_t staged = 0;
    for (int i = 0; i < n; i++) {
      HIP_TRY(hs.buf[io[i].buf].reserve(io[i].bytes));
      if (io[i].flags & kStaged) staged += pad256(io[i].bytes);
    }
    HIP_TRY(hs.stage.reserve(staged));
    for (int i = 0; i < n_in; i++) HIP_TRY(upload(dev(io[i].buf), io[i].src, io[i].bytes, hs.stage, st));
    for (int i = n_in; i < n; i++)
      if (io[i].flags & kZero) HIP_TRY(hipMemsetAsync(dev(io[i].buf), 0, io[i].bytes, st));
    return SCTL_AMD_OK;
  }
  int finish() {
    const void* back[8];
    for (int i = n_in; i < n; i++) {
      void* to = (io[i].flags & kStaged) ? (void*)hs.stage.take(io[i].bytes) : io[i].dst;
      HIP_TRY(hipMemcpyAsync(to, dev(io[i].buf), io[i].bytes, hipMemcpyDeviceToHost, st));
      back[i] = to;
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = n_in; i < n; i++)
      if (io[i].flags & kStaged) store_or_add(real, io[i].dst, back[i], (int64_t)(io[i].bytes / real_size(real)), (io[i].flags & kAccumulate) != 0);
    return SCTL_AMD_OK;
  }
};
constexpr int kAddStaged = HostCall::kZero | HostCall::kStaged | HostCall::kAccumulate;   // v += device result (generic-kernel.txx:182-186)

// one GPU: all targets against all sources
int eval_host_one(const KernelEntry& k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                  void* v_trg, int digits, const void* ctx, int device) {
  if (Nt <= 0 || Ns <= 0) return SCTL_AMD_OK;
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k.nd * rs);
  c.in(3, v_src, (size_t)Ns * k.k0 * rs);
  c.out(4, v_trg, (size_t)Nt * k.k1 * rs, kAddStaged);
  int rc = c.start();
  if (rc == SCTL_AMD_OK) rc = eval_device(k, real, Nt, Ns, c.dev(0), c.dev(1), c.dev(2), c.dev(3), c.dev(4), digits, ctx, c.st);
  return rc ? rc : c.finish();
}

}  // namespace
void host_slots_release() { host_slots().clear(); }
}  // namespace sctl_amd

using namespace sctl_amd;

extern "C" {

int sctl_amd_eval_host_multi(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                             const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, const int* devices, int n_devices) {
  const KernelEntry* k = registry(kernel);
  int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((Ns > 0 && !v_src) || (Nt > 0 && !v_trg)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null density or potential array");
  const int avail = device_count_quiet();
  if (avail <= 0) return no_device();
  if (n_devices <= 0) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "n_devices must be positive");
  std::vector<int> devs(n_devices);
  for (int g = 0; g < n_devices; g++) {
    devs[g] = devices ? devices[g] : g;
    if (devs[g] < 0 || devs[g] >= avail) return fail(SCTL_AMD_ERR_NO_DEVICE, "device index " + std::to_string(devs[g]) + " out of range");
  }
  if (n_devices == 1) return eval_host_one(*k, real, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, devs[0]);
  // several GPUs: the device-resident operator does it (Morton-ordered target slabs with the rank formula of
  // fmm-wrapper.txx:507, sources replicated, one host thread and one stream per GPU).  The operator — its streams, device buffers and
  // pinned staging — is kept between calls (the operator cache of op.hip): a caller like the reference's ParticleFMM::EvalDirect comes back every
  // solver iteration with arrays of the same sizes, and creating and freeing a dozen device buffers per GPU per call cost more than the
  // evaluation's share of a GPU on an 8-GPU node.
  sctl_amd_op* op = nullptr;
  rc = op_cache_acquire(kernel, real, devs, &op);
  if (rc == SCTL_AMD_OK) rc = sctl_amd_op_set_targets(op, Nt, r_trg);
  if (rc == SCTL_AMD_OK) rc = sctl_amd_op_set_sources(op, Ns, r_src, n_src);
  if (rc == SCTL_AMD_OK && Nt > 0 && Ns > 0) rc = sctl_amd_op_eval(op, v_src, v_trg, /*accumulate*/ 1, digits, ctx, ctx_bytes);
  const std::string msg = error_text();
  op_cache_release(op, rc != SCTL_AMD_OK);
  if (rc != SCTL_AMD_OK) error_text() = msg;
  return rc;
}

int sctl_amd_eval_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                       const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device) {
  return sctl_amd_eval_host_multi(kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, &device, 1);
}

// nd == 1 goes through the single-density entry (bit-identical results); nd == 0 is a no-op after the argument checks.
// Coordinates and normals go down once, the nd density rows in one transfer, the nd result rows come back in one.
int sctl_amd_eval_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                 const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_host(kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, device);
  if ((rc = check_device(device))) return rc;
  if (nd == 0 || Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, v_src, (size_t)nd * Ns * k->k0 * rs);
  c.out(4, v_trg, (size_t)nd * Nt * k->k1 * rs, kAddStaged);
  rc = c.start();
  if (rc == SCTL_AMD_OK) rc = eval_densities_device(*k, real, nd, Nt, Ns, c.dev(0), c.dev(1), c.dev(2), c.dev(3), c.dev(4), digits, ctx, c.st);
  return rc ? rc : c.finish();
}

int sctl_amd_eval_transpose_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                 const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_transpose(k, real, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, ctx_bytes, ctx);
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;   // an empty set: nothing is read or written
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, w_trg, (size_t)Nt * k->k1 * rs);
  c.out(4, g_src, (size_t)Ns * k->k0 * rs, HostCall::kZero | HostCall::kStaged | (accumulate ? HostCall::kAccumulate : 0));
  rc = c.start();
  if (rc == SCTL_AMD_OK) rc = eval_transpose_device(*k, real, Nt, Ns, c.dev(0), c.dev(1), c.dev(2), c.dev(3), c.dev(4), digits, ctx, c.st);
  return rc ? rc : c.finish();
}

// nd == 1 goes through the single transposed entry (bit-identical results); nd == 0 is a no-op after the argument checks.
// Coordinates and normals go down once, the nd weight rows in one transfer, the nd result rows come back in one.
int sctl_amd_eval_transpose_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                           const void* w_trg, void* g_src, int accumulate, int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_transpose_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_transpose_host(kernel, real, Nt, Ns, r_trg, r_src, n_src, w_trg, g_src, accumulate, digits, ctx, ctx_bytes, device);
  if ((rc = check_device(device))) return rc;
  if (nd == 0 || Nt == 0 || Ns == 0) return SCTL_AMD_OK;   // nothing is read or written
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, w_trg, (size_t)nd * Nt * k->k1 * rs);
  c.out(4, g_src, (size_t)nd * Ns * k->k0 * rs, HostCall::kZero | HostCall::kStaged | (accumulate ? HostCall::kAccumulate : 0));
  rc = c.start();
  if (rc == SCTL_AMD_OK) rc = eval_transpose_densities_device(*k, real, nd, Nt, Ns, c.dev(0), c.dev(1), c.dev(2), c.dev(3), c.dev(4), digits, ctx, c.st);
  return rc ? rc : c.finish();
}

int sctl_amd_eval_grad_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                            const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int accumulate, int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_grad(k, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_nrm, ctx_bytes, ctx);
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;   // an empty set: nothing is read or written
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, v_src, (size_t)Ns * k->k0 * rs);
  c.in(4, w_trg, (size_t)Nt * k->k1 * rs);
  void* out[3] = {g_trg, g_src, g_nrm};   // a null output is not declared: no buffer, no transfer
  for (int i = 0; i < 3; i++)
    if (out[i]) c.out(5 + i, out[i], (size_t)(i == 0 ? Nt : Ns) * 3 * rs, HostCall::kZero | HostCall::kStaged | (accumulate ? HostCall::kAccumulate : 0));
  rc = c.start();
  if (rc == SCTL_AMD_OK)
    rc = eval_grad_device(*k, real, Nt, Ns, c.dev(0), c.dev(1), k->nd ? c.dev(2) : nullptr, c.dev(3), c.dev(4), g_trg ? c.dev(5) : nullptr,
                          g_src ? c.dev(6) : nullptr, g_nrm ? c.dev(7) : nullptr, digits, ctx, c.st);
  return rc ? rc : c.finish();
}

// A null tangent is not declared: no buffer, no transfer, and the driver gets a null pointer for it.
int sctl_amd_eval_jvp_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                           const void* d_trg, const void* d_src, const void* d_nrm, void* dv_trg, int accumulate, int digits, const void* ctx, int ctx_bytes,
                           int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_jvp(k, real, Nt, Ns, r_trg, r_src, n_src, v_src, d_nrm, dv_trg, ctx_bytes, ctx);
  if (rc) return rc;
  if ((rc = check_device(device))) return rc;
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;                  // an empty set: nothing is read or written
  if (!d_trg && !d_src && !d_nrm && accumulate) return SCTL_AMD_OK;   // the tangent along a zero perturbation: nothing to add
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, v_src, (size_t)Ns * k->k0 * rs);
  if (d_trg) c.in(4, d_trg, (size_t)Nt * 3 * rs);
  if (d_src) c.in(5, d_src, (size_t)Ns * 3 * rs);
  if (d_nrm) c.in(6, d_nrm, (size_t)Ns * k->nd * rs);
  c.out(7, dv_trg, (size_t)Nt * k->k1 * rs, HostCall::kZero | HostCall::kStaged | (accumulate ? HostCall::kAccumulate : 0));
  rc = c.start();
  if (rc == SCTL_AMD_OK)
    rc = eval_jvp_device(*k, real, Nt, Ns, c.dev(0), c.dev(1), k->nd ? c.dev(2) : nullptr, c.dev(3), d_trg ? c.dev(4) : nullptr, d_src ? c.dev(5) : nullptr,
                         d_nrm ? c.dev(6) : nullptr, c.dev(7), digits, ctx, c.st);
  return rc ? rc : c.finish();
}

// nd == 1 goes through the single gradient entry (bit-identical results); nd == 0 is a no-op after the argument checks.
// Coordinates and normals go down once, the nd density rows and the nd weight rows in one transfer each; the outputs do not grow with nd.
int sctl_amd_eval_grad_densities_host(int kernel, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                      const void* v_src, const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int accumulate, int digits, const void* ctx,
                                      int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_grad_densities(k, real, nd, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_nrm, ctx_bytes, ctx);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_eval_grad_host(kernel, real, Nt, Ns, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, accumulate, digits, ctx, ctx_bytes, device);
  if ((rc = check_device(device))) return rc;
  if (nd == 0 || Nt == 0 || Ns == 0) return SCTL_AMD_OK;   // nothing is read or written
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.in(3, v_src, (size_t)nd * Ns * k->k0 * rs);
  c.in(4, w_trg, (size_t)nd * Nt * k->k1 * rs);
  void* out[3] = {g_trg, g_src, g_nrm};   // a null output is not declared: no buffer, no transfer
  for (int i = 0; i < 3; i++)
    if (out[i]) c.out(5 + i, out[i], (size_t)(i == 0 ? Nt : Ns) * 3 * rs, HostCall::kZero | HostCall::kStaged | (accumulate ? HostCall::kAccumulate : 0));
  rc = c.start();
  if (rc == SCTL_AMD_OK)
    rc = eval_grad_densities_device(*k, real, nd, Nt, Ns, c.dev(0), c.dev(1), k->nd ? c.dev(2) : nullptr, c.dev(3), c.dev(4), g_trg ? c.dev(5) : nullptr,
                                    g_src ? c.dev(6) : nullptr, g_nrm ? c.dev(7) : nullptr, digits, ctx, c.st);
  return rc ? rc : c.finish();
}

int sctl_amd_kernel_matrix_host(int kernel, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, void* M,
                                int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_common(k, real, Nt, Ns, r_trg, r_src, n_src, ctx_bytes, ctx);
  if (rc) return rc;
  if (Nt > 0 && Ns > 0 && !M) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null matrix");
  if ((rc = check_device(device))) return rc;
  if (Nt == 0 || Ns == 0) return SCTL_AMD_OK;
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)Nt * 3 * rs);
  c.in(1, r_src, (size_t)Ns * 3 * rs);
  c.in(2, n_src, (size_t)Ns * k->nd * rs);
  c.out(3, M, (size_t)Ns * k->k0 * Nt * k->k1 * rs, 0);   // M is written once by this call: no staging needed for a D2H
  rc = c.start();
  if (rc == SCTL_AMD_OK)
    rc = sctl_amd_kernel_matrix_device(kernel, real, Nt, Ns, c.dev(0), c.dev(1), k->nd ? c.dev(2) : nullptr, c.dev(3), digits, ctx, ctx_bytes, c.st);
  return rc ? rc : c.finish();
}

int sctl_amd_kernel_matrix_batch_host(int kernel, int real, int64_t nbatch, const int64_t* Nt, const int64_t* Ns, const void* r_trg, const void* r_src,
                                      const void* n_src, void* M, int digits, const void* ctx, int ctx_bytes, int device) {
  const KernelEntry* k = registry(kernel);
  int rc = check_real_sizes(k, real, 0, 0);
  if (rc) return rc;
  if (nbatch < 0 || (nbatch > 0 && (!Nt || !Ns))) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "negative batch count or null size arrays");
  if ((rc = check_ctx(*k, ctx, ctx_bytes))) return rc;
  std::vector<MatTile> tiles;
  int64_t nt_all = 0, ns_all = 0, m_all = 0, pairs = 0;
  for (int64_t b = 0; b < nbatch; b++) {
    if (Nt[b] < 0 || Ns[b] < 0 || Nt[b] > INT32_MAX || Ns[b] > INT32_MAX) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "block size out of range");
    if (Nt[b] > 0 && Ns[b] > 0)
      for (int64_t t0 = 0; t0 < Nt[b]; t0 += 64) tiles.push_back(MatTile{nt_all, ns_all, m_all, (int32_t)Nt[b], (int32_t)Ns[b], (int32_t)t0, 0});
    nt_all += Nt[b];
    ns_all += Ns[b];
    m_all += Ns[b] * k->k0 * Nt[b] * k->k1;
    pairs += Nt[b] * Ns[b];
  }
  if ((nt_all > 0 && !r_trg) || (ns_all > 0 && !r_src)) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate array");
  if (ns_all > 0 && k->nd > 0 && !n_src) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k->name) + " needs source normals (n_src is null)");
  if (m_all > 0 && !M) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "null matrix array");
  if ((rc = check_device(device))) return rc;
  if (tiles.empty()) return SCTL_AMD_OK;
  if (tiles.size() > 0x7fffffffu) return fail(SCTL_AMD_ERR_BAD_ARGUMENT, "too many tiles for one launch");
  const size_t rs = real_size(real);
  HostCall c(device, real);
  c.in(0, r_trg, (size_t)nt_all * 3 * rs);
  c.in(1, r_src, (size_t)ns_all * 3 * rs);
  c.in(2, n_src, (size_t)ns_all * k->nd * rs);
  c.in(3, tiles.data(), tiles.size() * sizeof(MatTile));
  c.out(4, M, (size_t)m_all * rs, 0);   // M is written once by this call: no staging needed for a D2H
  if ((rc = c.start())) return rc;
  (void)hipGetLastError();
  matrix_batch_launch(*k, real, (const MatTile*)c.dev(3), (int64_t)tiles.size(), c.dev(0), c.dev(1), c.dev(2), c.dev(4), digits, ctx, c.st);
  HIP_TRY(hipGetLastError());
  if ((rc = c.finish())) return rc;
  count_work(pairs, *k);
  return SCTL_AMD_OK;
}

}  // extern "C"
