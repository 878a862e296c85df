// What the translation units of libsctl_amd.so share: the kernel registry, the digits -> refinement-mode rule, the per-thread error text, the argument
// checks and the work counters (all defined in capi.hip), the pinned staging of staging.hpp bound to HIP, and the few entry points that op.hip and
// host_entries.hip offer each other.  Not installed: plugins see only include/sctl_amd/device/.
#pragma once
#include <sctl_amd.h>
#include <sctl_amd/device/launch.hpp>

#include "staging.hpp"

#include <string>
#include <vector>

namespace sctl_amd {

const KernelEntry* registry(int id);               // nullptr for an unknown id; built-ins 0..SCTL_AMD_NUM_KERNELS-1, then registered plugins
int registry_size();
int registry_find(const char* name);               // id or SCTL_AMD_ERR_UNKNOWN_KERNEL
int registry_add(const KernelEntry& e, std::string* why);   // copies the entry, assigns and returns its id; < 0 with *why on refusal

int mode_for(int real, int digits);                // digits -> rsqrt refinement mode (ukernels.hpp)
KerCtx make_ctx(const KernelEntry& k, const void* ctx);
int set_error(int code, const std::string& msg);   // records the text for sctl_amd_last_error() on this thread, returns code
int device_count_quiet();
int comm_agree(sctl_amd_comm* c, int local_rc, const char* what);   // comm.hip: all ranks learn whether every rank's local step succeeded
void count_work(int64_t pairs, const KernelEntry& k);   // sctl_amd_counters (generic-kernel.txx:188)

#pragma GCC visibility push(hidden)
inline int fail(int code, const std::string& msg) { return set_error(code, msg); }
std::string& error_text();                         // this thread's text, for the callers that carry it across threads or a clean-up
#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) return fail(SCTL_AMD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

// argument checks that every entry shares; each sets the error text and returns its code, SCTL_AMD_OK when the arguments pass
int check_ctx(const KernelEntry& k, const void* ctx, int ctx_bytes);          // the kernel's context blob is there and has its size
int check_real_sizes(const KernelEntry* k, int real, int64_t Nt, int64_t Ns);  // known kernel, F64 or F32, no negative size
int check_common(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, int ctx_bytes, const void* ctx);
int check_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                    const void* v_trg, int ctx_bytes, const void* ctx);
int check_transpose(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg,
                    const void* g_src, int ctx_bytes, const void* ctx);
int check_transpose_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                              const void* w_trg, const void* g_src, int ctx_bytes, const void* ctx);
int check_grad(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
               const void* w_trg, const void* g_nrm, int ctx_bytes, const void* ctx);
int check_grad_densities(const KernelEntry* k, int real, int nd, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                         const void* v_src, const void* w_trg, const void* g_nrm, int ctx_bytes, const void* ctx);
int check_jvp(const KernelEntry* k, int real, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
              const void* d_nrm, const void* dv_trg, int ctx_bytes, const void* ctx);
int no_device();                                  // SCTL_AMD_ERR_NO_DEVICE with the text every entry gives
int check_device(int device);                      // ... and a device index within the devices there are

struct HipPinned {
  using error = hipError_t;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(char** p, size_t bytes) { return hipHostMalloc((void**)p, bytes, hipHostMallocPortable); }
  static void free(char* p) { (void)hipHostFree(p); }
};
using PinnedBuf = PinnedBufT<HipPinned>;
// host array -> pinned slice -> device (async on st); the slice must stay untouched until st is synchronised
inline hipError_t upload(void* dst, const void* src, size_t bytes, PinnedBuf& stage, hipStream_t st) {
  if (!bytes) return hipSuccess;
  char* q = stage.take(bytes);
  std::memcpy(q, src, bytes);   // (against a copy straight from the caller's pageable array: profiles/r01b_host_entry.txt)
  return hipMemcpyAsync(dst, q, bytes, hipMemcpyHostToDevice, st);
}

// host_entries.hip
void host_slots_release();                         // the calling thread's slots: streams, device buffers and pinned staging go with them
// op.hip: the operators that the host-buffer entry over a device list keeps between calls
int op_cache_acquire(int kernel, int real, const std::vector<int>& devs, sctl_amd_op** out);
void op_cache_release(sctl_amd_op* op, bool failed);
void op_cache_trim();
#pragma GCC visibility pop

}  // namespace sctl_amd
