// Batched list evaluation (sctl_amd_lists_*, sctl_amd_eval_lists_*): the host side of include/sctl_amd/device/lists_kernel.hpp.
// A plan validates the lists, groups them by target range (a leaf box and ALL the source boxes listed for it become the work of
// whole waves), orders the work items by cost and keeps them on the device; an evaluation is ONE launch.
#include "internal.hpp"
#include "lists_rows_kernel.hpp"
#include <sctl_amd/device/lists_grad_kernel.hpp>
#include "workspace.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace sctl_amd {
namespace {
#define LISTS_TRY(expr)                                                                                             \
  do {                                                                                                              \
    hipError_t e_ = (expr);                                                                                         \
    if (e_ != hipSuccess) return set_error(SCTL_AMD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)
}  // namespace
}  // namespace sctl_amd

// The work list of one direction.  FORWARD: the owners are the targets and the sources are streamed (lists_kernel.hpp); TRANSPOSE: the owners are the sources and
// the targets are streamed (lists_transpose_kernel.hpp).  Both are made by the same planning code (plan_side) with the two point sets exchanged.
struct ListsSide {
  int64_t nitems = 0, nranges = 0, pairs = 0, nblocks = 0;
  int32_t xcd_first[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  void *d_items = nullptr, *d_ranges = nullptr, *d_groups = nullptr, *d_flat = nullptr;   // (groups + flat indices of the streamed points: the packed small owner ranges)
  int64_t npacked_groups = 0, nflat = 0;
};

struct sctl_amd_lists {
  const sctl_amd::KernelEntry* k = nullptr;
  int real = 0, device = 0, directions = 0;
  int64_t Nt = 0, Ns = 0;
  ListsSide side[2];      // [0] FORWARD, [1] TRANSPOSE; a side that was not planned stays empty
  // host-pointer evaluation: device copies of the caller's arrays and pinned staging, grown on demand
  hipStream_t st = nullptr;
  void* dbuf[8] = {};     // [0 .. 4]: lists_host_call; [5 .. 7]: the gradient's g_trg, g_src, g_nrm (lists_grad_host_call)
  size_t dcap[8] = {};
  char* pinned = nullptr;
  size_t pinned_cap = 0;
};

using namespace sctl_amd;
// Owner ranges of up to this many points are packed, several to a wave (lists_kernel.hpp); larger ones keep a wave (or several) to themselves.  Measured on
// 2^21 points in g^3 boxes, every box against its 27 neighbours (tools/time_lists.py, profiles/r04_time_lists_classes.txt; Laplace / Stokeslet, % of the fp64
// peak, packing up to 0 | 8 | 16 | 32 | 64 points): ~8 per box 4.4 | 6.6 | 11.2 | 11.3 | 11.0 and 11.7 | 15.8 | 23.7 | 23.9 | 23.6; ~11 per box 7.3 | 7.7 | 11.5 |
// 12.9 | 12.8; ~24 per box 12.0 | 11.9 | 11.8 | 15.5 | 15.5; ~64 per box 21.1 | 20.9 | 20.9 | 20.7 | 18.3 and 45.7 | 46.5 | 46.0 | 46.0 | 40.6: 32.
constexpr int64_t kPackUpTo = 32;

namespace {
// One side's work list on the host, before it goes to the device
struct SidePlan {
  std::vector<ListItem> items;
  std::vector<ListRange> ranges;
  std::vector<PackedGroup> pgroups;
  std::vector<uint32_t> flat;
  int32_t xcd_first[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int64_t pairs = 0, longest = 0;
};

// Plans one side: the lists grouped by OWNER range (own_off, own_cnt), the other point set STREAMED (str_off, str_cnt; Nstr points, each at most
// `widest` bytes in the widest of its arrays).  `owner` / `streamed` name the two sets in messages ("target" / "source" forward, exchanged transposed).
int plan_side(int64_t nlists, const int64_t* own_off, const int64_t* own_cnt, const int64_t* str_off, const int64_t* str_cnt, int64_t Nstr, int64_t widest,
              const char* owner, SidePlan& out) {
  // group the lists by owner range: stable sort by (first owner, count) keeps the caller's order inside a group, which is
  // the order the streamed points are summed in
  std::vector<int64_t> order;
  order.reserve((size_t)nlists);
  for (int64_t l = 0; l < nlists; l++)
    if (own_cnt[l] > 0 && str_cnt[l] > 0) order.push_back(l);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return own_off[a] != own_off[b] ? own_off[a] < own_off[b] : own_cnt[a] < own_cnt[b]; });
  struct Group { int64_t t0, nt, first_range, nranges, nsrc; };
  std::vector<Group> groups;
  std::vector<ListRange>& ranges = out.ranges;
  ranges.reserve(order.size());
  int64_t pairs = 0;
  for (size_t i = 0; i < order.size(); i++) {
    const int64_t l = order[i];
    if (groups.empty() || groups.back().t0 != own_off[l] || groups.back().nt != own_cnt[l]) {
      if (!groups.empty() && own_off[l] < groups.back().t0 + groups.back().nt)
        return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("the ") + owner + " ranges of lists " + std::to_string(order[i - 1]) + " and " + std::to_string(l) +
                                                        " overlap without being equal: " + owner + " ranges must be identical or disjoint");
      groups.push_back(Group{own_off[l], own_cnt[l], (int64_t)ranges.size(), 0, 0});
    }
    ranges.push_back(ListRange{str_off[l], str_cnt[l]});
    groups.back().nranges++;
    groups.back().nsrc += str_cnt[l];
    pairs += own_cnt[l] * str_cnt[l];
  }
  for (const Group& g : groups)
    if (g.nranges > INT32_MAX) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, std::string("too many lists for one ") + owner + " range");
  // Eight shares, one per XCD (lists_kernel.hpp): contiguous runs of owner ranges in the caller's order — a tree code lists its
  // boxes along a space-filling curve, so a run is a compact region whose boxes stream the same points — each with 1/8 of the
  // pair count.  Inside a share: long items first (a short tail), coarsely — by the number of 4096-point chunks —, neighbours
  // otherwise staying neighbours.
  std::vector<ListItem>& items = out.items;
  std::vector<PackedGroup>& pgroups = out.pgroups;
  std::vector<uint32_t>& flat = out.flat;
  // The packed form keeps one 32-bit index per (small owner range, streamed point): it is used while that list stays below 2^30 entries (4 GB) and the
  // streamed points can be indexed with 32 bits; SCTL_AMD_LISTS_PACK=0 keeps every range on the one-range-per-wave items (A/B runs, tests of that path)
  // (and while every streamed array stays under 4 GB: the packed items address a streamed point by a 32-bit byte offset)
  bool pack_small = Nstr <= (int64_t)UINT32_MAX / widest;
  int64_t pack_upto = kPackUpTo;
  if (const char* e = std::getenv("SCTL_AMD_LISTS_PACK")) pack_upto = std::min<int64_t>(64, std::atoi(e));   // (0: off; 8 / 16 / 32 / 64: the largest packed range)
  pack_small = pack_small && pack_upto > 0;
  if (pack_small) {
    int64_t entries = 0;
    for (const Group& g : groups)
      if (g.nt <= pack_upto) entries += g.nsrc;
    if (entries > ((int64_t)1 << 30)) pack_small = false;
    else flat.reserve((size_t)entries);
  }
  int32_t* const xcd_first = out.xcd_first;
  {
    size_t g0 = 0;
    int64_t done = 0;
    for (int x = 0; x < 8; x++) {
      size_t g1 = g0;
      const int64_t upto = pairs / 8 * (x + 1) + (x == 7 ? pairs % 8 : 0);
      while (g1 < groups.size() && (x == 7 || done + groups[g1].nt * groups[g1].nsrc / 2 < upto)) { done += groups[g1].nt * groups[g1].nsrc; g1++; }
      std::vector<size_t> gorder(g1 - g0);
      std::iota(gorder.begin(), gorder.end(), g0);
      std::stable_sort(gorder.begin(), gorder.end(), [&](size_t a, size_t b) { return (groups[a].nsrc >> 12) > (groups[b].nsrc >> 12); });
      // Small owner ranges (<= 64 points) are PACKED (lists_kernel.hpp): those of one class (lanes x owners per lane) share waves, 64 / P at a time, in
      // the share's order — neighbours along the caller's space-filling curve —, each with its flat sequence.  They follow the share's larger items.
      std::vector<size_t> small[4];
      for (size_t gi : gorder) {
        const Group& g = groups[gi];
        if (pack_small && g.nt <= pack_upto && g.nsrc <= INT32_MAX) {
          small[g.nt <= 8 ? 0 : g.nt <= 16 ? 1 : g.nt <= 32 ? 2 : 3].push_back(gi);
          continue;
        }
        // 128-owner items (two owners per lane: half the LDS reads per pair); the remainder: more than 96 -> one more such item,
        // 65..96 -> a one-owner-per-lane item of 64 plus a small one, up to 64 -> one item (up to 32: run as lane replicas)
        for (int64_t t = 0; t < g.nt;) {
          const int64_t left = g.nt - t;
          const int64_t n = left > 96 ? std::min<int64_t>(left, 2 * kListWave) : (left > kListWave ? kListWave : left);
          items.push_back(ListItem{g.t0 + t, (int32_t)n, (int32_t)g.nranges, g.first_range});
          t += n;
        }
      }
      for (int cls = 3; cls >= 0; cls--) {
        const size_t per_item = (size_t)(kListWave / kPackedLanes[cls]);
        for (size_t k = 0; k < small[cls].size(); k++) {
          if (k % per_item == 0) items.push_back(ListItem{(int64_t)pgroups.size(), 0, -1 - cls, 0});
          const Group& g = groups[small[cls][k]];
          items.back().nt++;
          pgroups.push_back(PackedGroup{g.t0, (int64_t)flat.size(), (int32_t)g.nt, (int32_t)g.nsrc});
          for (int64_t r = g.first_range; r < g.first_range + g.nranges; r++)
            for (int64_t q = 0; q < ranges[(size_t)r].ns; q++) flat.push_back((uint32_t)(ranges[(size_t)r].s0 + q));
        }
      }
      if (items.size() > 0x7ffffff0u) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "too many work items for one launch");
      xcd_first[x + 1] = (int32_t)items.size();
      g0 = g1;
    }
  }
  int64_t longest = 0;
  for (int x = 0; x < 8; x++) longest = std::max<int64_t>(longest, xcd_first[x + 1] - xcd_first[x]);
  if (longest * 8 > 0x7fffffff) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "too many work items for one launch");
  out.pairs = pairs;
  out.longest = longest;
  return SCTL_AMD_OK;
}

// The handle's stream, its device buffers [0, n) grown to bytes[i] and its pinned block grown to hold them all; the plan's device is current.
int lists_staging(sctl_amd_lists* p, const size_t* bytes, int n) {
  if (!p->st) LISTS_TRY(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    total += Carver::pad(bytes[i]);
    if (bytes[i] > p->dcap[i]) {
      if (p->dbuf[i]) { LISTS_TRY(hipFree(p->dbuf[i])); p->dbuf[i] = nullptr; p->dcap[i] = 0; }
      LISTS_TRY(hipMalloc(&p->dbuf[i], bytes[i]));
      p->dcap[i] = bytes[i];
    }
  }
  if (total > p->pinned_cap) {   // every host transfer goes through pinned staging (staging.hpp: PinnedBufT explains why)
    if (p->pinned) { LISTS_TRY(hipHostFree(p->pinned)); p->pinned = nullptr; p->pinned_cap = 0; }
    LISTS_TRY(hipHostMalloc((void**)&p->pinned, total, hipHostMallocPortable));
    p->pinned_cap = total;
  }
  return SCTL_AMD_OK;
}

// A host-pointer evaluation of nd rows in either direction, after the entry's own checks: device copies of the caller's arrays and pinned staging, kept on
// the handle and grown on demand.  Slots [0] r_trg, [1] r_src, [2] n_src, [3] nd rows of Ns x K0, [4] nd rows of Nt x K1.  FORWARD sends `in` (v_src) in [3]
// and returns [4] (v_trg); TRANSPOSE sends `in` (w_trg) in [4] and returns [3] (g_src).  Coordinates and normals go down once, the nd input rows in one
// transfer; the output slot is zeroed, filled by the direction's _device entry (nd == 1: the single-row kernel), comes back in one transfer and is added
// into `out` (the accumulate semantics of GenericKernel::Eval).
int lists_host_call(sctl_amd_lists* p, bool transpose, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* in, void* out, int digits,
                    const void* ctx, int ctx_bytes) {
  const KernelEntry& k = *p->k;
  const size_t rs = real_size(p->real);
  const int slot_out = transpose ? 3 : 4;
  const size_t bytes[5] = {(size_t)p->Nt * 3 * rs, (size_t)p->Ns * 3 * rs, (size_t)p->Ns * k.nd * rs, (size_t)nd * p->Ns * k.k0 * rs, (size_t)nd * p->Nt * k.k1 * rs};
  const void* src[5] = {r_trg, r_src, n_src, transpose ? nullptr : in, transpose ? in : nullptr};
  DeviceScope scope(p->device);
  LISTS_TRY(scope.err);
  if (const int rc = lists_staging(p, bytes, 5)) return rc;
  // the caller's sources ARE its targets (one array): one device copy, which is how the kernel knows that every box meets its own points
  const bool same = r_src == r_trg && bytes[0] == bytes[1];
  Carver cut(p->pinned);
  char* back = nullptr;
  for (int i = 0; i < 5; i++) {
    char* q = cut.take<char>(bytes[i]);
    if (i == slot_out) { back = q; continue; }
    if (!bytes[i] || (i == 1 && same)) continue;
    std::memcpy(q, src[i], bytes[i]);
    LISTS_TRY(hipMemcpyAsync(p->dbuf[i], q, bytes[i], hipMemcpyHostToDevice, p->st));
  }
  LISTS_TRY(hipMemsetAsync(p->dbuf[slot_out], 0, bytes[slot_out], p->st));
  void* const d_src = same ? p->dbuf[0] : p->dbuf[1];
  const int rc = transpose ? sctl_amd_lists_eval_transpose_densities_device(p, nd, p->dbuf[0], d_src, p->dbuf[2], p->dbuf[4], p->dbuf[3], digits, ctx, ctx_bytes, p->st)
                           : sctl_amd_lists_eval_densities_device(p, nd, p->dbuf[0], d_src, p->dbuf[2], p->dbuf[3], p->dbuf[4], digits, ctx, ctx_bytes, p->st);
  if (rc != SCTL_AMD_OK) return rc;
  LISTS_TRY(hipMemcpyAsync(back, p->dbuf[slot_out], bytes[slot_out], hipMemcpyDeviceToHost, p->st));
  LISTS_TRY(hipStreamSynchronize(p->st));
  add_into(p->real, out, back, (int64_t)nd * (transpose ? p->Ns * k.k0 : p->Nt * k.k1));
  return SCTL_AMD_OK;
}
}  // namespace

extern "C" {

int sctl_amd_lists_create_directions(int kernel, int real, int device, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                     const int64_t* src_cnt, int64_t Nt, int64_t Ns, int directions, sctl_amd_lists** out) {
  const KernelEntry* k = registry(kernel);
  if (!k) return set_error(SCTL_AMD_ERR_UNKNOWN_KERNEL, "unknown kernel id");
  if (real != SCTL_AMD_F64 && real != SCTL_AMD_F32) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "real must be SCTL_AMD_F64 or SCTL_AMD_F32");
  if (directions == 0 || (directions & ~(SCTL_AMD_LISTS_FORWARD | SCTL_AMD_LISTS_TRANSPOSE)) != 0)
    return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "directions must be SCTL_AMD_LISTS_FORWARD, SCTL_AMD_LISTS_TRANSPOSE or both");
  if ((directions & SCTL_AMD_LISTS_TRANSPOSE) && !k->lists_t_f64[0])
    return set_error(SCTL_AMD_ERR_UNKNOWN_KERNEL, std::string(k->name) + " has no transposed form (pair_t): its lists can be planned FORWARD only");
  if (!out || nlists < 0 || Nt < 0 || Ns < 0 || (nlists > 0 && (!trg_off || !trg_cnt || !src_off || !src_cnt)))
    return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle pointer, negative size or null list arrays");
  for (int64_t l = 0; l < nlists; l++) {
    if (trg_cnt[l] < 0 || src_cnt[l] < 0 || trg_off[l] < 0 || src_off[l] < 0 || trg_off[l] + trg_cnt[l] > Nt || src_off[l] + src_cnt[l] > Ns)
      return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "list " + std::to_string(l) + " reaches outside the target or source arrays");
  }
  // Each direction checks its own ownership rule only.  The streamed arrays of the forward side are r_src, n_src and v_src, those of the transposed side
  // r_trg and w_trg: the widest of them bounds the 32-bit byte offsets of the packed form.  The gradient kernels (lists_grad_kernel.hpp) stream the same
  // arrays side by side: max(3, ND, K0) reals per point on side 0, max(3, K1) on side 1.
  const int64_t rs = (int64_t)real_size(real);
  SidePlan plans[2];
  if (directions & SCTL_AMD_LISTS_FORWARD) {
    const int rc = plan_side(nlists, trg_off, trg_cnt, src_off, src_cnt, Ns, rs * std::max<int64_t>(3, std::max<int64_t>(k->nd, k->k0)), "target", plans[0]);
    if (rc) return rc;
  }
  if (directions & SCTL_AMD_LISTS_TRANSPOSE) {
    const int rc = plan_side(nlists, src_off, src_cnt, trg_off, trg_cnt, Nt, rs * std::max<int64_t>(3, k->k1), "source", plans[1]);
    if (rc) return rc;
  }

  sctl_amd_lists* p = new sctl_amd_lists;
  p->k = k; p->real = real; p->device = device; p->Nt = Nt; p->Ns = Ns; p->directions = directions;
  for (int d = 0; d < 2; d++) {
    ListsSide& sd = p->side[d];
    const SidePlan& pl = plans[d];
    sd.nitems = (int64_t)pl.items.size(); sd.nranges = (int64_t)pl.ranges.size(); sd.pairs = pl.pairs; sd.nblocks = pl.longest * 8;
    sd.npacked_groups = (int64_t)pl.pgroups.size(); sd.nflat = (int64_t)pl.flat.size();
    std::memcpy(sd.xcd_first, pl.xcd_first, sizeof sd.xcd_first);
  }
  *out = p;
  if (plans[0].items.empty() && plans[1].items.empty()) return SCTL_AMD_OK;       // nothing to do: legal, and needs no device
  const int avail = device_count_quiet();
  if (avail <= 0) { delete p; *out = nullptr; return set_error(SCTL_AMD_ERR_NO_DEVICE, "no HIP device: libsctl_amd has no CPU fallback"); }
  if (device < 0 || device >= avail) { delete p; *out = nullptr; return set_error(SCTL_AMD_ERR_NO_DEVICE, "device index out of range"); }
  DeviceScope scope(device);
  auto fail_hip = [&](hipError_t e, const char* what) {
    sctl_amd_lists_destroy(p);
    *out = nullptr;
    return set_error(SCTL_AMD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  if (scope.err != hipSuccess) return fail_hip(scope.err, "hipSetDevice");
  for (int d = 0; d < 2; d++) {
    ListsSide& sd = p->side[d];
    const SidePlan& pl = plans[d];
    if (pl.items.empty()) continue;
    hipError_t e;
    if ((e = hipMalloc(&sd.d_items, pl.items.size() * sizeof(ListItem))) != hipSuccess) return fail_hip(e, "hipMalloc(items)");
    if ((e = hipMalloc(&sd.d_ranges, pl.ranges.size() * sizeof(ListRange))) != hipSuccess) return fail_hip(e, "hipMalloc(ranges)");
    // the vectors are fresh, written once and alive until the synchronous copies return
    if ((e = hipMemcpy(sd.d_items, pl.items.data(), pl.items.size() * sizeof(ListItem), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy(items)");
    if ((e = hipMemcpy(sd.d_ranges, pl.ranges.data(), pl.ranges.size() * sizeof(ListRange), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy(ranges)");
    if (!pl.pgroups.empty()) {
      if ((e = hipMalloc(&sd.d_groups, pl.pgroups.size() * sizeof(PackedGroup))) != hipSuccess) return fail_hip(e, "hipMalloc(groups)");
      if ((e = hipMalloc(&sd.d_flat, pl.flat.size() * sizeof(uint32_t))) != hipSuccess) return fail_hip(e, "hipMalloc(flat)");
      if ((e = hipMemcpy(sd.d_groups, pl.pgroups.data(), pl.pgroups.size() * sizeof(PackedGroup), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy(groups)");
      if ((e = hipMemcpy(sd.d_flat, pl.flat.data(), pl.flat.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy(flat)");
    }
  }
  return SCTL_AMD_OK;
}

int sctl_amd_lists_create(int kernel, int real, int device, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                          const int64_t* src_cnt, int64_t Nt, int64_t Ns, sctl_amd_lists** out) {
  return sctl_amd_lists_create_directions(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, SCTL_AMD_LISTS_FORWARD, out);
}

void sctl_amd_lists_destroy(sctl_amd_lists* p) {
  if (!p) return;
  bool on_device = p->st || p->pinned;
  for (const ListsSide& sd : p->side) on_device = on_device || sd.d_items || sd.d_ranges || sd.d_groups || sd.d_flat;
  if (on_device) {
    DeviceScope scope(p->device);
    if (scope.err == hipSuccess) {
      if (p->st) (void)hipStreamSynchronize(p->st);
      for (const ListsSide& sd : p->side)
        for (void* b : {sd.d_items, sd.d_ranges, sd.d_groups, sd.d_flat})
          if (b) (void)hipFree(b);
      for (void* b : p->dbuf)
        if (b) (void)hipFree(b);
      if (p->pinned) (void)hipHostFree(p->pinned);
      if (p->st) (void)hipStreamDestroy(p->st);
    }
  }
  delete p;
}

int sctl_amd_lists_info(const sctl_amd_lists* p, int64_t* pairs, int64_t* work_items, int64_t* source_ranges) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (pairs) *pairs = p->side[0].pairs;
  if (work_items) *work_items = p->side[0].nitems;
  if (source_ranges) *source_ranges = p->side[0].nranges;
  return SCTL_AMD_OK;
}

int sctl_amd_lists_transpose_info(const sctl_amd_lists* p, int64_t* pairs, int64_t* work_items, int64_t* target_ranges) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (pairs) *pairs = p->side[1].pairs;
  if (work_items) *work_items = p->side[1].nitems;
  if (target_ranges) *target_ranges = p->side[1].nranges;
  return SCTL_AMD_OK;
}

int sctl_amd_lists_eval_device(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg, int digits,
                               const void* ctx, int ctx_bytes, void* stream) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!(p->directions & SCTL_AMD_LISTS_FORWARD)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the FORWARD direction");
  const ListsSide& fw = p->side[0];
  const KernelEntry& k = *p->k;
  if (const int rc = check_ctx(k, ctx, ctx_bytes)) return rc;
  if (p->side[0].nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !v_src || !v_trg || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or potential array");
  DeviceScope scope(p->device);      // the work list lives on the plan's device: launch there whatever the caller's current device is
  LISTS_TRY(scope.err);
  (void)hipGetLastError();
  const int mode = mode_for(p->real, digits);
  const double scale = k.scale / k.acc_factor[mode];
  with_real(p->real, [&](auto zero) {
    using R = decltype(zero);
    ListArgs<R> a{{0}, (const ListItem*)fw.d_items, (const ListRange*)fw.d_ranges, (const R*)r_trg, (const R*)r_src, (const R*)n_src,
                  (const R*)v_src, (R*)v_trg, (R)scale, make_ctx(k, ctx), (const PackedGroup*)fw.d_groups, (const uint32_t*)fw.d_flat};
    std::memcpy(a.xcd_first, fw.xcd_first, sizeof a.xcd_first);
    if constexpr (std::is_same<R, double>::value) k.lists_f64[mode](a, fw.nblocks, (hipStream_t)stream);
    else k.lists_f32[mode](a, fw.nblocks, (hipStream_t)stream);
    return 0;
  });
  LISTS_TRY(hipGetLastError());
  count_work(fw.pairs, k);
  return SCTL_AMD_OK;
}

int sctl_amd_lists_eval_host(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg, int digits,
                             const void* ctx, int ctx_bytes) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!(p->directions & SCTL_AMD_LISTS_FORWARD)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the FORWARD direction");
  const KernelEntry& k = *p->k;
  if (const int rc = check_ctx(k, ctx, ctx_bytes)) return rc;
  if (p->side[0].nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !v_src || !v_trg || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or potential array");
  return lists_host_call(p, false, 1, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes);
}

// ---- the transposed sum over the lists (sctl_amd_lists_eval_transpose_*, lists_transpose_kernel.hpp) -----------------------------------
// g_src += A^T w_trg over the plan's lists, from the side of the plan whose work items own sources.  Checks and their order are those of
// sctl_amd_lists_eval_*; w_trg has the size of v_trg and g_src the size of v_src, so the handle's device buffers and staging serve both directions.
int sctl_amd_lists_eval_transpose_device(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg, void* g_src, int digits,
                                         const void* ctx, int ctx_bytes, void* stream) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!(p->directions & SCTL_AMD_LISTS_TRANSPOSE)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the TRANSPOSE direction");
  const ListsSide& tr = p->side[1];
  const KernelEntry& k = *p->k;
  if (const int rc = check_ctx(k, ctx, ctx_bytes)) return rc;
  if (tr.nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !w_trg || !g_src || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, weight or result array");
  DeviceScope scope(p->device);
  LISTS_TRY(scope.err);
  (void)hipGetLastError();
  const int mode = mode_for(p->real, digits);
  const double scale = k.scale / k.acc_factor[mode];
  with_real(p->real, [&](auto zero) {
    using R = decltype(zero);
    ListTArgs<R> a{{0}, (const ListItem*)tr.d_items, (const ListRange*)tr.d_ranges, (const R*)r_src, (const R*)n_src, (const R*)r_trg,
                   (const R*)w_trg, (R*)g_src, (R)scale, make_ctx(k, ctx), (const PackedGroup*)tr.d_groups, (const uint32_t*)tr.d_flat};
    std::memcpy(a.xcd_first, tr.xcd_first, sizeof a.xcd_first);
    if constexpr (std::is_same<R, double>::value) k.lists_t_f64[mode](a, tr.nblocks, (hipStream_t)stream);
    else k.lists_t_f32[mode](a, tr.nblocks, (hipStream_t)stream);
    return 0;
  });
  LISTS_TRY(hipGetLastError());
  count_work(tr.pairs, k);
  return SCTL_AMD_OK;
}

int sctl_amd_lists_eval_transpose_host(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg, void* g_src, int digits,
                                       const void* ctx, int ctx_bytes) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (!(p->directions & SCTL_AMD_LISTS_TRANSPOSE)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the TRANSPOSE direction");
  const KernelEntry& k = *p->k;
  if (const int rc = check_ctx(k, ctx, ctx_bytes)) return rc;
  if (p->side[1].nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !w_trg || !g_src || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, weight or result array");
  return lists_host_call(p, true, 1, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes);
}

// one-shot form: plan the transposed side only, evaluate, release
int sctl_amd_eval_lists_transpose_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                       const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                       const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, int device) {
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create_directions(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, SCTL_AMD_LISTS_TRANSPOSE, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_transpose_host(p, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes);
  sctl_amd_lists_destroy(p);
  return rc;
}

// ---- several rows over the lists, either direction (lists_rows_kernel.hpp): several densities (sctl_amd_lists_eval_densities_*) ... -----------------
// The plan is the single-row plan: the same handle serves any nd.
}  // extern "C"

namespace sctl_amd {
namespace {
// Launch table of the several-rows list forms of a direction (Dir: ListFwd, ListTrans): the built-in kernels only; a registered plugin kernel has none
// (null) and runs its rows one at a time.
template <class Dir> const ListsRowsEntry<Dir>* multi_entry(int kernel_id) {
  if (kernel_id < 0 || kernel_id >= SCTL_AMD_NUM_KERNELS) return nullptr;
  if constexpr (Dir::SIDE == 0) {
    static const ListsMultiEntry* tab[SCTL_AMD_NUM_KERNELS] = {
        &lmulti_Laplace3D_FxU(), &lmulti_Laplace3D_DxU(), &lmulti_Laplace3D_FxdU(),  &lmulti_Stokes3D_FxU(),      &lmulti_Stokes3D_DxU(),
        &lmulti_Stokes3D_FxT(),  &lmulti_Stokes3D_FSxU(), &lmulti_Stokes3D_FxUP(), &lmulti_Laplace3D_FDxUdU(), &lmulti_Helmholtz3D_FxU()};
    return tab[kernel_id];
  } else {
    static const ListsMultiTEntry* tab[SCTL_AMD_NUM_KERNELS] = {
        &ltmulti_Laplace3D_FxU(), &ltmulti_Laplace3D_DxU(), &ltmulti_Laplace3D_FxdU(),  &ltmulti_Stokes3D_FxU(),      &ltmulti_Stokes3D_DxU(),
        &ltmulti_Stokes3D_FxT(),  &ltmulti_Stokes3D_FSxU(), &ltmulti_Stokes3D_FxUP(), &ltmulti_Laplace3D_FDxUdU(), &ltmulti_Helmholtz3D_FxU()};
    return tab[kernel_id];
  }
}
template <class Dir, class R> ListsRowsLaunch<Dir, R> multi_launch(const ListsRowsEntry<Dir>& me, int mode, int form) {
  if constexpr (std::is_same<R, double>::value) return me.f64[mode][form];
  else return me.f32[mode][form];
}
// the form for `left` >= 2 rows still to do: the narrowest that takes them all, else the widest; -1: none (the single-row kernel)
template <class Dir, class R> int multi_form(const ListsRowsEntry<Dir>* me, int mode, int left) {
  if (!me || left < 2) return -1;
  int widest = -1;
  for (int i = 0; i < kNumListRowsM; i++) {
    if (!multi_launch<Dir, R>(*me, mode, i)) continue;
    if (kListRowsM[i] >= left) return i;
    widest = i;
  }
  return widest;
}

// (the two entries check in different orders: the context comes last forward, right after the handle transposed)
int check_lists_densities(const sctl_amd_lists* p, int nd, const void* ctx, int ctx_bytes) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  if (!(p->directions & SCTL_AMD_LISTS_FORWARD)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the FORWARD direction");
  const KernelEntry& k = *p->k;
  if (const int rc = check_ctx(k, ctx, ctx_bytes)) return rc;
  return SCTL_AMD_OK;
}
int check_lists_transpose_densities(const sctl_amd_lists* p, int nd, const void* ctx, int ctx_bytes) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  if (const int rc = check_ctx(*p->k, ctx, ctx_bytes)) return rc;
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  if (!(p->directions & SCTL_AMD_LISTS_TRANSPOSE)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "this plan was not made for the TRANSPOSE direction");
  return SCTL_AMD_OK;
}

// nd >= 2 rows, row-major, on the plan's device: passes of the widest form, then the narrowest form that holds the rest; one row left over (and every
// row of a plugin kernel) takes the single-row kernel of the direction on the same stream.  FORWARD: in = v_src (rows of Ns x K0), out = v_trg (rows of
// Nt x K1); TRANSPOSE: in = w_trg (rows of Nt x K1), out = g_src (rows of Ns x K0).  out is accumulated into.
template <class Dir, class R>
int lists_eval_rows(sctl_amd_lists* p, int nd, const R* xt, const R* xs, const R* xn, const R* in, R* out, int digits, const void* ctx, int ctx_bytes, hipStream_t st) {
  constexpr bool transpose = Dir::SIDE == 1;
  const KernelEntry& k = *p->k;
  const ListsSide& sd = p->side[Dir::SIDE];
  const int64_t in_stride = transpose ? p->Nt * k.k1 : p->Ns * k.k0, out_stride = transpose ? p->Ns * k.k0 : p->Nt * k.k1;
  const ListsRowsEntry<Dir>* me = multi_entry<Dir>(k.id);
  const int mode = mode_for(p->real, digits);
  for (int m0 = 0; m0 < nd;) {
    const R* const in0 = in + m0 * in_stride;
    R* const out0 = out + m0 * out_stride;
    const int form = multi_form<Dir, R>(me, mode, nd - m0);
    if (form < 0) {
      const int rc = transpose ? sctl_amd_lists_eval_transpose_device(p, xt, xs, xn, in0, out0, digits, ctx, ctx_bytes, st)
                               : sctl_amd_lists_eval_device(p, xt, xs, xn, in0, out0, digits, ctx, ctx_bytes, st);
      if (rc) return rc;
      m0++;
      continue;
    }
    const int M = kListRowsM[form], nact = nd - m0 < M ? nd - m0 : M;
    (void)hipGetLastError();
    const R scale = (R)(k.scale / k.acc_factor[mode]);
    typename Dir::template Args<R> a{};
    if constexpr (transpose)
      a.l = ListTArgs<R>{{0}, (const ListItem*)sd.d_items, (const ListRange*)sd.d_ranges, xs, xn, xt, in0, out0, scale, make_ctx(k, ctx), (const PackedGroup*)sd.d_groups, (const uint32_t*)sd.d_flat};
    else
      a.l = ListArgs<R>{{0}, (const ListItem*)sd.d_items, (const ListRange*)sd.d_ranges, xt, xs, xn, in0, out0, scale, make_ctx(k, ctx), (const PackedGroup*)sd.d_groups, (const uint32_t*)sd.d_flat};
    std::memcpy(a.l.xcd_first, sd.xcd_first, sizeof a.l.xcd_first);
    a.in_stride = in_stride; a.out_stride = out_stride; a.nact = nact;
    multi_launch<Dir, R>(*me, mode, form)(a, sd.nblocks, st);
    LISTS_TRY(hipGetLastError());
    count_work(sd.pairs * nact, k);
    m0 += nact;
  }
  return SCTL_AMD_OK;
}
}  // namespace
}  // namespace sctl_amd

extern "C" {

int sctl_amd_lists_eval_densities_device(sctl_amd_lists* p, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg,
                                         int digits, const void* ctx, int ctx_bytes, void* stream) {
  const int rc = check_lists_densities(p, nd, ctx, ctx_bytes);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_lists_eval_device(p, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, stream);
  if (nd == 0 || p->side[0].nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !v_src || !v_trg || (p->k->nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or potential array");
  DeviceScope scope(p->device);      // the work list lives on the plan's device
  LISTS_TRY(scope.err);
  return with_real(p->real, [&](auto zero) { using R = decltype(zero); return lists_eval_rows<ListFwd, R>(p, nd, (const R*)r_trg, (const R*)r_src, (const R*)n_src, (const R*)v_src, (R*)v_trg, digits, ctx, ctx_bytes, (hipStream_t)stream); });
}

// (the handle's device buffers and pinned block are the single-density entry's, grown to nd rows on demand: lists_host_call)
int sctl_amd_lists_eval_densities_host(sctl_amd_lists* p, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, void* v_trg,
                                       int digits, const void* ctx, int ctx_bytes) {
  const int rc0 = check_lists_densities(p, nd, ctx, ctx_bytes);
  if (rc0) return rc0;
  if (nd == 1) return sctl_amd_lists_eval_host(p, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes);
  if (nd == 0 || p->side[0].nitems == 0) return SCTL_AMD_OK;
  const KernelEntry& k = *p->k;
  if (!r_trg || !r_src || !v_src || !v_trg || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or potential array");
  return lists_host_call(p, false, nd, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes);
}

int sctl_amd_eval_lists_densities_host(int kernel, int real, int nd, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                       const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src,
                                       const void* v_src, void* v_trg, int digits, const void* ctx, int ctx_bytes, int device) {
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_densities_host(p, nd, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes);
  sctl_amd_lists_destroy(p);
  return rc;
}

// ---- ... and several weight vectors through the transposed sum (sctl_amd_lists_eval_transpose_densities_*) ------------------------------------------
int sctl_amd_lists_eval_transpose_densities_device(sctl_amd_lists* p, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg,
                                                   void* g_src, int digits, const void* ctx, int ctx_bytes, void* stream) {
  const int rc = check_lists_transpose_densities(p, nd, ctx, ctx_bytes);
  if (rc) return rc;
  if (nd == 1) return sctl_amd_lists_eval_transpose_device(p, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes, stream);
  if (nd == 0 || p->side[1].nitems == 0) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !w_trg || !g_src || (p->k->nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, weight or result array");
  DeviceScope scope(p->device);      // the work list lives on the plan's device
  LISTS_TRY(scope.err);
  return with_real(p->real, [&](auto zero) { using R = decltype(zero); return lists_eval_rows<ListTrans, R>(p, nd, (const R*)r_trg, (const R*)r_src, (const R*)n_src, (const R*)w_trg, (R*)g_src, digits, ctx, ctx_bytes, (hipStream_t)stream); });
}

int sctl_amd_lists_eval_transpose_densities_host(sctl_amd_lists* p, int nd, const void* r_trg, const void* r_src, const void* n_src, const void* w_trg,
                                                 void* g_src, int digits, const void* ctx, int ctx_bytes) {
  const int rc0 = check_lists_transpose_densities(p, nd, ctx, ctx_bytes);
  if (rc0) return rc0;
  if (nd == 1) return sctl_amd_lists_eval_transpose_host(p, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes);
  if (nd == 0 || p->side[1].nitems == 0) return SCTL_AMD_OK;
  const KernelEntry& k = *p->k;
  if (!r_trg || !r_src || !w_trg || !g_src || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, weight or result array");
  return lists_host_call(p, true, nd, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes);
}

int sctl_amd_eval_lists_transpose_densities_host(int kernel, int real, int nd, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt,
                                                 const int64_t* src_off, const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src,
                                                 const void* n_src, const void* w_trg, void* g_src, int digits, const void* ctx, int ctx_bytes, int device) {
  if (nd < 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "negative number of densities");
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create_directions(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, SCTL_AMD_LISTS_TRANSPOSE, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_transpose_densities_host(p, nd, r_trg, r_src, n_src, w_trg, g_src, digits, ctx, ctx_bytes);
  sctl_amd_lists_destroy(p);
  return rc;
}

// one-shot forms: plan, evaluate, release
int sctl_amd_eval_lists_device(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                               const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                               void* v_trg, int digits, const void* ctx, int ctx_bytes, void* stream) {
  int dev = 0;
  if (device_count_quiet() > 0 && hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create(kernel, real, dev, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_device(p, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes, stream);
  if (rc == SCTL_AMD_OK && p->side[0].nitems > 0 && hipStreamSynchronize((hipStream_t)stream) != hipSuccess)   // the work list is freed below
    rc = set_error(SCTL_AMD_ERR_HIP, "hipStreamSynchronize failed after the list evaluation");
  sctl_amd_lists_destroy(p);
  return rc;
}

int sctl_amd_eval_lists_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                             const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                             void* v_trg, int digits, const void* ctx, int ctx_bytes, int device) {
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_host(p, r_trg, r_src, n_src, v_src, v_trg, digits, ctx, ctx_bytes);
  sctl_amd_lists_destroy(p);
  return rc;
}

}  // extern "C"

// ---- geometry gradients over the lists (sctl_amd_lists_eval_grad_*, include/sctl_amd/device/lists_grad_kernel.hpp) ------------------------------------
// g_trg from the plan's FORWARD side (its work items own targets), g_src and g_nrm from its TRANSPOSE side (they own sources): one launch per side, only
// for the sides whose outputs are asked for.
namespace sctl_amd {
namespace {
// the launch table of a built-in kernel; null for a registered plugin kernel
const ListsGradEntry* lists_grad_entry(int kernel_id) {
  if (kernel_id < 0 || kernel_id >= SCTL_AMD_NUM_KERNELS) return nullptr;
  static const ListsGradEntry* tab[SCTL_AMD_NUM_KERNELS] = {
      &lists_grad_Laplace3D_FxU(), &lists_grad_Laplace3D_DxU(), &lists_grad_Laplace3D_FxdU(),  &lists_grad_Stokes3D_FxU(),      &lists_grad_Stokes3D_DxU(),
      &lists_grad_Stokes3D_FxT(),  &lists_grad_Stokes3D_FSxU(), &lists_grad_Stokes3D_FxUP(), &lists_grad_Laplace3D_FDxUdU(), &lists_grad_Helmholtz3D_FxU()};
  return tab[kernel_id];
}

// the checks both entries make, in the order of sctl_amd_lists_eval_transpose_*: the handle, the directions, the context
int check_lists_grad(const sctl_amd_lists* p, const void* g_trg, const void* g_src, const void* g_nrm, const void* ctx, int ctx_bytes) {
  if (!p) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null handle");
  const KernelEntry& k = *p->k;
  if (!lists_grad_entry(k.id))
    return set_error(SCTL_AMD_ERR_UNKNOWN_KERNEL, std::string(k.name) + " is a plugin kernel: gradients over lists are built for the built-in kernels only");
  if (g_trg && !(p->directions & SCTL_AMD_LISTS_FORWARD))
    return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "g_trg comes from the FORWARD direction, which this plan was not made for: plan with SCTL_AMD_LISTS_FORWARD");
  if ((g_src || g_nrm) && !(p->directions & SCTL_AMD_LISTS_TRANSPOSE))
    return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "g_src and g_nrm come from the TRANSPOSE direction, which this plan was not made for: plan with SCTL_AMD_LISTS_TRANSPOSE");
  if (g_nrm && k.nd == 0) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, std::string(k.name) + " has no source normal: g_nrm must be null");
  return check_ctx(k, ctx, ctx_bytes);
}
// does side d of the plan have anything to launch for these outputs
bool lists_grad_side(const sctl_amd_lists* p, int d, const void* g_trg, const void* g_src, const void* g_nrm) {
  return (d == 0 ? g_trg != nullptr : (g_src || g_nrm)) && p->side[d].nitems > 0;
}

// The host-pointer form, after the entry's checks: lists_host_call's slots [0 .. 4] carry the five inputs down, [5 .. 7] bring the wanted outputs back.
int lists_grad_host_call(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, const void* w_trg, void* g_trg,
                         void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes) {
  const KernelEntry& k = *p->k;
  const size_t rs = real_size(p->real);
  void* const out[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, g_trg, g_src, g_nrm};
  const void* const src[5] = {r_trg, r_src, n_src, v_src, w_trg};
  const int64_t out_n[8] = {0, 0, 0, 0, 0, p->Nt * 3, p->Ns * 3, p->Ns * 3};
  size_t bytes[8] = {(size_t)p->Nt * 3 * rs, (size_t)p->Ns * 3 * rs, (size_t)p->Ns * k.nd * rs, (size_t)p->Ns * k.k0 * rs, (size_t)p->Nt * k.k1 * rs, 0, 0, 0};
  for (int i = 5; i < 8; i++) bytes[i] = out[i] ? (size_t)out_n[i] * rs : 0;
  DeviceScope scope(p->device);
  LISTS_TRY(scope.err);
  if (const int rc = lists_staging(p, bytes, 8)) return rc;
  const bool same = r_src == r_trg && bytes[0] == bytes[1];   // one array: one device copy, which is how the kernel knows that every box meets its own points
  Carver cut(p->pinned);
  char* back[8] = {};
  for (int i = 0; i < 8; i++) {
    char* q = cut.take<char>(bytes[i]);
    if (!bytes[i] || (i == 1 && same)) continue;
    if (i >= 5) {
      back[i] = q;
      LISTS_TRY(hipMemsetAsync(p->dbuf[i], 0, bytes[i], p->st));
    } else {
      std::memcpy(q, src[i], bytes[i]);
      LISTS_TRY(hipMemcpyAsync(p->dbuf[i], q, bytes[i], hipMemcpyHostToDevice, p->st));
    }
  }
  const int rc = sctl_amd_lists_eval_grad_device(p, p->dbuf[0], same ? p->dbuf[0] : p->dbuf[1], p->dbuf[2], p->dbuf[3], p->dbuf[4], g_trg ? p->dbuf[5] : nullptr,
                                                 g_src ? p->dbuf[6] : nullptr, g_nrm ? p->dbuf[7] : nullptr, digits, ctx, ctx_bytes, p->st);
  if (rc != SCTL_AMD_OK) return rc;
  for (int i = 5; i < 8; i++)
    if (back[i]) LISTS_TRY(hipMemcpyAsync(back[i], p->dbuf[i], bytes[i], hipMemcpyDeviceToHost, p->st));
  LISTS_TRY(hipStreamSynchronize(p->st));
  for (int i = 5; i < 8; i++)
    if (back[i]) add_into(p->real, out[i], back[i], out_n[i]);
  return SCTL_AMD_OK;
}
}  // namespace
}  // namespace sctl_amd

extern "C" {

int sctl_amd_lists_eval_grad_device(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, const void* w_trg, void* g_trg,
                                    void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes, void* stream) {
  if (const int rc = check_lists_grad(p, g_trg, g_src, g_nrm, ctx, ctx_bytes)) return rc;
  const bool run[2] = {lists_grad_side(p, 0, g_trg, g_src, g_nrm), lists_grad_side(p, 1, g_trg, g_src, g_nrm)};
  if (!run[0] && !run[1]) return SCTL_AMD_OK;
  const KernelEntry& k = *p->k;
  if (!r_trg || !r_src || !v_src || !w_trg || (k.nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or weight array");
  const ListsGradEntry& ge = *lists_grad_entry(k.id);
  DeviceScope scope(p->device);      // the work lists live on the plan's device
  LISTS_TRY(scope.err);
  const int mode = mode_for(p->real, digits);
  const double scale = k.scale / ge.grad_factor[mode];
  for (int d = 0; d < 2; d++) {
    if (!run[d]) continue;
    const ListsSide& sd = p->side[d];
    (void)hipGetLastError();
    with_real(p->real, [&](auto zero) {
      using R = decltype(zero);
      ListGArgs<R> a{{0}, (const ListItem*)sd.d_items, (const ListRange*)sd.d_ranges, (const R*)(d ? r_src : r_trg), (const R*)(d ? r_trg : r_src), (const R*)n_src,
                     (const R*)v_src, (const R*)w_trg, (R*)(d ? g_src : g_trg), (R*)(d ? g_nrm : nullptr), (R)scale, make_ctx(k, ctx),
                     (const PackedGroup*)sd.d_groups, (const uint32_t*)sd.d_flat};
      std::memcpy(a.xcd_first, sd.xcd_first, sizeof a.xcd_first);
      if constexpr (std::is_same<R, double>::value) ge.f64[mode][d](a, sd.nblocks, (hipStream_t)stream);
      else ge.f32[mode][d](a, sd.nblocks, (hipStream_t)stream);
      return 0;
    });
    LISTS_TRY(hipGetLastError());
    count_work(sd.pairs, k);
  }
  return SCTL_AMD_OK;
}

int sctl_amd_lists_eval_grad_host(sctl_amd_lists* p, const void* r_trg, const void* r_src, const void* n_src, const void* v_src, const void* w_trg, void* g_trg,
                                  void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes) {
  if (const int rc = check_lists_grad(p, g_trg, g_src, g_nrm, ctx, ctx_bytes)) return rc;
  if (!lists_grad_side(p, 0, g_trg, g_src, g_nrm) && !lists_grad_side(p, 1, g_trg, g_src, g_nrm)) return SCTL_AMD_OK;
  if (!r_trg || !r_src || !v_src || !w_trg || (p->k->nd > 0 && !n_src)) return set_error(SCTL_AMD_ERR_BAD_ARGUMENT, "null coordinate, normal, density or weight array");
  return lists_grad_host_call(p, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits, ctx, ctx_bytes);
}

// one-shot form: plan both directions, evaluate, release
int sctl_amd_eval_lists_grad_host(int kernel, int real, int64_t nlists, const int64_t* trg_off, const int64_t* trg_cnt, const int64_t* src_off,
                                  const int64_t* src_cnt, int64_t Nt, int64_t Ns, const void* r_trg, const void* r_src, const void* n_src, const void* v_src,
                                  const void* w_trg, void* g_trg, void* g_src, void* g_nrm, int digits, const void* ctx, int ctx_bytes, int device) {
  sctl_amd_lists* p = nullptr;
  int rc = sctl_amd_lists_create_directions(kernel, real, device, nlists, trg_off, trg_cnt, src_off, src_cnt, Nt, Ns,
                                            SCTL_AMD_LISTS_FORWARD | SCTL_AMD_LISTS_TRANSPOSE, &p);
  if (rc != SCTL_AMD_OK) return rc;
  rc = sctl_amd_lists_eval_grad_host(p, r_trg, r_src, n_src, v_src, w_trg, g_trg, g_src, g_nrm, digits, ctx, ctx_bytes);
  sctl_amd_lists_destroy(p);
  return rc;
}

}  // extern "C"
