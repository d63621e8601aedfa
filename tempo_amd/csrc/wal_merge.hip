// wal_merge.hip — wal_merge_kernel: a refreshed WAL block's columns written on the device
// from the block it follows (tsg_wal_block_refresh; DESIGN.md §3 "Refreshing a WAL block").
//
// The new block is the old one with a few entries inserted at their sorted positions and a few
// replaced (a page whose id the block already held, combined on the host). Every output entry
// finds its source with one binary search over the delta's positions, so the kernel is a
// streaming copy: each old column is read once (non-temporal: it is not read again), each new
// column is written once, consecutive lanes write consecutive entries. Term columns pass
// through the key's renumbering table on the way (the dictionaries of keys that stay narrow
// are renumbered canonically when values join them) and widen where the key outgrew its width.
//
// Grid: x = runs of kRun entries, y = one job per column (WalMergeJob). A workgroup stages the
// delta's positions in LDS when they fit (kLdsDelta; larger deltas are searched in global
// memory, where the few hot levels of the search stay in cache) and a one-byte column's table
// (at most 256 entries). Plain vector loads and stores only; no workgroup waits for another.
#include "wal_merge.hpp"

#include "devctx.hpp"

namespace tsg {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRun = 8 * kThreads;  // entries per workgroup
constexpr uint32_t kLdsDelta = 2048;     // delta entries staged in LDS (16 KiB + 4 B)

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

template <class T>
__device__ inline T load_once(const void *base, uint64_t i) {
  return __builtin_nontemporal_load(static_cast<const T *>(base) + i);
}

__global__ __launch_bounds__(kThreads) void wal_merge_kernel(const WalMergeArgs a) {
  __shared__ uint32_t s_pos[kLdsDelta], s_ins[kLdsDelta + 1], s_lut[256];
  const uint32_t tid = threadIdx.x;
  const WalMergeJob J = a.jobs[blockIdx.y];
  const uint32_t nd = a.ndelta;
  const bool staged = nd <= kLdsDelta;
  if (staged) {
    for (uint32_t i = tid; i < nd; i += kThreads) s_pos[i] = a.dpos[i];
    for (uint32_t i = tid; i <= nd; i += kThreads) s_ins[i] = a.dins[i];
  }
  const bool lut_staged = J.kind == WalMergeJob::kTerm && J.wo == 1 && J.lut != nullptr;
  if (lut_staged) s_lut[tid] = tid < J.lut_n ? J.lut[tid] : 0xffffffffu;
  __syncthreads();
  const uint32_t *pos = staged ? s_pos : a.dpos;
  const uint32_t *ins = staged ? s_ins : a.dins;
  const bool padded = J.kind == WalMergeJob::kScan || J.kind == WalMergeJob::kTerm;
  const uint64_t end = padded ? a.npad : a.n_new;
  const uint64_t j0 = uint64_t(blockIdx.x) * kRun + tid;
  for (uint32_t t = 0; t < kRun / kThreads; t++) {
    const uint64_t j = j0 + uint64_t(t) * kThreads;
    if (j >= end) break;
    // the entry's source: delta entry `idx`, old entry `idx`, or none (the columns' padding)
    bool none = j >= a.n_new, from_delta = false;
    uint64_t idx = 0;
    if (!none) {
      uint32_t lo = 0, hi = nd;
      while (lo < hi) {  // delta entries placed before j
        const uint32_t m = (lo + hi) >> 1;
        if (pos[m] < j) lo = m + 1;
        else hi = m;
      }
      if (lo < nd && pos[lo] == j) {
        from_delta = true;
        idx = lo;
      } else {
        idx = j - ins[lo];
        none = idx >= a.n_old;  // (never for a plan that adds up: nothing is read out of bounds)
      }
    }
    switch (J.kind) {
      case WalMergeJob::kScan: {
        uint32_t *dst = static_cast<uint32_t *>(J.dst);
        const uint32_t *dl = static_cast<const uint32_t *>(J.delta);
        for (uint32_t c = 0; c < 4; c++) {
          uint32_t v = 0;
          if (!none) v = from_delta ? dl[uint64_t(c) * nd + idx] : load_once<uint32_t>(J.src, c * J.src_stride + idx);
          dst[c * J.dst_stride + j] = v;
        }
        break;
      }
      case WalMergeJob::kCopy: {
        const void *src = from_delta ? J.delta : J.src;
        if (J.wn == 16) {
          v4u v = {0, 0, 0, 0};
          if (!none) v = from_delta ? static_cast<const v4u *>(src)[idx] : load_once<v4u>(src, idx);
          static_cast<v4u *>(J.dst)[j] = v;
        } else if (J.wn == 8) {
          uint64_t v = 0;
          if (!none) v = from_delta ? static_cast<const uint64_t *>(src)[idx] : load_once<uint64_t>(src, idx);
          static_cast<uint64_t *>(J.dst)[j] = v;
        } else {
          uint8_t v = 0;
          if (!none) v = from_delta ? static_cast<const uint8_t *>(src)[idx] : load_once<uint8_t>(src, idx);
          static_cast<uint8_t *>(J.dst)[j] = v;
        }
        break;
      }
      case WalMergeJob::kNames: {
        v2u v = {0xffffffffu, 0xffffffffu};
        if (!none) {
          if (from_delta) {
            v = static_cast<const v2u *>(J.delta)[idx];
          } else {
            v = load_once<v2u>(J.src, idx);
            if (J.lut && v.x != 0xffffffffu) v.x = v.x < J.lut_n ? J.lut[v.x] : 0xffffffffu;
            if (J.lut2 && v.y != 0xffffffffu) v.y = v.y < J.lut2_n ? J.lut2[v.y] : 0xffffffffu;
          }
        }
        static_cast<v2u *>(J.dst)[j] = v;
        break;
      }
      default: {  // kTerm
        uint32_t v;
        if (none) {
          v = J.wn == 1 ? 0xffu : 0u;
        } else if (from_delta) {
          v = static_cast<const uint32_t *>(J.delta)[idx];  // (absent = all-ones at every width)
        } else if (J.wo == 0) {
          v = 0xffffffffu;
        } else {
          uint32_t o, ones;
          if (J.wo == 1) {
            o = load_once<uint8_t>(J.src, idx);
            ones = 0xffu;
          } else if (J.wo == 2) {
            o = load_once<uint16_t>(J.src, idx);
            ones = 0xffffu;
          } else {
            o = load_once<uint32_t>(J.src, idx);
            ones = 0xffffffffu;
          }
          if (o == ones) v = 0xffffffffu;
          else if (!J.lut) v = o;
          else if (lut_staged) v = s_lut[o];
          else v = o < J.lut_n ? J.lut[o] : 0xffffffffu;
        }
        if (J.wn == 1) static_cast<uint8_t *>(J.dst)[j] = uint8_t(v);
        else if (J.wn == 2) static_cast<uint16_t *>(J.dst)[j] = uint16_t(v);
        else static_cast<uint32_t *>(J.dst)[j] = v;
        break;
      }
    }
  }
}

}  // namespace

void wal_merge_launch(const WalMergeArgs &a, hipStream_t s) {
  if (!a.njobs) return;
  const uint64_t runs = (a.npad + kRun - 1) / kRun;
  if (runs == 0 || runs > 0x7fffffffull || a.njobs > 65535) fail(TSG_E_UNSUPPORTED, "wal merge: launch shape out of range");
  hipLaunchKernelGGL(wal_merge_kernel, dim3(uint32_t(runs), a.njobs), dim3(kThreads), 0, s, a);
  HIP_OK(hipGetLastError());
}

}  // namespace tsg
