// wal_merge.hpp — the device half of a WAL block refresh: the new block's columns written
// from the old block's columns, a small delta and one renumbering table per key
// (wal_merge.hip; planned by block.cpp plan_wal_refresh, driven by devctx.hip block_refresh).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsg {

// One output column (or column group) of the merge. Every pointer is device memory.
struct WalMergeJob {
  enum Kind : uint32_t {
    kScan = 0,   // [dur32 | start_s | end_s | ds]: four u32 columns, src_stride / dst_stride entries apart
    kCopy = 1,   // a cold column of `wn` bytes per entry (1, 8 or 16), copied as it is
    kNames = 2,  // {svc vid, name vid} pairs, each half through its table (lut / lut2, null: unchanged)
    kTerm = 3,   // a term column: `wo` bytes per old entry (0: the key is new, every old entry absent)
                 // through lut (lut_n entries, null: unchanged) to `wn` bytes; all-ones stays all-ones
  };
  const void *src;       // the old block's column
  void *dst;             // the new block's
  const void *delta;     // the delta entries' values in the new block's form (kTerm: u32 per entry)
  const uint32_t *lut, *lut2;
  uint32_t kind, wo, wn;
  uint32_t lut_n, lut2_n;  // entries of lut / lut2 (an id at or above it reads as absent)
  uint32_t pad_;
  uint64_t src_stride, dst_stride;  // (kScan)
};

struct WalMergeArgs {
  const WalMergeJob *jobs;
  uint32_t njobs;
  // delta entry d lands at scan position dpos[d] (ascending); dins[d] = inserts among the delta
  // entries before d (ndelta + 1 values): a position j that is no delta entry's reads old
  // entry j - dins[c], c = delta entries placed before j
  const uint32_t *dpos, *dins;
  uint32_t ndelta;
  uint64_t n_old, n_new;
  uint64_t npad;  // scan and term columns are written to here (the padding: 0, one-byte columns all-ones)
};

void wal_merge_launch(const WalMergeArgs &a, hipStream_t s);

}  // namespace tsg
