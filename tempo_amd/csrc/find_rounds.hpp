// find_rounds.hpp — how tsg_find_ids stages the hit pages of blocks whose data file stays on disk
// (TSG_V2_DATA_ON_DEMAND; find.hip device_find). No HIP in here: tests/find_rounds_check.cpp
// drives it on the host.
//
// The on-demand pages of a batch, in the batch's page order, are cut into rounds. A round's pages
// are read from their files into one staging buffer, each at a 16-byte aligned offset, copied to
// the device and run through the size / decode / scan / gather kernels before the next round
// reuses the buffer. A round is a maximal run of pages whose packed bytes (the last page's end)
// fit the staging cap; a page longer than the cap is a round of its own (the buffer grows for
// it). No on-demand page at all is one empty round: the caller's resident pages ride in round 0.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tsg {

constexpr uint64_t kFindStageDefault = uint64_t(256) << 20;  // the staging cap (bytes) unless set
constexpr uint64_t kFindStageAlign = 16;
// test hook (tsg_debug_set "find_stage_bytes"): the cap in bytes, 0 = TSG_FIND_STAGE_BYTES or the default
inline std::atomic<uint64_t> g_find_stage_bytes{0};

struct FindRound {
  uint32_t first, count;  // pages [first, first + count) of the list planned
  uint64_t bytes;         // the staging bytes they fill: the last page's offset + its length
};
struct FindRoundPlan {
  std::vector<FindRound> rounds;  // never empty
  std::vector<uint64_t> offsets;  // per page: its offset in its round's staging buffer
};

inline void plan_find_rounds(const uint32_t *len, size_t n, uint64_t cap, FindRoundPlan &plan) {
  plan.rounds.clear();
  plan.offsets.assign(n, 0);
  if (cap == 0) cap = kFindStageDefault;
  FindRound cur{0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    uint64_t off = (cur.bytes + kFindStageAlign - 1) / kFindStageAlign * kFindStageAlign;
    if (cur.count && off + len[i] > cap) {  // (a round's first page always fits: the buffer grows)
      plan.rounds.push_back(cur);
      cur = FindRound{uint32_t(i), 0, 0};
      off = 0;
    }
    plan.offsets[i] = off;
    cur.count++;
    cur.bytes = off + len[i];
  }
  plan.rounds.push_back(cur);
}

}  // namespace tsg
