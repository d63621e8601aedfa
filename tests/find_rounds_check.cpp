// The round planner of tsg_find_ids over on-demand blocks (tempo_amd/csrc/find_rounds.hpp) as a
// stand-alone program: tests/test_find_rounds.py drives it and compares its lines with a model.
//
//   find_rounds_check CAP [LEN ...]     the plan of pages of those lengths under a staging cap of CAP
//     bytes (0: the default): one line "first count bytes" per round, then one line of the pages'
//     offsets ("-" when there is no page)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "find_rounds.hpp"

int main(int argc, char **argv) {
  using namespace tsg;
  if (argc < 2) return 2;
  const uint64_t cap = std::strtoull(argv[1], nullptr, 10);
  std::vector<uint32_t> len;
  for (int i = 2; i < argc; i++) len.push_back(uint32_t(std::strtoul(argv[i], nullptr, 10)));
  FindRoundPlan plan;
  plan_find_rounds(len.data(), len.size(), cap, plan);
  for (const FindRound &r : plan.rounds) std::printf("%u %u %" PRIu64 "\n", r.first, r.count, r.bytes);
  if (plan.offsets.size() != len.size()) return 3;
  if (len.empty()) std::printf("-");
  for (size_t i = 0; i < plan.offsets.size(); i++) std::printf("%s%" PRIu64, i ? " " : "", plan.offsets[i]);
  std::printf("\n");
  return 0;
}
