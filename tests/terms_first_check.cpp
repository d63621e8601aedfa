// The terms-first planner's host arithmetic (tempo_amd/csrc/terms_first.hpp) as a stand-alone
// program: tests/test_terms_first_plan.py drives it and compares its lines with numpy.
//
//   terms_first_check count NSETS V0 V1 ...     the per-set counts of a column (4294967295 = absent)
//   terms_first_check plan MODE < blocks        the launch's p, its share of steps and the choice;
//     one block per line: entries scanned nterms, then per term: ncounts (0: no counts), the
//     counts, the eight bitmap words
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "terms_first.hpp"

int main(int argc, char **argv) {
  using namespace tsg;
  if (argc >= 3 && !std::strcmp(argv[1], "count")) {
    const uint32_t ns = uint32_t(std::strtoul(argv[2], nullptr, 10));
    std::vector<uint32_t> col, out(ns ? ns : 1);
    for (int i = 3; i < argc; i++) col.push_back(uint32_t(std::strtoul(argv[i], nullptr, 10)));
    count_sets(col.data(), col.size(), ns, out.data());
    for (uint32_t s = 0; s < ns; s++) std::printf("%u%c", out[s], s + 1 < ns ? ' ' : '\n');
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "plan")) {
    const int mode = std::atoi(argv[2]);
    std::vector<TermsFirstBlock> blk;
    std::vector<std::vector<uint32_t>> keep;
    unsigned long long entries, scanned;
    unsigned nterms;
    while (std::scanf("%llu %llu %u", &entries, &scanned, &nterms) == 3) {
      TermsFirstBlock b{};
      b.entries = entries;
      b.scanned = scanned;
      b.nterms = nterms;
      for (unsigned t = 0; t < nterms && t < 4; t++) {
        unsigned nc;
        if (std::scanf("%u", &nc) != 1) return 2;
        std::vector<uint32_t> c(nc), bm(8);
        for (auto &x : c)
          if (std::scanf("%" SCNu32, &x) != 1) return 2;
        for (auto &x : bm)
          if (std::scanf("%" SCNu32, &x) != 1) return 2;
        keep.push_back(std::move(c));
        keep.push_back(std::move(bm));
        b.ncounts[t] = nc;
      }
      blk.push_back(b);
    }
    size_t at = 0;
    for (auto &b : blk)  // (the vectors no longer move)
      for (unsigned t = 0; t < b.nterms && t < 4; t++, at += 2) {
        b.counts[t] = b.ncounts[t] ? keep[at].data() : nullptr;
        b.bitmap[t] = keep[at + 1].data();
      }
    const double p = terms_first_p(blk.data(), blk.size());
    std::printf("%.17g %.17g %d %.17g\n", p, p < 0 ? -1.0 : terms_first_share(p), int(terms_first_pick(mode, p)),
                kTermsFirstMaxShare);
    return 0;
  }
  return 2;
}
