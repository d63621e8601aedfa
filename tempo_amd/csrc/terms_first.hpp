// terms_first.hpp — the host's choice between the narrow kernels' two modes (pool_kernels.hpp:
// terms first reads the packed scan word only where an entry passed every term). Plain C++: the
// planner in pool.hip and tests/terms_first_check.cpp include it. See DESIGN.md §4.
//
// Per block and term q, p_q = (entries whose value set is in the term's bitmap) / entries, from the
// per-set entry counts kept when the block was loaded (KeyColumn::set_count). A block's p is the
// product of its p_q: the terms are taken as independent, which no count here can check (a
// conjunction of correlated tags passes more entries than the product says, one of exclusive tags
// fewer). The launch's p is the blocks' p weighted by the entries each contributes to the scan. A
// wave's 256-entry step then holds a term-passing entry with probability 1 - (1 - p)^256, and
// terms first is chosen when that share is below kTermsFirstMaxShare. A wrong estimate costs time,
// never a result: both modes compute the same verdicts.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace tsg {

// The largest share of steps holding a term-passing entry at which terms first is chosen: from the
// measured crossover (profiles/terms_first/README.md), set toward "off" because a wrong "on" costs
// more than a wrong "off".
constexpr double kTermsFirstMaxShare = 0.30;
constexpr uint32_t kTermsFirstStep = 256;  // entries of a wave's step (64 lanes x 4)

// The entries per value-set id of a key column (ids >= nsets, the absent key's all-ones among
// them, are not counted): out[s] for s < nsets.
inline void count_sets(const uint32_t *col, size_t n, uint32_t nsets, uint32_t *out) {
  for (uint32_t s = 0; s < nsets; s++) out[s] = 0;
  for (size_t i = 0; i < n; i++)
    if (col[i] < nsets) out[col[i]]++;
}

// One block of a launch: `scanned` of its `entries` entries are scanned; per term the counts of the
// key's value sets (nullptr: the block has none) and the term's 256-bit bitmap over them.
struct TermsFirstBlock {
  uint64_t entries, scanned;
  uint32_t nterms;
  const uint32_t *counts[4];
  uint32_t ncounts[4];
  const uint32_t *bitmap[4];
};

// The launch's p, or a negative value when some block has no counts (or nothing is scanned).
inline double terms_first_p(const TermsFirstBlock *blk, size_t nblk) {
  double num = 0, den = 0;
  for (size_t i = 0; i < nblk; i++) {
    const TermsFirstBlock &b = blk[i];
    if (!b.scanned) continue;
    if (!b.entries || !b.nterms) return -1.0;
    double p = 1.0;
    for (uint32_t t = 0; t < b.nterms && t < 4; t++) {
      if (!b.counts[t] || !b.bitmap[t]) return -1.0;
      uint64_t in = 0;
      for (uint32_t s = 0; s < b.ncounts[t] && s < 256; s++)
        if ((b.bitmap[t][s >> 5] >> (s & 31u)) & 1u) in += b.counts[t][s];
      p *= double(in) / double(b.entries);
    }
    num += p * double(b.scanned);
    den += double(b.scanned);
  }
  return den > 0 ? num / den : -1.0;
}
// The expected share of steps that hold a term-passing entry.
inline double terms_first_share(double p) {
  if (p <= 0) return 0.0;
  if (p >= 1) return 1.0;
  return -std::expm1(double(kTermsFirstStep) * std::log1p(-p));
}
// The choice: mode 0 off, 1 forced, 2 auto (from p; no counts: off).
inline bool terms_first_pick(int mode, double p) {
  if (mode == 0) return false;
  if (mode == 1) return true;
  return p >= 0 && terms_first_share(p) < kTermsFirstMaxShare;
}

}  // namespace tsg
