// scan_pred_check.cpp — the narrow kernels' short predicate forms (tempo_amd/csrc/ds_word.hpp:
// ds_dur_ok, ds_range_ok with ds_range_form and the escape / late-base fallback, ds_term_word,
// ds_valid_mask, ds_div1000_24) checked on the host against the header's own decode-and-compare,
// which stays the definition. Built and run by tests/test_scan_pred.py. Exit status 0 and a last
// line "ok <checks>" when everything holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ds_word.hpp"

using namespace tsg;

static uint64_t g_checked = 0, g_failed = 0;
static void expect(bool ok, const char *what, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  g_checked++;
  if (!ok && g_failed++ < 10)
    std::printf("FAIL %s %llu %llu %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c,
                (unsigned long long)d);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// The range verdict as the kernels had it: start from the word or, escaped, the exact column (xs);
// end from that start or, escaped, the exact column (xe); req.Start <= end && req.End >= start.
static bool range_ref(uint32_t w, uint32_t base, uint32_t xs, uint32_t xe, uint32_t qs, uint32_t qe) {
  const uint32_t sv = ds_start_escaped(w) ? xs : ds_start(w, base);
  const uint32_t ev = ds_end_escaped(w) ? xe : ds_end(w, sv);
  return qs <= ev && qe >= sv;
}
// ... and as unit_mask has it now: the word's two compares, or the decode where an escape is
// set or the block's base is too late for the thresholds
static bool range_new(uint32_t w, uint32_t base, uint32_t xs, uint32_t xe, uint32_t qs, uint32_t qe) {
  const DsRange f = ds_range_form(base, qs, qe);
  const bool slow = ds_any_start_escaped(w, 0, 0, 0) || ds_any_end_escaped(w, 0, 0, 0) || !f.fast;
  return slow ? range_ref(w, base, xs, xe, qs, qe) : ds_range_ok(w, f.e_lim, f.s_lim);
}

int main() {
  // ---- the 24-bit multiply
  for (uint32_t q = 0; q <= 32767; q++) expect(ds_div1000_24(q) == ds_div1000(q) && ds_div1000_24(q) == q / 1000, "div1000", q, 0, 0, 0);

  // ---- duration: every D16, every pair of bounds from the edge set (lo > hi included)
  const uint32_t edge[] = {0, 1, 2, 19, 20, 21, 1999, 2000, 2001, 65534, 65535, 0xffffffffu};
  for (uint32_t lo : edge)
    for (uint32_t hi : edge) {
      const DsDur f = ds_dur_form(lo, hi);
      for (uint32_t d = 0; d <= 65535; d++) {
        const uint32_t w = d | uint32_t(rnd() << 16);  // (the upper half is not the duration's)
        expect(ds_dur_ok(w, f) == (ds_d16(w) >= lo && ds_d16(w) <= hi), "dur", lo, hi, d, 0);
      }
    }

  // ---- range: every D16 x carry, rel and base at their edges, query bounds on and beside the
  // decoded seconds; escaped words against exact columns of their own
  const uint32_t rels[] = {0, 1, 16383, 0x7ffd, 0x7ffe, 0x7fff};
  const uint32_t bases[] = {0, 1, 16383, 1700000000u, 0xffffffffu - 0x7fffu, 0xffffffffu - 0x7ffeu, 0xffffffffu};
  for (uint32_t base : bases)
    for (uint32_t rel : rels)
      for (uint32_t carry = 0; carry < 2; carry++)
        for (uint32_t d = 0; d <= 65535; d++) {
          const uint32_t w = d | carry << 16 | rel << 17;
          // the exact columns an escaped word would be read with: a start outside the window,
          // an end before it (a wrapped duration) or long after
          const uint32_t xs = base + (d & 1 ? 0x7fffu + d : 0u - 1u - d), xe = (d & 2) ? xs + 40000u + d : (d & 4 ? 0u : xs - 1u);
          const uint32_t sv = ds_start_escaped(w) ? xs : ds_start(w, base), ev = ds_end_escaped(w) ? xe : ds_end(w, sv);
          const uint32_t qs[] = {0, sv - 1, sv, sv + 1, ev - 1, ev, ev + 1, 0xffffffffu};
          for (uint32_t a : qs)
            for (uint32_t b : qs)
              expect(range_new(w, base, xs, xe, a, b) == range_ref(w, base, xs, xe, a, b), "range", w, base, a, b);
        }
  // the four-word escape tests against the per-word ones
  for (int i = 0; i < 200000; i++) {
    uint32_t w[4];
    for (uint32_t &x : w) {
      x = uint32_t(rnd());
      if (rnd() % 5 == 0) x |= 0xffffu;
      if (rnd() % 5 == 0) x |= 0xfffe0000u;
    }
    expect(ds_any_start_escaped(w[0], w[1], w[2], w[3]) ==
               (ds_start_escaped(w[0]) || ds_start_escaped(w[1]) || ds_start_escaped(w[2]) || ds_start_escaped(w[3])),
           "any_start", w[0], w[1], w[2], w[3]);
    expect(ds_any_end_escaped(w[0], w[1], w[2], w[3]) ==
               (ds_end_escaped(w[0]) || ds_end_escaped(w[1]) || ds_end_escaped(w[2]) || ds_end_escaped(w[3])),
           "any_end", w[0], w[1], w[2], w[3]);
  }

  // ---- term tables: every x, the set counts' edges, fixed and seeded random bitmaps
  std::vector<std::vector<uint32_t>> bms;
  bms.push_back(std::vector<uint32_t>(8, 0u));
  bms.push_back(std::vector<uint32_t>(8, 0xffffffffu));
  for (uint32_t bit : {0u, 31u, 32u, 255u}) {
    std::vector<uint32_t> bm(8, 0u);
    bm[bit >> 5] = 1u << (bit & 31);
    bms.push_back(bm);
  }
  for (int i = 0; i < 64; i++) {
    std::vector<uint32_t> bm(8);
    for (uint32_t &x : bm) x = uint32_t(rnd()) & (i & 1 ? uint32_t(rnd()) : 0xffffffffu);
    bms.push_back(bm);
  }
  const uint32_t nss[] = {0, 1, 2, 31, 32, 33, 254, 255};
  for (const auto &bm : bms)
    for (uint32_t ns : nss) {
      uint8_t table[256];
      for (uint32_t x0 = 0; x0 < 256; x0 += 4) {
        const uint32_t wd = ds_term_word(ds_term_bits4(bm.data(), x0), x0, ns);
        for (uint32_t j = 0; j < 4; j++) table[x0 + j] = uint8_t(wd >> (8 * j));
      }
      for (uint32_t x = 0; x < 256; x++) {
        const uint32_t ref = uint32_t(x < ns) & (bm[x >> 5] >> (x & 31)) & 1u;  // (the bitmap test it replaces)
        expect(table[x] == ref, "term", x, ns, bm[x >> 5], table[x]);
      }
    }

  // ---- the entries of a unit that exist
  for (uint32_t nv = 0; nv <= 520; nv++)
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t m = ds_valid_mask(nv, lane);
      for (uint32_t k = 0; k < 2; k++)
        for (uint32_t j = 0; j < 4; j++)
          expect(((m >> (4 * k + j)) & 1u) == uint32_t(256 * k + 4 * lane + j < nv) && m < 256, "valid", nv, lane, k, j);
    }

  if (g_failed) {
    std::printf("%llu of %llu checks failed\n", (unsigned long long)g_failed, (unsigned long long)g_checked);
    return 1;
  }
  std::printf("ok %llu\n", (unsigned long long)g_checked);
  return 0;
}
