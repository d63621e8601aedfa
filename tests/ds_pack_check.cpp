// ds_pack_check.cpp — the packed scan word (tempo_amd/csrc/ds_word.hpp) checked on the host: the
// multiply-shift division exhaustively, and pack -> decode against the exact start / end seconds
// and the two escape rules over edge entries and seeded random ones. Built and run by
// tests/test_ds_pack.py. Exit status 0 and a last line "ok <entries>" when everything holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ds_word.hpp"

using namespace tsg;

static const uint64_t S = 1000000000ULL, MS = 1000000ULL;
static uint64_t g_checked = 0, g_failed = 0, g_end_esc = 0, g_start_esc = 0;

static void check(uint64_t start, uint64_t end, uint32_t base) {
  const uint32_t w = ds_pack(start, end, base);
  const uint32_t ss = uint32_t(start / S), es = uint32_t(end / S);
  const uint64_t dd = end - start, q = dd / MS;
  const uint32_t d16 = q >= 0x8000 ? 0xffffu : uint32_t(2 * q + (dd % MS != 0));
  const bool want_end_esc = d16 == 0xffffu, want_start_esc = uint32_t(ss - base) > 0x7ffeu;
  bool ok = ds_d16(w) == d16 && ds_end_escaped(w) == want_end_esc && ds_start_escaped(w) == want_start_esc;
  if (want_end_esc) ok = ok && ((w >> 16) & 1u) == 0;
  if (!want_start_esc) ok = ok && ds_start(w, base) == ss;
  // the kernel decodes the end from the entry's start seconds: the decoded ones, or the exact
  // column's after a start escape
  if (!want_end_esc) ok = ok && ds_end(w, ss) == es;
  if (!want_end_esc && !want_start_esc) ok = ok && ds_end(w, ds_start(w, base)) == es;
  g_checked++;
  g_end_esc += want_end_esc;
  g_start_esc += want_start_esc;
  if (!ok && g_failed++ < 10)
    std::printf("FAIL start=%llu end=%llu base=%u word=%08x\n", (unsigned long long)start, (unsigned long long)end, base, w);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ULL);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

int main() {
  for (uint32_t q = 0; q <= 32767; q++)
    if (ds_div1000(q) != q / 1000) {
      std::printf("FAIL ds_div1000(%u) = %u\n", q, ds_div1000(q));
      return 1;
    }
  if (ds_base(0) != 0 || ds_base(16383) != 0 || ds_base(16384) != 1 || ds_base(1700000000u) != 1700000000u - 16383u) {
    std::printf("FAIL ds_base\n");
    return 1;
  }
  // durations: around whole seconds, and whole ms +- 1 ns around the seconds and the code's end
  std::vector<uint64_t> durs = {0, 1, S - 1, S, S + 1};
  for (uint64_t m : {999, 1000, 1001, 31999, 32000, 32766, 32767, 32768}) {
    durs.push_back(m * MS - 1);
    durs.push_back(m * MS);
    durs.push_back(m * MS + 1);
  }
  const uint64_t subs[] = {0, 1, S - 1};
  // bases: 0, a usual one, one whose window ends at the last uint32 second
  const uint32_t bases[] = {0u, 1700000000u - 16383u, 0xffffffffu - 0x7ffeu, 0xffffffffu - 5u};
  for (uint32_t base : bases) {
    // starts at base - 1, base, the window's last second, one past it, far past it, second 1,
    // and near 2^32 - 1
    std::vector<uint32_t> secs = {base - 1u, base, base + 0x7ffeu, base + 0x7fffu, base + 100000u, 1u, 0xffffffffu, 0xfffffffeu};
    for (uint32_t sec : secs)
      for (uint64_t sub : subs) {
        const uint64_t start = uint64_t(sec) * S + sub;
        for (uint64_t d : durs) check(start, start + d, base);
        check(start, 0, base);          // end = 0
        check(start, start - 1, base);  // an end before the start
      }
  }
  // seeded random entries: starts within +- 12 h of the window's middle, durations lognormal-like
  // (a random magnitude from ns to ~100 s), a few ends of 0 and before the start
  for (int i = 0; i < 400000; i++) {
    const uint32_t base = (rnd() & 7) ? 1700000000u - 16383u : uint32_t(rnd() % 3000000000ULL);
    const uint64_t sec = uint64_t(base) + 16383 + rnd() % 86400 - 43200;
    const uint64_t start = (sec & 0xffffffffULL) * S + rnd() % S;
    const uint64_t d = rnd() % (1ULL << (1 + rnd() % 37));
    const uint64_t k = rnd() % 100;
    check(start, k == 0 ? 0 : k == 1 ? start - 1 - rnd() % (20 * S) : start + d, base);
  }
  if (g_failed) {
    std::printf("%llu of %llu entries failed\n", (unsigned long long)g_failed, (unsigned long long)g_checked);
    return 1;
  }
  std::printf("end escapes %llu, start escapes %llu\n", (unsigned long long)g_end_esc, (unsigned long long)g_start_esc);
  std::printf("ok %llu\n", (unsigned long long)g_checked);
  return 0;
}
