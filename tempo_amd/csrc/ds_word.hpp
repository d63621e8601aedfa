// ds_word.hpp — the narrow-scan kernels' packed scan word: one definition for the host packer
// (devctx.hip pack_scan) and the kernels' decode (pool_kernels.hpp unit_ends). Plain C++: the
// host compiler includes it too (tests/ds_pack_check.cpp). See DESIGN.md §3.
//
//   bits  0..15  D16    2 * floor(dur / 1 ms) + (dur % 1 ms != 0), 0xffff when floor(dur / 1 ms) >= 0x8000
//   bit   16     carry  (end_s - start_s) - floor(dur / 1 s): 0 or 1; 0 when D16 == 0xffff
//   bits 17..31  rel    start_s - base when that is in [0, 0x7ffe], else 0x7fff
//
// base is the block's (DevBlock::sbase). An unsaturated D16 means 0 <= end - start < 32.768 s, so
// floor(end / 1 s) - floor(start / 1 s) is floor(dur / 1 s) or one more, and floor(dur / 1 s) =
// (D16 >> 1) / 1000: start and end seconds come back exactly (uint32, wrapping as the exact
// columns do). What does not fit escapes: D16 == 0xffff (durations >= 32.768 s, ends before the
// start, whose uint64 duration wraps) -> the exact end_s column; rel == 0x7fff -> the exact
// start_s column.
#pragma once
#include <cstdint>

#ifndef TSG_DS_HD
#if defined(__HIP__) || defined(__CUDACC__)
#define TSG_DS_HD __host__ __device__
#else
#define TSG_DS_HD
#endif
#endif

namespace tsg {

constexpr uint32_t kDsEndEsc = 0xffffu;    // D16: the end is read from end_s
constexpr uint32_t kDsRelEsc = 0x7fffu;    // rel: the start is read from start_s
constexpr uint32_t kDsBaseBack = 16383u;   // base = max(0, median start_s - this): the window centred on the median

// q / 1000 for q in [0, 32767] (exhaustively checked by tests/test_ds_pack.py): 67109 / 2^26 is
// 1/1000 + 2.1e-9, and 32767 x 2.1e-9 < 1/1000; 32767 x 67109 < 2^32
TSG_DS_HD inline uint32_t ds_div1000(uint32_t q) { return (q * 67109u) >> 26; }

TSG_DS_HD inline uint32_t ds_base(uint32_t median_start_s) {
  return median_start_s > kDsBaseBack ? median_start_s - kDsBaseBack : 0u;
}

TSG_DS_HD inline uint32_t ds_pack(uint64_t start_ns, uint64_t end_ns, uint32_t base) {
  const uint64_t dd = end_ns - start_ns;  // uint64 wrap (pitfall P2)
  const uint64_t q = dd / 1000000ULL;
  const uint32_t d16 = q >= 0x8000ULL ? kDsEndEsc : uint32_t(2 * q + (dd % 1000000ULL != 0));
  const uint32_t ss = uint32_t(start_ns / 1000000000ULL), es = uint32_t(end_ns / 1000000000ULL);
  const uint32_t carry = d16 == kDsEndEsc ? 0u : ((es - ss) - ds_div1000(uint32_t(q))) & 1u;
  const uint32_t off = ss - base;  // (uint32: a start before the base wraps to a large value)
  const uint32_t rel = off < kDsRelEsc ? off : kDsRelEsc;
  return d16 | carry << 16 | rel << 17;
}

TSG_DS_HD inline uint32_t ds_d16(uint32_t w) { return w & 0xffffu; }
TSG_DS_HD inline bool ds_end_escaped(uint32_t w) { return (w & 0xffffu) == kDsEndEsc; }
TSG_DS_HD inline bool ds_start_escaped(uint32_t w) { return (w >> 17) == kDsRelEsc; }
// start seconds (exact unless ds_start_escaped)
TSG_DS_HD inline uint32_t ds_start(uint32_t w, uint32_t base) { return base + (w >> 17); }
// end seconds from the entry's exact start seconds (exact unless ds_end_escaped)
TSG_DS_HD inline uint32_t ds_end(uint32_t w, uint32_t sv) {
  return sv + ds_div1000((w & 0xffffu) >> 1) + ((w >> 16) & 1u);
}

}  // namespace tsg
