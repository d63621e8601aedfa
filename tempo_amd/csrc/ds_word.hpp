// ds_word.hpp — the narrow-scan kernels' packed scan word: one definition for the host packer
// (devctx.hip pack_scan) and the kernels' predicates (pool_kernels.hpp unit_mask). Plain C++: the
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

// ------------------------------------------------------------------------------------
// The predicates' short forms (pool_kernels.hpp unit_mask). The decode above stays the definition:
// tests/scan_pred_check.cpp checks every form below against it.

// a x b for a, b < 2^24 (the device's one-pass multiply)
TSG_DS_HD inline uint32_t ds_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}
// ds_div1000 by the 24-bit multiply (q <= 32767 < 2^24, 67109 < 2^24, the product < 2^32)
TSG_DS_HD inline uint32_t ds_div1000_24(uint32_t q) { return ds_mul24(q, 67109u) >> 26; }

// Duration: lo <= D16 <= hi as one unsigned compare, D16 - lo <= hi - lo (D16 below lo wraps past
// every span; an absent side is 0 / 2^32 - 1 and passes as it did). lo > hi matches nothing: lo
// becomes 2^32 - 1 and the span 0, D16 + 1 is never 0.
struct DsDur {
  uint32_t lo, span;
};
TSG_DS_HD inline DsDur ds_dur_form(uint32_t lo, uint32_t hi) {
  return lo > hi ? DsDur{0xffffffffu, 0u} : DsDur{lo, hi - lo};
}
TSG_DS_HD inline bool ds_dur_ok(uint32_t w, DsDur f) { return (w & 0xffffu) - f.lo <= f.span; }

// Time range on the word itself, for a block (base) and a query (start_s, end_s), while neither
// escape is set:
//   end_s >= start seconds   <=>  rel <= end_s - base            <=>  w < e_lim
//   start_s <= end seconds   <=>  rel + carry + floor(ms / 1000) >= start_s - base
//                            <=>  2000 (rel + carry) + D16 >= 2000 (start_s - base) = s_lim
// (ms = D16 >> 1; 2000 x + 2 ms >= 2000 y <=> x + floor(ms / 1000) >= y, and D16's low bit cannot
// carry an even sum past an even bound; rel + carry = (w + 2^16) >> 17, rel <= 0x7ffe.) Both
// sides are clamped to what a word can reach, so the thresholds always exist; what does not is a
// base so late that base + rel + 33 s wraps uint32: `fast` is 0 then and every entry of the
// block takes the decode above, as the escaped ones do.
struct DsRange {
  uint32_t fast, e_lim, s_lim;
};
TSG_DS_HD inline DsRange ds_range_form(uint32_t base, uint32_t start_s, uint32_t end_s) {
  DsRange f;
  f.fast = base < 0xffff0000u;
  const uint32_t er = end_s - base, sr = start_s - base;
  f.e_lim = end_s >= base ? ((er < 0x7ffeu ? er : 0x7ffeu) + 1u) << 17 : 0u;
  f.s_lim = start_s > base ? 2000u * (sr < 0x8100u ? sr : 0x8100u) : 0u;  // (2000 x 0x8100 > any word's sum)
  return f;
}
TSG_DS_HD inline bool ds_range_ok(uint32_t w, uint32_t e_lim, uint32_t s_lim) {
  const uint32_t rc = (w + 0x10000u) >> 17;
  return (w < e_lim) & (ds_mul24(rc, 2000u) + (w & 0xffffu) >= s_lim);
}
// some of four words escaped, as one maximum each
TSG_DS_HD inline uint32_t ds_max4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t x = a > b ? a : b, y = c > d ? c : d;
  return x > y ? x : y;
}
TSG_DS_HD inline bool ds_any_start_escaped(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return ds_max4(a, b, c, d) >= (kDsRelEsc << 17);
}
TSG_DS_HD inline bool ds_any_end_escaped(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return ds_max4(a & 0xffffu, b & 0xffffu, c & 0xffffu, d & 0xffffu) == kDsEndEsc;
}

// Term verdicts as bytes: a 256-bit value-set bitmap and its set count ns become a 256-byte table,
// byte x = (x < ns) & bit x. This is the table's dword for the bytes x0 .. x0 + 3 (x0 a multiple
// of 4) from the bitmap's four bits there (bit j -> bit 8j: the shifts 0, 7, 14, 21 do not meet).
TSG_DS_HD inline uint32_t ds_term_word(uint32_t bits4, uint32_t x0, uint32_t ns) {
  const uint32_t left = ns > x0 ? ns - x0 : 0u, keep = left >= 4u ? 0xfu : (1u << left) - 1u;
  return ((bits4 & keep) * 0x00204081u) & 0x01010101u;
}
TSG_DS_HD inline uint32_t ds_term_bits4(const uint32_t *bm8, uint32_t x0) { return (bm8[x0 >> 5] >> (x0 & 31u)) & 0xfu; }

// The entries of a unit that exist, nv of them (nv >= 512: all): bit 4k + j of lane l is entry
// 256 k + 4 l + j, as in the unit's match mask.
TSG_DS_HD inline uint32_t ds_valid_mask(uint32_t nv, uint32_t lane) {
  if (nv >= 512u) return 0xffu;
  uint32_t m = 0;
  for (uint32_t k = 0; k < 2; k++) {
    const uint32_t first = 256u * k + 4u * lane;
    const uint32_t c = nv > first ? (nv - first < 4u ? nv - first : 4u) : 0u;
    m |= ((1u << c) - 1u) << (4 * k);
  }
  return m;
}

}  // namespace tsg
