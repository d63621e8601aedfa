// pool_kernels.hpp — the device side of pool.hip (its only includer): the argument structs of the
// three narrow-scan kernels, the unit helpers they share, and the kernels. See DESIGN.md §4.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ds_word.hpp"
#include "search_common.hpp"

namespace tsg {

// ------------------------------------------------------------------------------------
// pool search: narrow full scans (limit 0) with a CU-wide work pool
//
// One 1024-thread workgroup per CU (16 waves; its LDS request keeps a second one off the
// CU). The query's blocks form one space of 512-entry units (a wave tile: 8 entries per
// lane). A workgroup owns a static run of units, handed out one unit per claim from an
// LDS counter to whichever of its waves is free, so the waves of a CU finish together
// whatever order the CU's issue arbitration serves them in (the static split's four
// workgroups per CU finished as a ladder 22/25/28/33 us, profiles/r02_prio). The last
// units of the launch are claimed in chunks from one device counter (dequeue: one
// returning atomic per chunk, issued `lookahead` claims before the chunk is needed), so
// CUs that the fabric serves faster take more of them. Matches go to the workgroup's LDS
// record buffer as they are found (gathered from the cold columns right away; record
// order inside a workgroup is claim order — the host sorts each block's records by scan
// position, which is the reference order), then to the workgroup's segment of pinned
// host memory with write-through stores, then its count. Records beyond the LDS capacity
// are counted, not kept: the host then reruns the query on the segment/look-back path.
constexpr int kPoolWaves = 16;
constexpr int kPoolThreads = kPoolWaves * 64;
constexpr uint32_t kPoolTile = 512;       // entries per unit (wave tile)
constexpr uint32_t kPoolChunks = 1024;    // dynamic chunks one workgroup can take
constexpr uint32_t kPoolPending = 0xffffffffu, kPoolNone = 0xfffffffeu;
constexpr uint32_t kPoolSpinMax = 1u << 24;  // LDS poll bound (~1 s of s_sleep 2)
// LDS: the record buffer is sized so that one workgroup takes more than half a CU
constexpr size_t kPoolLds = 96 << 10;
static_assert(kColPad % kPoolTile == 0, "column padding covers whole units");

struct PoolBlk {           // 64 B, staged in LDS
  const uint32_t *scan;    // dur32 | start_s | end_s | ds, npad entries each (the pool reads ds; escapes the exact ones)
  const uint8_t *col[4];   // one-byte term columns
  uint32_t npad, nent;
  uint32_t ubase;          // first unit of the block in the launch's unit space
  uint32_t bmi4, nsets4;   // per term: bitmap index into `bms`, value-set count (bytes)
  uint32_t block_idx;
};
static_assert(sizeof(PoolBlk) == 64, "pool block layout");
struct PoolArgs {
  PoolBlk blk[kArgSegs];
  const DevBlockDesc *desc[kArgSegs];  // cold columns (ids, times, names) of matches
  uint32_t bms[kArgBms][8];
  uint32_t ubase[kArgSegs + 1];  // first unit of each block, units at nsegs (static kernel's block walk)
  uint32_t ebase[kArgSegs];      // scan position of each block's first unit (a limit wave's part of a block)
  uint32_t sbase[kArgSegs];      // each block's base second of its packed scan words (ds_word.hpp)
  uint32_t nsegs, units, static_per_wg, dyn0;  // static run of workgroup w: [w*S, w*S+S); dynamic [dyn0, units)
  uint32_t chunk_shift, lookahead, rec_cap, seg_cap, has_min, has_max, min32, max32, start_s, end_s;
  unsigned *head;       // this launch's dynamic-chunk counter (zero at launch)
  unsigned *head_next;  // the next launch's counter: zeroed by this one
  uint8_t *recs;        // pinned host: workgroup w's first seg_cap records at w * seg_cap (rec_cap: LDS records)
  uint32_t *counts;     // pinned host: workgroup w's match count, stored after its records
  unsigned long long *stamps;
  uint32_t *err;        // pinned host: set when an LDS poll ran past its bound (the host fails the query)
  // limit L > 0: a unit keeps its first L matches in scan order (a block's first L records lie
  // in the first L of each of its units; the host cuts each block to L): a dense limit query
  // hands over at most L records per unit instead of every match
  uint32_t unit_cap;
  // the launch shape, passed explicitly: the kernels read no implicit kernel argument (blockDim /
  // gridDim come from them), so an AQL packet of our own needs none (aql.cpp)
  uint32_t nthreads, ngroups;
  // static kernel: the launch's NW waves split the units as wave g -> [g*sq + min(g, sr), ...),
  // the first sr waves one unit more (sq, sr = units / NW, units % NW: no division on the device)
  uint32_t sq, sr;
  uint32_t nbms;                     // bitmaps in `bms` (the resident kernel's slot checksum)
  uint32_t cstride;                  // resident kernel: workgroup w's count at counts[w * cstride] (0 = 1)
  uint32_t wq, wr;                   // resident kernel: workgroup w scans units [w*wq + min(w, wr), +wq + (w < wr))
  // resident kernel, XCD-weighted split (xsplit != 0; W a multiple of 8): workgroup w = 8i + x (XCD x)
  // scans xn[x] + (i < xr[x]) units, the runs in workgroup order (pool.hip res_split)
  uint32_t xsplit;
  unsigned long long *qstamps;       // resident kernel, timed queries: per workgroup {seen, end} (100 MHz)
  uint32_t xn[8], xr[8];
  // the set count of each bitmap slot's (dictionary, term) pair: what the slot's byte table folds in
  // (the planner gives a slot to one pair, so its blocks agree on it)
  uint8_t bm_ns[kArgBms];
};
static_assert(sizeof(PoolArgs) <= 4096, "kernel arguments");

// The argument words a query with nsegs blocks and nbms bitmaps uses, as kArgRanges byte ranges
// of PoolArgs: the block table, descriptors, bitmaps, unit, entry and start bases, and the scalars from
// `nsegs` on. The host writes only those (a mailbox slot, an AQL packet of our own) and the
// resident kernel's slot checksum covers exactly them: all three read this one description.
struct ArgRange {
  uint32_t off, len;
};
constexpr int kArgRanges = 7;
__host__ __device__ inline ArgRange arg_range(int i, uint32_t nsegs, uint32_t nbms) {
  switch (i) {
    case 0: return {uint32_t(offsetof(PoolArgs, blk)), nsegs * uint32_t(sizeof(PoolBlk))};
    case 1: return {uint32_t(offsetof(PoolArgs, desc)), nsegs * 8u};
    case 2: return {uint32_t(offsetof(PoolArgs, bms)), nbms * 32u};
    case 3: return {uint32_t(offsetof(PoolArgs, ubase)), (nsegs + 1) * 4u};
    case 4: return {uint32_t(offsetof(PoolArgs, ebase)), nsegs * 4u};
    case 5: return {uint32_t(offsetof(PoolArgs, sbase)), nsegs * 4u};
    default: return {uint32_t(offsetof(PoolArgs, nsegs)), uint32_t(sizeof(PoolArgs) - offsetof(PoolArgs, nsegs))};
  }
}
__host__ __device__ inline bool res_word_used(uint32_t off, uint32_t nsegs, uint32_t nbms) {
  bool used = false;
#pragma unroll
  for (int i = 0; i < kArgRanges; i++) {
    const ArgRange r = arg_range(i, nsegs, nbms);
    used |= off >= r.off && off < r.off + r.len;
  }
  return used;
}

// ------------------------------------------------------------------------------------
// unit helpers, shared by the three kernels

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(v)); }

// A pointer read from LDS by every lane (same value), moved to SGPRs. (readfirstlane
// returns int: each half goes through uint32_t, or the low half sign-extends.)
template <typename T>
__device__ __forceinline__ T *uniform_ptr(T *p) {
  const uint64_t v = uint64_t(uintptr_t(p));
  const uint32_t lo = rfl(uint32_t(v)), hi = rfl(uint32_t(v >> 32));
  return reinterpret_cast<T *>((uint64_t(hi) << 32) | lo);
}

// The block of unit u: lanes test the block boundaries (ubase[b] = block b's first unit), the
// ballot counts those passed.
__device__ __forceinline__ uint32_t block_of(const uint32_t *ubase, uint32_t nsegs, uint32_t u, int lane) {
  return uint32_t(__popcll(__ballot(uint32_t(lane) + 1 < nsegs && u >= ubase[lane + 1])));
}

// A unit's filter columns in registers (wave-uniform e0: the unit's first entry in its block).
template <int NT>
struct UnitRegs {
  u32x4 d[kSteps];  // ds: the packed scan word (duration | carry | relative start)
  uint32_t tv[NT > 0 ? NT : 1][kSteps];
  uint32_t e0;
};

// Stream loads: default cache policy, or non-temporal (NTL: `nt`, the once-read filter
// columns do not displace the L2 / MALL lines other work reuses).
template <bool NTL>
__device__ __forceinline__ u32x4 stream4(const uint32_t *p, uint64_t e) {
  if constexpr (NTL) return __builtin_nontemporal_load(G<u32x4>(p + e));
  else return *G<u32x4>(p + e);
}
template <bool NTL>
__device__ __forceinline__ uint32_t stream1(const uint8_t *p, uint64_t e) {
  if constexpr (NTL) return __builtin_nontemporal_load(G<uint32_t>(p + e));
  else return *G<uint32_t>(p + e);
}

// Terms first (TF, a compile-time mode of load_unit and unit_mask and through them of the three
// kernels; instantiated where it means something: kTermsFirstShape): the packed scan word is 4 of a
// unit's 7 bytes per entry, and the result needs it only for an entry that has passed every term.
// A unit's loads are then the term columns alone, and a lane reads its 16 bytes of `ds` for a step
// only when one of its four entries of that step passed the terms (unit_mask). Which mode a query
// runs in is the host's choice per launch, from counted selectivities (terms_first.hpp): with a
// conjunction that passes 1 entry in 8000 a 64-byte line of `ds` holds a passing entry 0.2 % of
// the time; with one that passes 1 in 50 nearly every step would take the gated load, which waits
// for everything the wave has in flight.
template <int NT, bool DUR, bool RANGE>
constexpr bool kTermsFirstShape = NT > 0 && (DUR || RANGE);

// The loads of the unit at entry e0 of a block (scan columns of npad entries each; cols(q): the
// block's q-th term column, read when its loads are issued). Wave-uniform arguments.
template <int NT, bool DUR, bool RANGE, bool NTL, bool TF, class Cols>
__device__ __forceinline__ void load_unit(UnitRegs<NT> &R, const uint32_t *scan, uint32_t npad, Cols &&cols,
                                          uint32_t e0, int lane) {
  static_assert(!TF || kTermsFirstShape<NT, DUR, RANGE>, "terms first: a term and a filter on the scan word");
  R.e0 = e0;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint64_t e = uint64_t(e0) + uint64_t(k) * 256 + uint64_t(lane) * 4;
    if ((DUR || RANGE) && !TF) R.d[k] = stream4<NTL>(scan + 3ull * npad, e);
  }
#pragma unroll
  for (int q = 0; q < (NT > 0 ? NT : 1); q++) {
    if (NT <= 0) break;
    const uint8_t *col = cols(q);
#pragma unroll
    for (int k = 0; k < kSteps; k++)
      R.tv[q][k] = stream1<NTL>(col, uint64_t(e0) + uint64_t(k) * 256 + uint64_t(lane) * 4);
  }
}

// The ranks of a unit's matches (mask bit 4k + j of lane l = entry e0 + 256k + 4l + j) in scan
// order (k, then lane, then j), from per-step ballots (every lane takes part): rank0[k] = the rank
// of this lane's first match of step k, total = the unit's matches.
__device__ __forceinline__ void unit_ranks(uint32_t mask, int lane, uint32_t (&rank0)[kSteps], uint32_t &total) {
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  total = 0;
#pragma unroll
  for (int k = 0; k < kSteps; k++) {
    const uint32_t nib = (mask >> (4 * k)) & 0xfu;
    uint32_t lower = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t b = __ballot((nib >> j) & 1u);
      lower += uint32_t(__popcll(b & below));
      tot += uint32_t(__popcll(b));
    }
    rank0[k] = total + lower;
    total += tot;
  }
}
// the rank of this lane's match `bit` of `mask`
__device__ __forceinline__ uint32_t match_rank(const uint32_t (&rank0)[kSteps], uint32_t mask, uint32_t bit) {
  const uint32_t k = bit >> 2, j = bit & 3u;
  return (k ? rank0[1] : rank0[0]) + uint32_t(__popc((mask >> (4 * k)) & ((1u << j) - 1u)));
}
static_assert(kSteps == 2, "match_rank selects between two steps");

// The unit's matches cut to the first `cap` in scan order.
__device__ __forceinline__ uint32_t cap_unit_mask(uint32_t mask, uint32_t cap, int lane) {
  uint32_t rank0[kSteps], total, out = 0;
  unit_ranks(mask, lane, rank0, total);
#pragma unroll
  for (uint32_t bit = 0; bit < 4 * kSteps; bit++)
    if (((mask >> bit) & 1u) && match_rank(rank0, mask, bit) < cap) out |= 1u << bit;
  return out;
}

// The predicates of one unit (8 entries per lane) as a 32-bit lane mask, branch-free: every
// test is evaluated for every entry and combined with bitwise ands (short-circuit tests
// compiled to ~130 exec-mask branches per unit; with real, mixed values the lanes diverge
// and the 150 MB scan ran 8 us longer than with uniform data, profiles/r03_launch). The tests
// are ds_word.hpp's short forms, their wave-uniform parts in UnitPred (per query and block):
// a term is one byte read of its LDS table, the duration one compare, the range two compares on
// the packed word (each entry's verdict still costs a select and an or on its way into the mask).
// The entries that do not exist (a block's last unit) are cut once per unit.
//
// Range, escapes: for a lane's four entries of a step where some start lies outside the 15-bit
// window (rel 0x7fff) or some duration code is saturated (0xffff: durations from 32.768 s, ends
// before the start, e.g. the end = 0 entries of pitfall P1), and for every entry of a block
// whose base is too late for the word's thresholds (DsRange::fast), the word's tests are passed over and
// the four range verdicts come from ds_word.hpp's decode: starts from the exact start column
// where a start escaped, ends from the exact end column where an end did (rare; only the lanes
// that need them load: a unit-wide reload moved 16 MB more per config-2 query, the PMC count in
// profiles/r04_final). That decode sits under a per-lane branch, as the reloads always did: only
// the lanes that need it run it, the others wait for them (not a wave-uniform branch). A lane
// needs it when one of its four entries has passed everything else: with 0.1 % of the entries
// escaped about a fifth of a wave's steps hold an escaped word, but few of those an entry the
// terms and the duration let through, and the reloads drain the wave's loads in flight.
template <int NT>
struct UnitPred {
  DsDur dur;
  DsRange rng;
  uint32_t start_s, end_s, sbase, n;
  uint32_t tb[NT > 0 ? NT : 1];  // each term's table in s_tb (bytes)
};
template <int NT>
__device__ __forceinline__ UnitPred<NT> unit_pred(uint32_t dlo, uint32_t dhi, uint32_t start_s, uint32_t end_s,
                                                  uint32_t sbase, uint32_t n, uint32_t bmi4) {
  UnitPred<NT> P;
  P.dur = ds_dur_form(dlo, dhi);
  P.rng = ds_range_form(sbase, start_s, end_s);
  P.start_s = start_s;
  P.end_s = end_s;
  P.sbase = sbase;
  P.n = n;
#pragma unroll
  for (int q = 0; q < (NT > 0 ? NT : 1); q++) P.tb[q] = ((bmi4 >> (8 * q)) & 0xffu) * 256u;
  return P;
}
// The range verdicts of a lane's four words of a step from ds_word.hpp's decode (the escape path
// above): bit j = entry j lies in the query's range.
template <bool NTL>
__device__ __forceinline__ uint32_t range_decode_nib(const uint32_t (&w)[4], bool esc_s, bool esc_e, uint32_t start_s,
                                                     uint32_t end_s, uint32_t sbase, const uint32_t *scan, uint32_t npad,
                                                     uint64_t e) {
  // req.Start <= endSeconds && req.End >= startSeconds (pipeline.go:62-63)
  u32x4 sv = {ds_start(w[0], sbase), ds_start(w[1], sbase), ds_start(w[2], sbase), ds_start(w[3], sbase)};
  if (esc_s) sv = stream4<NTL>(scan + npad, e);
  u32x4 ev = {ds_end(w[0], sv.x), ds_end(w[1], sv.y), ds_end(w[2], sv.z), ds_end(w[3], sv.w)};
  if (esc_e) ev = stream4<NTL>(scan + 2ull * npad, e);
  return uint32_t((start_s <= ev.x) & (end_s >= sv.x)) | uint32_t((start_s <= ev.y) & (end_s >= sv.y)) << 1 |
         uint32_t((start_s <= ev.z) & (end_s >= sv.z)) << 2 | uint32_t((start_s <= ev.w) & (end_s >= sv.w)) << 3;
}
// Terms first: a step's nib is formed from the byte-table term tests alone; a lane whose nib is not
// zero (the same kind of per-lane branch as the escape reloads': the other lanes wait for it) loads
// its 16 bytes of `ds` for the step, applies the duration and range tests to them, and runs the
// escape path behind them as it is. The verdicts are the same bits in the same order: an entry's
// bit is the and of its tests either way, and a zero nib stays zero. The gated load is waited for
// at once, which drains what the wave has in flight, as an escape reload does: the host chooses this
// mode only where few steps hold a term-passing entry.
template <int NT, bool DUR, bool RANGE, bool NTL, bool TF>
__device__ __forceinline__ uint32_t unit_mask(const UnitRegs<NT> &R, const UnitPred<NT> &P, const uint8_t *s_tb,
                                              const uint32_t *scan, uint32_t npad, int lane) {
  uint32_t mask = 0;
#pragma unroll
  for (int k = kSteps - 1; k >= 0; k--) {
    const uint64_t e = uint64_t(R.e0) + uint64_t(k) * 256 + uint64_t(lane) * 4;
    uint32_t w[4] = {0, 0, 0, 0};
    if ((DUR || RANGE) && !TF) {
      w[0] = R.d[k].x;
      w[1] = R.d[k].y;
      w[2] = R.d[k].z;
      w[3] = R.d[k].w;
    }
    bool esc_s = false, esc_e = false, slow = false;
    if (RANGE && !TF) {
      esc_s = ds_any_start_escaped(w[0], w[1], w[2], w[3]);
      esc_e = ds_any_end_escaped(w[0], w[1], w[2], w[3]);
      slow = esc_s | esc_e | !P.rng.fast;
    }
    uint32_t nib = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
      bool ok = true;
      if (DUR && !TF) ok = ds_dur_ok(w[j], P.dur);
      if (RANGE && !TF) ok = ok & (slow | ds_range_ok(w[j], P.rng.e_lim, P.rng.s_lim));
      if (NT > 0) {
        uint32_t hits = 0;
#pragma unroll
        for (int q = 0; q < (NT > 0 ? NT : 1); q++) hits += s_tb[P.tb[q] + ((R.tv[q][k] >> (8 * j)) & 0xffu)];
        ok = ok & (hits == uint32_t(NT));
      }
      nib = nib + nib + uint32_t(ok);
    }
    if constexpr (TF) {
      if (nib != 0) {
        const u32x4 d = stream4<NTL>(scan + 3ull * npad, e);
        w[0] = d.x;
        w[1] = d.y;
        w[2] = d.z;
        w[3] = d.w;
        if (RANGE) {
          esc_s = ds_any_start_escaped(w[0], w[1], w[2], w[3]);
          esc_e = ds_any_end_escaped(w[0], w[1], w[2], w[3]);
          slow = esc_s | esc_e | !P.rng.fast;
        }
        uint32_t fn = 0;
#pragma unroll
        for (int j = 3; j >= 0; j--) {
          bool ok = true;
          if (DUR) ok = ds_dur_ok(w[j], P.dur);
          if (RANGE) ok = ok & (slow | ds_range_ok(w[j], P.rng.e_lim, P.rng.s_lim));
          fn = fn + fn + uint32_t(ok);
        }
        nib &= fn;
        if (RANGE && slow && nib != 0)
          nib &= range_decode_nib<NTL>(w, esc_s, esc_e, P.start_s, P.end_s, P.sbase, scan, npad, e);
      }
    } else if (RANGE && slow && nib != 0) {
      // (only a lane that can still match: the terms, the duration and, where the word's tests hold,
      // the range are in nib already, and nib &= in leaves a zero nib as it is)
      nib &= range_decode_nib<NTL>(w, esc_s, esc_e, P.start_s, P.end_s, P.sbase, scan, npad, e);
    }
    mask = (mask << 4) | nib;
  }
  const uint32_t nv = P.n - R.e0;  // (wave-uniform: only a block's last unit is cut)
  if (nv < kPoolTile) mask &= ds_valid_mask(nv, uint32_t(lane));
  return mask;
}

// The launch's term tables: slot j of the bitmaps becomes s_tb[256 j ..], byte x = (x < ns) & bit x
// (ds_word.hpp). One table dword per thread, so the build is a dozen instructions deep on every
// wave, not a hundred on two (every wave waits for it at the staging barrier): dword i holds the
// bytes 4 (i % 64) .. of slot i / 64, from bitmap word i / 8 (bmw) and the slot's set count
// (PoolArgs::bm_ns); only the launch's nbms slots are built.
constexpr uint32_t kTermDwords = uint32_t(kArgBms) * 64;
__device__ __forceinline__ void stage_term_dword(uint8_t *s_tb, uint32_t i, uint32_t bmw, uint32_t ns) {
  const uint32_t x0 = (i & 63u) * 4;
  reinterpret_cast<uint32_t *>(s_tb)[i] = ds_term_word((bmw >> (x0 & 31u)) & 0xfu, x0, ns);
}
// (pool and static kernels: this thread's dword from the words it loaded ahead of the units'
// loads; a workgroup of fewer than 1024 threads, TSG_POOL_WAVES, builds the rest from the kernel
// arguments directly)
template <int NT>
__device__ __forceinline__ void stage_term_tables(uint8_t *s_tb, const PoolArgs &A, uint32_t xbm, uint32_t xns,
                                                  uint32_t tid) {
  if (NT <= 0) return;
  const uint32_t n = min(A.nbms, uint32_t(kArgBms)) * 64;
  if (tid < n) stage_term_dword(s_tb, tid, xbm, xns);
  for (uint32_t i = tid + A.nthreads; i < n; i += A.nthreads)
    stage_term_dword(s_tb, i, reinterpret_cast<const uint32_t *>(A.bms)[i >> 3], A.bm_ns[i >> 6]);
}
static_assert(kTermDwords <= kPoolThreads, "one table dword per thread of a full workgroup");

// A workgroup barrier that waits for this wave's LDS and scalar-memory operations only
// (lgkmcnt), not for its vector loads in flight: __syncthreads()' fence also waits
// vmcnt(0), which at the staging barrier drained the units each wave had already asked for
// (the whole launch-wide burst: ~8-10 us before any wave evaluated its first unit). The
// staging below reads the kernel arguments with scalar loads, so nothing it needs is
// counted by vmcnt. (asm memory clobber: no LDS access moves across it)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// One match record (MatchRec: six words) into slot r of the LDS record buffer.
__device__ __forceinline__ void put_rec(unsigned long long *s_rec, uint32_t r, const u32x4 &id, uint64_t st, uint64_t en,
                                        uint32_t ei, uint32_t bidx, uint32_t il, uint64_t nm) {
  unsigned long long *d = s_rec + uint64_t(r) * 6;
  d[0] = (unsigned long long)id.x | (unsigned long long)id.y << 32;
  d[1] = (unsigned long long)id.z | (unsigned long long)id.w << 32;
  d[2] = st;
  d[3] = en;
  d[4] = (unsigned long long)ei | (unsigned long long)(bidx | (il << 24)) << 32;
  d[5] = nm;
}

// The cold columns of a block (what a match's record is gathered from).
struct ColdCols {
  const uint8_t *ids, *id_len;
  const uint64_t *st_ns, *en_ns, *names;
};
__device__ __forceinline__ ColdCols cold_cols(const DevBlockDesc *D) {
  const auto *Dc = K4(D);
  return {Dc->ids, Dc->id_len, Dc->start_ns, Dc->end_ns, reinterpret_cast<const uint64_t *>(Dc->names)};
}
// Entry ei's record, gathered and stored at once.
__device__ __forceinline__ void gather_put(unsigned long long *s_rec, uint32_t r, const ColdCols &C, uint32_t ei,
                                           uint32_t bidx) {
  const u32x4 id = *G<u32x4>(C.ids + uint64_t(ei) * 16);
  const uint64_t st = G(C.st_ns)[ei], en = G(C.en_ns)[ei];
  const uint64_t nm = G(C.names)[ei];
  const uint32_t il = G(C.id_len)[ei];
  put_rec(s_rec, r, id, st, en, ei, bidx, il, nm);
}
// A unit's matches (pool and static kernels): slots in the workgroup's LDS record buffer in
// claim order, record fields gathered now; records past rec_cap are counted, not kept.
__device__ __forceinline__ void put_unit(unsigned long long *s_rec, uint32_t *s_nrec, uint32_t rec_cap, uint32_t mask,
                                         const DevBlockDesc *D, uint32_t bidx, uint32_t e0, int lane) {
  const ColdCols C = cold_cols(D);
  const uint32_t cnt = __popc(mask);
  uint32_t slot = 0;
  if (cnt) slot = atomicAdd(s_nrec, cnt);
  for (int b = 0; b < 4 * kSteps; b++) {
    if (!(mask & (1u << b))) continue;
    const uint32_t r = slot++;
    if (r >= rec_cap) continue;
    gather_put(s_rec, r, C, e0 + uint32_t(b >> 2) * 256 + uint32_t(lane) * 4 + uint32_t(b & 3), bidx);
  }
}

// The pool and static kernels' stamps (TSG_STAMPS) once their tables are staged: the kernel's
// start, the end of its setup, the hardware id of the workgroup's CU.
__device__ __forceinline__ void stamp_begin(unsigned long long *stamps, uint32_t w, unsigned long long t_start, int tid) {
  if (stamps && tid == 0) {
    stamps[uint64_t(w) * kStampSlots] = t_start;
    stamps[uint64_t(w) * kStampSlots + 1] = __builtin_amdgcn_s_memrealtime();
    const unsigned long long hw = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
    const unsigned long long xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);
    stamps[uint64_t(w) * kStampSlots + 8] = (xcc << 32) | hw;
  }
}
// The pool and static kernels' end: once every wave has scanned its units, the LDS records to
// the workgroup's host segment (write-through), then the count.
__device__ __forceinline__ void hand_off_segment(const PoolArgs &A, const unsigned long long *s_rec,
                                                 const uint32_t *s_nrec, uint32_t w, int tid) {
  unsigned long long *const stamps = A.stamps;
  __syncthreads();
  if (stamps && tid == 0) {
    stamps[uint64_t(w) * kStampSlots + 2] = __builtin_amdgcn_s_memrealtime();
    stamps[uint64_t(w) * kStampSlots + 3] = __builtin_amdgcn_s_memrealtime();
  }
  const uint32_t total = *s_nrec;
  const uint32_t nw = min(total, min(A.rec_cap, A.seg_cap)) * 6;
  if (nw) {
    auto *dst = reinterpret_cast<unsigned long long *>(A.recs) + uint64_t(w) * A.seg_cap * 6;
    for (uint32_t i = tid; i < nw; i += A.nthreads) host_store(dst + i, s_rec[i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (tid == 0) {
    host_store(A.counts + w, total);
    if (stamps) stamps[uint64_t(w) * kStampSlots + 4] = __builtin_amdgcn_s_memrealtime();
  }
}

// ------------------------------------------------------------------------------------
template <int NT, bool DUR, bool RANGE, bool NTL, bool TF>
__global__ void __launch_bounds__(kPoolThreads, 1) search_pool_kernel(PoolArgs A) {
  const unsigned long long t_start = A.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
  __shared__ __attribute__((aligned(16))) PoolBlk s_blk[kArgSegs];
  __shared__ uint32_t s_ub[kArgSegs + 1], s_sb[kArgSegs];
  __shared__ __attribute__((aligned(16))) uint8_t s_tb[kArgBms * 256];  // the terms' byte tables
  __shared__ uint32_t s_chunk[kPoolChunks];
  __shared__ uint32_t s_next, s_nrec;
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_rec[];  // rec_cap x 6 words
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = blockIdx.x, nsegs = A.nsegs, units = A.units;
  const uint32_t S = A.static_per_wg, L = A.lookahead, cs = A.chunk_shift;
  const uint32_t wv = rfl(uint32_t(tid) >> 6), nwv = A.nthreads >> 6;
  struct Unit : UnitRegs<NT> {
    uint32_t blk;  // wave-uniform: the unit's block slot
  };
  // ---- the first two units of a wave, before anything is staged: a wave's first two claims
  // are wv and wv + nwv (claims below S map to the workgroup's static run in order), so their
  // loads go out with the block found by a scalar walk over the kernel arguments (the claims'
  // bookkeeping, a chunk request they may trigger, runs after the staging)
  Unit ra, rb;
  auto load_arg = [&](Unit &R, uint32_t u) {
    uint32_t b = 0;
    while (b + 1 < nsegs && u >= A.ubase[b + 1]) b++;
    R.blk = b;
    const PoolBlk &B = A.blk[b];
    load_unit<NT, DUR, RANGE, NTL, TF>(R, B.scan, B.npad, [&](int q) { return B.col[q]; },
                                   A.ebase[b] + (u - A.ubase[b]) * kPoolTile, lane);
  };
  // the staging's kernel-argument words first, by vector loads issued ahead of the units'
  // loads: vector loads complete in issue order, so the wait for these (before the LDS
  // writes below) does not wait for the burst of unit loads behind them. The units' loads
  // are unconditional (a wave without a unit reloads unit 0), so the compiler's count of the
  // loads issued after these is the same on every path.
  const uint32_t *blk_words = reinterpret_cast<const uint32_t *>(A.blk);
  const uint32_t xblk = uint32_t(tid) < nsegs * 16 ? blk_words[tid] : 0u;
  const uint32_t xub = uint32_t(tid) < nsegs ? A.blk[tid].ubase : units;
  const uint32_t xsb = uint32_t(tid) < nsegs ? A.sbase[tid] : 0u;
  const uint32_t xbm = NT > 0 ? reinterpret_cast<const uint32_t *>(A.bms)[tid >> 3] : 0u;  // (tid < 1024)
  const uint32_t xns = NT > 0 ? A.bm_ns[tid >> 6] : 0u;
  const bool pre0 = wv < S, pre1 = wv + nwv < S;
  uint32_t ua = kPoolNone, ub = kPoolNone;
  if (pre0 && uint64_t(w) * S + wv < units) ua = w * S + wv;
  if (pre1 && uint64_t(w) * S + wv + nwv < units) ub = w * S + wv + nwv;
  load_arg(ra, ua != kPoolNone ? ua : 0u);
  load_arg(rb, ub != kPoolNone ? ub : 0u);
  // ---- stage the launch's tables (scalar loads of the kernel arguments; the barrier does not
  // wait for the units' loads above)
  {
    static_assert(kArgSegs * 16 <= kPoolThreads, "one staging word per thread");
    if (uint32_t(tid) < nsegs * 16) reinterpret_cast<uint32_t *>(s_blk)[tid] = xblk;
    if (uint32_t(tid) <= nsegs) s_ub[tid] = xub;
    if (uint32_t(tid) < nsegs) s_sb[tid] = xsb;
    stage_term_tables<NT>(s_tb, A, xbm, xns, uint32_t(tid));
    for (uint32_t i = tid; i < kPoolChunks; i += A.nthreads) s_chunk[i] = kPoolPending;
    if (tid == 0) {
      s_next = min(2 * nwv, S);  // (the claims below it are the waves' first two)
      s_nrec = 0;
      if (w == 0) __hip_atomic_store(A.head_next, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  lds_barrier();
  stamp_begin(A.stamps, w, t_start, tid);
  const uint32_t rec_cap = A.rec_cap;
  const uint32_t dlo = A.has_min ? A.min32 : 0u, dhi = A.has_max ? A.max32 : 0xffffffffu;
  // An LDS chunk slot once its answer is in. Bounded: never reached unless the protocol
  // is broken, and then the query fails on the host instead of the GPU hanging.
  auto poll_chunk = [&](uint32_t k) -> uint32_t {
    uint32_t v, spins = 0;
    while ((v = __hip_atomic_load(&s_chunk[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == kPoolPending) {
      if (++spins > kPoolSpinMax) {
        host_store(A.err, 1u);
        return kPoolNone;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    return v;
  };
  // claim -> unit (or kPoolNone): claims below S are this workgroup's static run; claim
  // S + k*C + off is unit `off` of its k-th dynamic chunk, which the claim L before the
  // chunk's first one requested from the device counter (so a wave rarely waits for it)
  auto trigger = [&](uint32_t c) {
    if (c + L >= S) {
      const uint32_t t = c + L - S;
      const uint32_t k = t >> cs;
      if ((t & ((1u << cs) - 1)) == 0 && k < kPoolChunks) {
        // chunks are requested in order (chunk k after chunk k-1 has its answer), so once
        // one comes back empty every later one is empty too and a wave may stop at the
        // first empty claim without stranding units this workgroup took
        if (lane == 0) {
          uint32_t prev = 0;
          if (k > 0) prev = poll_chunk(k - 1);
          uint32_t val = kPoolNone;
          if (prev != kPoolNone) {
            const uint32_t g = __hip_atomic_fetch_add(A.head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t u0 = uint64_t(A.dyn0) + (uint64_t(g) << cs);
            if (u0 < units) val = uint32_t(u0);
          }
          __hip_atomic_store(&s_chunk[k], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
  };
  auto claim = [&]() -> uint32_t {
    uint32_t c = 0;
    if (lane == 0) c = atomicAdd(&s_next, 1u);
    c = __builtin_amdgcn_readfirstlane(c);
    trigger(c);
    if (c < S) {  // (a small search's last static runs end at `units`: past it, no work)
      const uint32_t u = w * S + c;
      return u < units ? u : kPoolNone;
    }
    const uint32_t d = c - S, k = d >> cs;
    if (k >= kPoolChunks) return kPoolNone;
    uint32_t v = poll_chunk(k);
    v = __builtin_amdgcn_readfirstlane(v);
    if (v == kPoolNone) return kPoolNone;
    const uint32_t u = v + (d & ((1u << cs) - 1));
    return u < units ? u : kPoolNone;
  };
  // after the staging: the block and its fields from LDS
  auto load = [&](Unit &R, uint32_t u) {
    const uint32_t b = block_of(s_ub, nsegs, u, lane);
    R.blk = b;
    const PoolBlk &B = s_blk[b];
    const uint32_t npad = rfl(B.npad);
    const uint32_t *scan = uniform_ptr(B.scan);
    load_unit<NT, DUR, RANGE, NTL, TF>(R, scan, npad, [&](int q) { return uniform_ptr(B.col[q]); },
                                   rfl(A.ebase[b]) + (u - rfl(B.ubase)) * kPoolTile, lane);
  };
  auto eval = [&](const Unit &R) {
    const PoolBlk &B = s_blk[R.blk];
    const UnitPred<NT> P = unit_pred<NT>(dlo, dhi, A.start_s, A.end_s, rfl(s_sb[R.blk]), rfl(B.nent), rfl(B.bmi4));
    uint32_t mask = unit_mask<NT, DUR, RANGE, NTL, TF>(R, P, s_tb, uniform_ptr(B.scan), rfl(B.npad), lane);
    if (__ballot(mask != 0) == 0) return;
    if (A.unit_cap) mask = cap_unit_mask(mask, A.unit_cap, lane);
    put_unit(s_rec, &s_nrec, rec_cap, mask, A.desc[R.blk], rfl(B.block_idx), R.e0, lane);
  };
  // ---- scan: two units in flight per wave (the first two loaded above when static). Every
  // claim index is triggered exactly once, by the wave that holds it, whether or not it
  // maps to a unit: a chunk request it owes is polled by later claims
  if (pre0) trigger(wv);
  if (pre1) trigger(wv + nwv);
  if (!pre0) {
    ua = claim();
    if (ua != kPoolNone) load(ra, ua);
  }
  if (ua != kPoolNone) {
    if (!pre1) {
      ub = claim();
      if (ub != kPoolNone) load(rb, ub);
    }
    for (;;) {
      eval(ra);
      if (ub == kPoolNone) break;
      ua = claim();
      if (ua != kPoolNone) load(ra, ua);
      eval(rb);
      if (ua == kPoolNone) break;
      ub = claim();
      if (ub != kPoolNone) load(rb, ub);
    }
  }
  hand_off_segment(A, s_rec, &s_nrec, w, tid);
}

// ------------------------------------------------------------------------------------
// static search: the pool kernel's loads, predicates and record hand-off without its
// machinery. One 1024-thread workgroup per CU; wave g of the launch owns the contiguous
// unit run [g * sq + min(g, sr), ...) of the launch's unit space (NW waves, runs differ
// by at most one unit), two units in flight. The block of a unit comes from the wave's own
// walk over the kernel arguments' unit bases (scalar loads, once per block boundary), not
// from LDS: the first loads are issued before anything is staged, and nothing is claimed.
// (scan_probe.hip measured this shape at 27.0 us for 150 MB against 32.4 us for the pool
// kernel with its LDS claims, staging and dynamic chunks.)
template <int NT, bool DUR, bool RANGE, bool NTL, bool TF>
__global__ void __launch_bounds__(kPoolThreads, 1) search_static_kernel(PoolArgs A) {
  const unsigned long long t_start = A.stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
  __shared__ __attribute__((aligned(16))) uint8_t s_tb[kArgBms * 256];  // the terms' byte tables
  __shared__ uint32_t s_nrec;
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_rec[];  // rec_cap x 6 words
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = blockIdx.x, nsegs = A.nsegs, units = A.units;
  const uint32_t nwv = A.nthreads >> 6;
  const uint32_t wave = rfl(uint32_t(tid) >> 6);
  const uint32_t gw = w * nwv + wave;
  const uint32_t u_begin = gw * A.sq + min(gw, A.sr), u_end = u_begin + A.sq + (gw < A.sr ? 1u : 0u);
  // the wave's current block (all scalar)
  uint32_t b = 0;
  while (b + 1 < nsegs && u_begin >= A.ubase[b + 1]) b++;
  struct Blk {
    const uint32_t *scan;
    const uint8_t *col[NT > 0 ? NT : 1];
    uint32_t npad, nent, ub, ue, eb, bmi4, nsets4, block_idx;
  } B;
  auto set_block = [&](uint32_t bb) {
    const PoolBlk &P = A.blk[bb];
    B.scan = P.scan;
#pragma unroll
    for (int q = 0; q < (NT > 0 ? NT : 1); q++)
      if (NT > 0) B.col[q] = P.col[q];
    B.npad = P.npad;
    B.nent = P.nent;
    B.ub = A.ubase[bb];
    B.ue = A.ubase[bb + 1];
    B.eb = A.ebase[bb];
    B.bmi4 = P.bmi4;
    B.nsets4 = P.nsets4;
    B.block_idx = P.block_idx;
  };
  set_block(b);
  using Unit = UnitRegs<NT>;
  auto load = [&](Unit &R, uint32_t u) {
    if (u >= B.ue) {  // (runs are short and blocks long: at most a step or two)
      while (b + 1 < nsegs && u >= A.ubase[b + 1]) b++;
      set_block(b);
    }
    load_unit<NT, DUR, RANGE, NTL, TF>(R, B.scan, B.npad, [&](int q) { return B.col[q]; },
                                   B.eb + (u - B.ub) * kPoolTile, lane);
  };
  const uint32_t rec_cap = A.rec_cap;
  const uint32_t dlo = A.has_min ? A.min32 : 0u, dhi = A.has_max ? A.max32 : 0xffffffffu;
  // (evaluated right after the unit's load, while the block state still describes it)
  auto eval = [&](const Unit &R, uint32_t bslot) {
    const PoolBlk &P = A.blk[bslot];
    const UnitPred<NT> U = unit_pred<NT>(dlo, dhi, A.start_s, A.end_s, A.sbase[bslot], P.nent, P.bmi4);
    uint32_t mask = unit_mask<NT, DUR, RANGE, NTL, TF>(R, U, s_tb, P.scan, P.npad, lane);
    if (__ballot(mask != 0) == 0) return;
    if (A.unit_cap) mask = cap_unit_mask(mask, A.unit_cap, lane);
    put_unit(s_rec, &s_nrec, rec_cap, mask, A.desc[bslot], P.block_idx, R.e0, lane);
  };
  // the bitmap words by vector loads issued ahead of the first unit's loads (in-order
  // completion: their wait does not wait for those); the first unit's loads are
  // unconditional (a wave without units reloads the launch's last unit), so every path issues
  // the same loads after these
  const uint32_t xbm = NT > 0 ? reinterpret_cast<const uint32_t *>(A.bms)[tid >> 3] : 0u;  // (tid < 1024)
  const uint32_t xns = NT > 0 ? A.bm_ns[tid >> 6] : 0u;
  Unit ra, rb;
  uint32_t u = u_begin, ba = b, bb = b;
  load(ra, u < u_end ? u : (units ? units - 1 : 0u));
  ba = b;
  stage_term_tables<NT>(s_tb, A, xbm, xns, uint32_t(tid));
  if (tid == 0) s_nrec = 0;
  lds_barrier();  // (not waiting for the first unit's loads)
  stamp_begin(A.stamps, w, t_start, tid);
  // two units in flight: ra (u), rb (u + 1)
  while (u < u_end) {
    const bool has_b = u + 1 < u_end;
    if (has_b) {
      load(rb, u + 1);
      bb = b;
    }
    eval(ra, ba);
    if (!has_b) break;
    const bool has_a = u + 2 < u_end;
    if (has_a) {
      load(ra, u + 2);
      ba = b;
    }
    eval(rb, bb);
    u += 2;
  }
  hand_off_segment(A, s_rec, &s_nrec, w, tid);
}

// ------------------------------------------------------------------------------------
// resident search (TSG_RESIDENT): the static kernel's scan as a kernel that stays on the
// device and takes its queries from a mailbox.
//
// A narrow search's kernel launch costs more than its own duration suggests: the command
// processor fetches the AQL packet over PCIe after the doorbell, runs the acquire fence, then
// launches 4096 waves, whose first loads go out together and whose kernel-argument loads
// queue behind them (the round-4 staging barrier passed 7 us into a 24 us kernel). A
// resident launch has its waves in place: the host writes a query's arguments into a
// mailbox slot of uncached device memory through the BAR, then the slot's header, then the
// doorbell word; each workgroup's first lane polls the doorbell, the workgroup loads the
// slot into LDS (one word per thread), checks the header's sequence number and the checksum
// of the words the query uses (a slot read before the host's writes landed is read again),
// and scans.
//
// Records come out in scan order: wave g of the launch owns a contiguous unit run (the
// static split), keeps its matches in its own LDS region in scan order (ranks from per-step
// ballots), and the workgroup writes its waves' regions one after another to its host
// segment; workgroup w's runs precede workgroup w+1's, so the segments in workgroup order
// are the reference order and the host only concatenates them (no sort). A wave whose
// region overflows reports the workgroup as overflowing (the host reruns the query on the
// other paths).
//
// Lifetime: a workgroup leaves when the host posts a quit, or when no query has been posted
// for idle_ticks of the 100 MHz clock (every wave reaches one of the two); the host relaunches
// at its next query. A post that races the idle exit is seen by the host as the launch
// completing with counts missing: it relaunches and posts again (pool.hip resident_*).
constexpr uint32_t kResSlots = 64, kResSlotBytes = 8192, kResHdrBytes = 64;
constexpr uint32_t kResSearch = 1, kResQuit = 2;
constexpr uint32_t kResMaxUnits = 2048;  // units per workgroup (the LDS tables); larger queries launch plainly
constexpr uint32_t kResRejectWord = 8;   // ResidentArgs::err word counting rejected slot reads
// a timed query's {seen, end} stamps, one 64-byte line per workgroup: four workgroups' 16-byte
// stamps in one line had been partial-line writes to a shared line from four CUs, which land one
// after another (the count lines' lesson, round 5): ~5 us more per timed query
constexpr uint32_t kResStampStride = 8;
struct ResHeader {  // the first 16 B of a mailbox slot; PoolArgs at +kResHdrBytes
  uint32_t seq, cmd, h0, h1;  // h0, h1: res_hash of (seq, cmd, the used argument words)
};
// The slot check: two independently keyed 32-bit sums of a nonlinear per-word mix of (word, its
// index, seq). A slot read while the host's writes were still landing holds some words of query
// seq - kResSlots: an additive checksum accepted any such mix whose plain sum happened to equal
// the new one; here a stale/new mix passes with probability ~2^-64, and a stale
// header (another seq, another cmd) never does.
__host__ __device__ inline uint32_t res_mix(uint32_t x, uint32_t wi, uint32_t seq, uint32_t key) {
  uint32_t h = x ^ (wi * 0x9E3779B1u) ^ (seq * 0x85EBCA77u) ^ key;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}
constexpr uint32_t kResKey0 = 0x2545F491u, kResKey1 = 0x6C8E9CF5u;
constexpr uint32_t kResCmdWord = 0xffffffffu;  // (the word index the command is mixed under)
struct ResidentArgs {
  const uint32_t *door;  // uncached device memory: [0] = the last posted sequence number
  const uint8_t *slots;  // uncached device memory: kResSlots x kResSlotBytes (slot = seq % kResSlots)
  uint32_t *err;         // pinned host: [0] set when a slot never verified (the host fails the query),
                         // [kResRejectWord] the slot reads a workgroup rejected (hash mismatch) for a query
  uint32_t first_seq;    // the first query of this launch
  uint32_t idle_ticks;   // s_memrealtime ticks without a post before a workgroup leaves
  uint32_t nthreads, ngroups;
  uint32_t mode, pad;  // TSG_RES_MODE (experiments): bit 0 = units interleaved over the waves (no LDS claims),
                       // bit 3 = no gathers (zero records), bit 4 = no records stored (counts only),
                       // bit 2 = poll the slot header alone, load the arguments once it shows the query,
                       // bit 1 = longer sleeps between doorbell polls
};
static_assert(sizeof(PoolArgs) <= kResSlotBytes - kResHdrBytes && sizeof(PoolArgs) % 4 == 0, "mailbox slot");

// 12 waves per workgroup (one workgroup per CU): 168 registers per lane, where the pool kernels'
// 16 waves allow 128 and this kernel's state (two units in flight, the mailbox checks, the
// ordered record output) spilled to scratch; 24 units in flight per CU still cover the HBM
// latency (config 2: 34 MB in flight)
constexpr uint32_t kResWaves = 12, kResThreads = kResWaves * 64;
constexpr uint32_t kResMaxRecs = uint32_t(kPoolLds / sizeof(MatchRec));  // the LDS record buffer
template <int NT, bool DUR, bool RANGE, bool NTL, bool TF>
__global__ void __launch_bounds__(kResThreads, 1) search_resident_kernel(ResidentArgs R) {
  __shared__ __attribute__((aligned(16))) uint32_t s_args[sizeof(PoolArgs) / 4];
  __shared__ __attribute__((aligned(16))) uint8_t s_tb[kArgBms * 256];  // the terms' byte tables
  __shared__ uint32_t s_ctl[4];   // [0] command for this round, [1] checksum, [2] header seq, [3] header csum
  __shared__ uint32_t s_wn[kPoolWaves + 1];
  __shared__ uint32_t s_ub[kResMaxUnits], s_uc[kResMaxUnits];  // per unit of the run: LDS record base, count
  __shared__ uint32_t s_map[kResMaxRecs];  // output record p (scan order) -> its LDS record
  __shared__ uint32_t s_next, s_nrec;
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_rec[];  // rec_cap x 6 words
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t w = blockIdx.x, nthreads = R.nthreads, nwv = nthreads >> 6;
  const uint32_t wave = rfl(uint32_t(tid) >> 6);
  const PoolArgs &A = *reinterpret_cast<const PoolArgs *>(s_args);
  constexpr uint32_t kWords = uint32_t(sizeof(PoolArgs) / 4);
  for (uint32_t seq = R.first_seq;; seq++) {
    // ---- wait for query `seq`: wave 0 polls its mailbox slot itself (header + the argument
    // struct, 16-byte system-coherent loads: 52 lines per poll), so the poll that sees the
    // header's sequence number already holds the arguments; they count when the checksum of
    // the words the query uses matches the header's (a slot read while the host's writes were
    // still landing is read again). No post for idle_ticks: the workgroup leaves.
    const uint8_t *slot = R.slots + uint64_t(seq % kResSlots) * kResSlotBytes;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(slot + kResHdrBytes);
    if (wave == 0) {
      constexpr uint32_t kQuads = (kWords + 3) / 4;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      uint32_t got = 0, bad = 0;  // got: 1 verified, 2 idle, 3 never verified
      const bool hdr_first = (R.mode & 4u) != 0;  // (experiment: poll the header line alone, then load the slot)
      for (uint32_t n = 0; !got; n++) {
        u32x4 hq, v[(kQuads + 63) / 64];
        {
          const u32x4 *hp = reinterpret_cast<const u32x4 *>(slot);
          asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(hq) : "v"(hp) : "memory");
        }
        if (hdr_first) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (rfl(hq.x) != seq) {
            if ((n & 15u) == 15u && __builtin_amdgcn_s_memrealtime() - t0 > R.idle_ticks) got = 2;
            else __builtin_amdgcn_s_sleep(2);
            continue;
          }
        }
#pragma unroll
        for (uint32_t k = 0; k < (kQuads + 63) / 64; k++) {
          const uint32_t qi = min(k * 64 + uint32_t(lane), kQuads - 1);
          const u32x4 *qp = reinterpret_cast<const u32x4 *>(words) + qi;
          asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v[k]) : "v"(qp) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t hseq = rfl(hq.x);
        if (hseq != seq) {  // not posted yet
          if ((n & 15u) == 15u && __builtin_amdgcn_s_memrealtime() - t0 > R.idle_ticks) got = 2;
          else if (R.mode & 2u) __builtin_amdgcn_s_sleep(32);
          else __builtin_amdgcn_s_sleep(2);
          continue;
        }
        // nsegs / nbms, from the lanes holding them
        constexpr uint32_t kNs = uint32_t(offsetof(PoolArgs, nsegs) / 4), kNb = uint32_t(offsetof(PoolArgs, nbms) / 4);
        uint32_t ns = 0, nb = 0;
#pragma unroll
        for (uint32_t k = 0; k < (kQuads + 63) / 64; k++) {
          const uint32_t w0 = (k * 64 + uint32_t(lane)) * 4;
          const uint32_t x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
          for (uint32_t j = 0; j < 4; j++) {
            if (w0 + j == kNs) ns = x[j];
            if (w0 + j == kNb) nb = x[j];
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          ns |= __shfl_xor(ns, o);
          nb |= __shfl_xor(nb, o);
        }
        const uint32_t cmd = rfl(hq.y);
        uint32_t p0 = 0, p1 = 0;
        const bool sane = ns <= uint32_t(kArgSegs) && nb <= uint32_t(kArgBms) && cmd == kResSearch;
#pragma unroll
        for (uint32_t k = 0; k < (kQuads + 63) / 64; k++) {
          const uint32_t qi = k * 64 + uint32_t(lane);
          if (qi >= kQuads) continue;
          const uint32_t x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
          for (uint32_t j = 0; j < 4; j++) {
            const uint32_t wi = qi * 4 + j;
            if (wi < kWords) {
              s_args[wi] = x[j];
              if (sane && res_word_used(4 * wi, ns, nb)) {
                p0 += res_mix(x[j], wi, seq, kResKey0);
                p1 += res_mix(x[j], wi, seq, kResKey1);
              }
            }
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          p0 += __shfl_xor(p0, o);
          p1 += __shfl_xor(p1, o);
        }
        p0 += res_mix(cmd, kResCmdWord, seq, kResKey0);
        p1 += res_mix(cmd, kResCmdWord, seq, kResKey1);
        const bool vok = (cmd == kResQuit || sane) && p0 == hq.z && p1 == hq.w;
        if (__builtin_amdgcn_readfirstlane(uint32_t(vok))) {
          got = 1;
          if (lane == 0) {
            s_ctl[0] = cmd;
            if (bad) host_store(R.err + kResRejectWord, bad);
          }
        } else if (++bad > 4096) {
          got = 3;
        } else {
          __builtin_amdgcn_s_sleep(2);
        }
      }
      if (lane == 0) s_ctl[1] = got;
    }
    __syncthreads();
    const unsigned long long t_seen = __builtin_amdgcn_s_memrealtime();
    if (s_ctl[1] == 2) return;  // idle
    const bool ok = s_ctl[1] == 1;
    if (!ok) {  // the slot never verified: the host fails the query (err)
      if (tid == 0) host_store(R.err, 1u);
      return;
    }
    if (s_ctl[0] == kResQuit) return;
    // ---- the query. Workgroup w owns the contiguous unit run [ua, ua + nk) (runs differ by at
    // most one unit: every CU the same share); its waves take the run's units one at a time
    // from an LDS counter (the first two of each wave implied), so they finish together; a
    // unit's matches go to the LDS record buffer at once, in scan order, and the unit
    // remembers where (s_ub / s_uc). At the end the units' counts are prefix-summed and each
    // unit's records written to the workgroup's host segment at its offset: the segment is in
    // scan order whichever wave took which unit.
    const uint32_t nsegs = rfl(A.nsegs);
    const uint32_t wq = rfl(A.wq), wr = rfl(A.wr);
    uint32_t ua = w * wq + min(w, wr), nk = wq + (w < wr ? 1u : 0u);
    if (rfl(A.xsplit)) {
      // XCD-weighted runs (the host's measured per-XCD rates, res_split): workgroup w = 8i + x;
      // the runs of every workgroup before it, in workgroup order
      const uint32_t x = w & 7u, i = w >> 3;
      uint32_t s = 0;
#pragma unroll
      for (uint32_t y = 0; y < 8; y++) {
        const uint32_t n = rfl(A.xn[y]), r = rfl(A.xr[y]);
        s += i * n + min(i, r) + (y < x ? n + (i < r ? 1u : 0u) : 0u);
      }
      ua = s;
      nk = rfl(A.xn[x]) + (i < rfl(A.xr[x]) ? 1u : 0u);
    }
    const uint32_t rec_cap = rfl(A.rec_cap);
    const uint32_t dlo = rfl(A.has_min ? A.min32 : 0u), dhi = rfl(A.has_max ? A.max32 : 0xffffffffu);
    const uint32_t start_s = rfl(A.start_s), end_s = rfl(A.end_s), ucap = rfl(A.unit_cap);
    // the block of the wave's last load (its fields are read from LDS per load); from the
    // block holding the run's first unit (a walk from block 0 had put up to nsegs dependent LDS
    // reads before a late workgroup's first loads)
    uint32_t b = block_of(A.ubase, nsegs, ua, lane);
    struct Unit : UnitRegs<NT> {
      uint32_t k;  // the unit's place in the workgroup's run
    };
    // (a wave's claims only grow: the block walk only moves forward)
    auto load = [&](Unit &Rg, uint32_t k) {
      const uint32_t u = ua + k;
      while (b + 1 < nsegs && u >= rfl(A.ubase[b + 1])) b++;
      const PoolBlk &P = A.blk[b];
      const uint32_t *scan = uniform_ptr(P.scan);
      const uint32_t npad = rfl(P.npad);
      Rg.k = k;
      load_unit<NT, DUR, RANGE, NTL, TF>(Rg, scan, npad, [&](int q) { return uniform_ptr(P.col[q]); },
                                     rfl(A.ebase[b]) + (u - rfl(A.ubase[b])) * kPoolTile, lane);
    };
    // the unit's matches into the LDS buffer in scan order (k-step, lane, j), in two halves:
    // eval_a finds them, ranks them and issues the gathers of each lane's first match into a
    // Pend (registers); eval_b stores them to LDS one unit of the same stream later (the loop
    // below). A lane's further matches (rare) are gathered and stored at once. A gather is a
    // full memory latency under the scan's load: waited for before the next unit's loads it had
    // left the wave one unit in flight meanwhile (workgroups holding matches ended ≈ 0.8 us
    // after those without); waited for right after them, ≈ 0.17 us per record (r06 stamps,
    // profiles/r06_xsplit/analysis.txt); one unit later, nothing: the wave waits there for the
    // loads issued after the gathers anyway.
    struct Pend {
      u32x4 id;
      uint64_t st, en, nm;
      uint32_t ei, r, ilw, bidx;  // ilw: the aligned word holding the id length byte
      bool has;
    };
    auto eval_a = [&](const Unit &Rg, Pend &Pd) {
      Pd.has = false;
      const uint32_t blk = block_of(A.ubase, nsegs, ua + Rg.k, lane);
      const PoolBlk &P = A.blk[blk];
      const UnitPred<NT> U = unit_pred<NT>(dlo, dhi, start_s, end_s, rfl(A.sbase[blk]), rfl(P.nent), rfl(P.bmi4));
      uint32_t mask = unit_mask<NT, DUR, RANGE, NTL, TF>(Rg, U, s_tb, uniform_ptr(P.scan), rfl(P.npad), lane);
      if (__ballot(mask != 0) == 0) return;
      if (ucap) mask = cap_unit_mask(mask, ucap, lane);
      uint32_t cnt = uint32_t(__popc(mask));
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
      cnt = rfl(cnt);
      if (!cnt) return;
      uint32_t base = 0;
      if (lane == 0) {
        base = atomicAdd(&s_nrec, cnt);
        s_ub[Rg.k] = base;
        s_uc[Rg.k] = cnt;
      }
      base = rfl(base);
      const ColdCols C = cold_cols(uniform_ptr(A.desc[blk]));
      const uint32_t bidx = rfl(P.block_idx);
      Pd.bidx = bidx;
      // each step's first LDS record for this lane
      uint32_t rank0[kSteps], total;
      unit_ranks(mask, lane, rank0, total);
#pragma unroll
      for (int kk = 0; kk < kSteps; kk++) rank0[kk] += base;
      if (!mask) return;
      {
        const uint32_t bit = uint32_t(__builtin_ctz(mask));
        const uint32_t r = match_rank(rank0, mask, bit);
        const uint32_t ei = Rg.e0 + (bit >> 2) * 256 + uint32_t(lane) * 4 + (bit & 3u);
        if (r < rec_cap && (R.mode & 8u)) {  // (experiment: no gathers, zero records)
          Pd.has = true;
          Pd.ei = ei;
          Pd.r = r;
          Pd.id = u32x4{0, 0, 0, 0};
          Pd.st = Pd.en = Pd.nm = 0;
          Pd.ilw = 0;
        } else if (r < rec_cap) {
          Pd.has = true;
          Pd.ei = ei;
          Pd.id = *G<u32x4>(C.ids + uint64_t(ei) * 16);
          Pd.st = G(C.st_ns)[ei];
          Pd.en = G(C.en_ns)[ei];
          Pd.nm = G(C.names)[ei];
          // (the id length's aligned word, untouched until the store: no arithmetic on a
          // gathered value here, or the wave waits for the gathers at once)
          Pd.r = r;
          Pd.ilw = *G<uint32_t>(C.id_len + (ei & ~3u));
        }
      }
      // a lane's further matches, one at a time (a loop kept rolled: the gathers of 8 records
      // at once had pushed the kernel past its registers)
#pragma unroll 1
      for (uint32_t m = mask & (mask - 1u); m; m &= m - 1) {
        const uint32_t bit = uint32_t(__builtin_ctz(m));
        const uint32_t r = match_rank(rank0, mask, bit);
        if (r >= rec_cap) continue;
        gather_put(s_rec, r, C, Rg.e0 + (bit >> 2) * 256 + uint32_t(lane) * 4 + (bit & 3u), bidx);
      }
    };
    auto eval_b = [&](const Pend &Pd) {
      if (Pd.has)
        put_rec(s_rec, Pd.r, Pd.id, Pd.st, Pd.en, Pd.ei, Pd.bidx, (Pd.ilw >> (8 * (Pd.ei & 3u))) & 0xffu, Pd.nm);
    };
    const bool interleave = (R.mode & 1u) != 0;
    auto claim = [&](uint32_t prev) -> uint32_t {
      if (interleave) return prev + 2 * nwv;
      uint32_t c = 0;
      if (lane == 0) c = atomicAdd(&s_next, 1u);
      return 2 * nwv + rfl(c);
    };
    Unit ra, rb;
    uint32_t ka = wave, kb = wave + nwv;
    if (ka < nk) load(ra, ka);
    if (kb < nk) load(rb, kb);
    // the query's LDS tables once the first loads are out (they read the arguments only): the
    // units' counts, the claim and record counters, the terms' byte tables; the barrier waits for
    // LDS alone, not for those loads
    for (uint32_t i = uint32_t(tid); i < nk; i += nthreads) s_uc[i] = 0;
    if (NT > 0)
      for (uint32_t i = uint32_t(tid), n = min(rfl(A.nbms), uint32_t(kArgBms)) * 64; i < n; i += nthreads)
        stage_term_dword(s_tb, i, reinterpret_cast<const uint32_t *>(A.bms)[i >> 3], A.bm_ns[i >> 6]);
    if (tid == 0) {
      s_next = 0;
      s_nrec = 0;
    }
    lds_barrier();
    // a unit's gathers are stored one unit later (eval_b of unit n of a stream runs before
    // eval_a of unit n+1 of the same stream): by then the loads issued after them are being
    // waited for anyway (vector loads complete in order), so a match costs the wave no stall
    Pend pa, pb;
    pa.has = pb.has = false;
    // ---- the steady state: both streams hold a unit and every claim yields one, so a stream's
    // next loads are issued with no branch around them. The compiler's count of the loads in
    // flight is then exact where it matters: the wait before a unit's registers are first used
    // leaves the other stream's eight loads outstanding (vmcnt >= 8). With the loads under
    // `if (k < nk)` the count at that wait was merged with the path that skips them, to 0: every
    // unit drained the loads just issued, one unit in flight per wave, not two
    // (profiles/res_inflight). Stream a's first unit is evaluated ahead of the loop: at a loop
    // head its wait would be merged with the entry path, where the first two loads are
    // conditional. The units, the claims and their order are those of the loop below, which
    // takes over as soon as a claim comes back past the run (and is all a wave with two units or
    // fewer runs).
    if (ka < nk && kb < nk) {
      eval_b(pa);
      eval_a(ra, pa);
      ka = claim(ka);
      if (ka < nk) {
        load(ra, ka);
        for (;;) {
          eval_b(pb);
          eval_a(rb, pb);
          kb = claim(kb);
          if (kb >= nk) break;
          load(rb, kb);
          eval_b(pa);
          eval_a(ra, pa);
          ka = claim(ka);
          if (ka >= nk) break;
          load(ra, ka);
        }
      }
    }
    while (ka < nk || kb < nk) {
      if (ka < nk) {
        eval_b(pa);
        eval_a(ra, pa);
        ka = claim(ka);
        if (ka < nk) load(ra, ka);
      }
      if (kb < nk) {
        eval_b(pb);
        eval_a(rb, pb);
        kb = claim(kb);
        if (kb < nk) load(rb, kb);
      }
    }
    eval_b(pa);
    eval_b(pb);
    __syncthreads();
    // ---- units' counts -> exclusive offsets (s_uc in place), then each unit's records to the
    // host segment at its offset, then the count
    const uint32_t total = s_nrec;
    // (two units per thread per pass: a run longer than 2 x nthreads units takes more passes,
    // each carrying the previous passes' total)
    for (uint32_t base = 0, carry = 0; base < nk; base += 2 * nthreads) {
      const uint32_t i0 = base + 2 * uint32_t(tid), i1 = i0 + 1;
      const uint32_t c0 = i0 < nk ? s_uc[i0] : 0u, c1 = i1 < nk ? s_uc[i1] : 0u;
      const uint32_t mine = c0 + c1;
      uint32_t incl = mine;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
      }
      if (lane == 63) s_wn[wave] = incl;
      __syncthreads();
      uint32_t woff = 0, pass = 0;
      for (uint32_t v = 0; v < nwv; v++) {
        const uint32_t t = s_wn[v];
        if (v < wave) woff += t;
        pass += t;
      }
      const uint32_t ex = carry + woff + incl - mine;
      __syncthreads();  // (every c0 / c1 / s_wn read before they are overwritten)
      if (i0 < nk) s_uc[i0] = ex;
      if (i1 < nk) s_uc[i1] = ex + c0;
      carry += pass;
      __syncthreads();
    }
    const uint32_t seg_cap = rfl(A.seg_cap);
    const bool over = total > rec_cap;
    if (!over && total <= seg_cap && total && !(R.mode & 16u)) {  // (mode 16: experiment, no records out)
      // output record p -> its LDS record: each unit with matches writes its range of the map
      // (a binary search of the offsets per output word had been ~7 dependent LDS reads)
      for (uint32_t k = uint32_t(tid); k < nk; k += nthreads) {
        const uint32_t o = s_uc[k], o1 = k + 1 < nk ? s_uc[k + 1] : total;
        for (uint32_t p = o; p < o1; p++) s_map[p] = s_ub[k] + (p - o);
      }
      __syncthreads();
      // consecutive lanes store consecutive words of the segment (the fabric merges them into
      // whole-line PCIe writes; a record per thread, 8-byte stores each, had been 8x the
      // transactions and made the host wait ~50 us per query for the last count)
      auto *dst0 = reinterpret_cast<unsigned long long *>(uniform_ptr(A.recs)) + uint64_t(w) * seg_cap * 6;
      for (uint32_t i = uint32_t(tid); i < total * 6; i += nthreads) {
        const uint32_t p = i / 6, j = i - p * 6;
        host_store(dst0 + i, s_rec[uint64_t(s_map[p]) * 6 + j]);
      }
    }
    const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the count last (more matches than the LDS buffer holds: the host reruns the query on the
    // segment / look-back path)
    // with the low 32 bits of the seen / end stamps in the same 16-byte store: a timed query's
    // span costs no store of its own (separate stamp stores had cost ~4-6 us per timed query:
    // before the count, the count waited for their round trip; after it, the next query's first
    // waits did)
    if (tid == 0) {
      uint32_t *cl = uniform_ptr(A.counts) + uint64_t(w) * max(1u, rfl(A.cstride));
      const u32x4 v = {over ? max(total, rec_cap + 1) : total, uint32_t(t_seen), uint32_t(t_end), 0u};
      asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(cl), "v"(v) : "memory");
    }
    // the full stamps (diagnostics: TSG_RES_DUMP, the XCD calibration) after the count
    if (tid == 0 && A.qstamps) {  // (a 64-byte line per workgroup: kResStampStride)
      unsigned long long *qs = uniform_ptr(A.qstamps) + uint64_t(w) * kResStampStride;
      host_store(qs, t_seen);
      host_store(qs + 1, t_end);
    }
    __syncthreads();  // (the LDS tables are reused by the next query)
  }
}

}  // namespace tsg
