// find.hip — tempodb.Find on MI355X: bloom + index (lookup.hip) and then findOne on the
// device: the data page each hit's index record names is decompressed in HBM and its
// objects are scanned for the exact trace id.
//
//   findOne                        tempodb/encoding/v2/finder_paged.go:79-110
//   dataReader.Read (one record)   tempodb/encoding/v2/data_reader.go:45-125
//   page framing                   tempodb/encoding/v2/page.go:28-57
//   object framing / iterator      tempodb/encoding/v2/object.go:50-80 (the reader form), iterator.go
//   snappy framed stream           vendor/github.com/golang/snappy/decode.go:121-232, snappy_dev.hpp;
//                                  block format decode_other.go:41-102
//   lz4 frame (lz4-64k .. lz4)     vendor/github.com/pierrec/lz4/v4/reader.go, lz4_dev.hpp
//   zstd frame                     RFC 8878, zstd_dev.hpp
//
// Per batch: (1) the distinct (block, record) pages of the lookup hits, (2) a size pass
// (one lane per page walks the frame headers), (3) decode: one wave per page, each
// snappy chunk (<= 64 KiB decoded; snapdev::ChunkWalk gives the chunks, as in the size pass)
// staged and decoded in LDS with all 64 lanes (snap_block_wave: tags
// parsed in lockstep, literal and match bytes copied in parallel: a match of offset o
// is periodic, byte j = out[d - o + j % o], so no lane waits on another), CRC32C of the
// chunk per lane segment and combined, then written to HBM coalesced; (4) object scan:
// one wave per page walks the objects through 64 KiB LDS windows and the lanes compare
// each object id against the page's pending ids (first exact match, as findOne);
// (5) the found objects are gathered into one arena for the copy back.
// Encodings (page_codec(), common.hpp; the three codec headers have one shape: constants, a frame
// walker and a size function, built for the host too, and this file holds their wave-level
// kernels): none, snappy, zstd (zstd_dev.hpp; find_decode_zstd_wave_kernel: one wave per page,
// step (3'z) below; the older one-lane kernel behind tsg_debug_set "zstd_find_lane") and the four lz4 ones
// (lz4_dev.hpp parses the frame; find_decode_lz4_kernel: one wave per page, each block
// decoded through a 64 KiB output ring in LDS, step (3'') below); gzip / s2 report
// TSG_E_UNSUPPORTED_ENCODING per hit (the caller's CPU path takes those blocks).
// A block opened with TSG_V2_DATA_ON_DEMAND has no page in HBM: step (1) also plans rounds over
// its pages (find_rounds.hpp), and each round's pages are read from the data file into pinned
// memory and copied to dc.fstage before steps (2) to (5) run on them (the host part, below).
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <numeric>
#include <thread>

#include "devctx.hpp"
#include "find_rounds.hpp"
#include "lz4_dev.hpp"
#include "snappy_dev.hpp"
#include "zstd_dev.hpp"

namespace tsg {

struct FindPage {
  const uint8_t *src;  // v2 page: [u32 total][u16 hdr len][payload]
  uint64_t out_off;    // decoded bytes in the arena
  uint32_t len;        // index record length (the page's bytes)
  uint32_t enc;        // backend.Encoding
  uint32_t out_len;    // decoded size (size pass)
  int32_t status;      // TSG_OK or the page's error
  uint32_t hit0, nhit; // this page's pending ids: hits [hit0, hit0 + nhit)
  constexpr PageCodec codec() const { return page_codec(int(enc)); }
};

constexpr uint32_t kFindWindow = 65536;  // object scan window (LDS)
using lz4dev::rd32;                      // the file's one little-endian 32-bit read

// (2) decoded size of each page; framing errors are recorded here
extern "C" __global__ void __launch_bounds__(256) find_size_kernel(FindPage *pages, uint32_t npages) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npages) return;
  FindPage &P = pages[i];
  P.out_len = 0;
  if (P.status != TSG_OK) return;  // (the host's verdict: no data file, a record past its end, a failed read)
  // unmarshalPageFromBytes with the data header (length 0) (page.go:28-57)
  if (P.len < 6 || rd32(P.src) != P.len || (uint32_t(P.src[4]) | uint32_t(P.src[5]) << 8) != 0) {
    P.status = TSG_E_CORRUPT;
    return;
  }
  const uint8_t *b = P.src + 6;
  const uint32_t n = P.len - 6;
  uint64_t sz = n;
  switch (P.codec()) {
    case PageCodec::None: P.status = TSG_OK; break;
    case PageCodec::Snappy: P.status = snapdev::snappy_size(b, n, sz); break;  // the chunks' declared lengths
    case PageCodec::Lz4: P.status = lz4dev::lz4_size(b, n, sz); break;  // the content size, or the blocks' tokens walked
    case PageCodec::Zstd: P.status = zdev::zstd_size(b, n, sz); break;  // frame content sizes (or block bounds)
    case PageCodec::Unsupported: P.status = TSG_E_UNSUPPORTED_ENCODING; break;
  }
  P.out_len = P.status == TSG_OK ? uint32_t(sz) : 0;
}

// a page's payload (behind the 6-byte page header the size pass checked) and where it decodes to
struct PageIO { const uint8_t *b; uint32_t n; uint8_t *out; };
__device__ __forceinline__ PageIO page_io(const FindPage &P, uint8_t *arena) {
  return PageIO{P.src + 6, P.len - 6, arena + P.out_off};
}

struct CrcArgs {
  uint32_t table[256];  // CRC-32C (Castagnoli), reflected
  uint32_t z1024[32];   // the register after 1024 zero bytes from state 1 << b
};

// (3) one wave per page
constexpr int kFindThreads = 64;
// one staged snappy block cbuf[t .. bl) -> obuf[0 .. ulen), the tags parsed in lockstep (every
// value that steers control is wave-uniform); decode_other.go:41-102
__device__ int32_t snap_block_wave(const uint8_t *cbuf, uint32_t t, uint32_t bl, uint8_t *obuf, uint32_t ulen,
                                   int lane) {
  int32_t status = TSG_OK;
  uint32_t d = 0;
  while (t < bl) {
    const uint32_t tag = cbuf[t];
    uint32_t len, off = 0;
    if ((tag & 3) == 0) {  // literal
      uint32_t x = tag >> 2;
      if (x < 60) {
        t += 1;
      } else {
        const uint32_t nb = x - 59;
        if (t + 1 + nb > bl) { status = TSG_E_CORRUPT; break; }
        x = 0;
        for (uint32_t q = 0; q < nb; q++) x |= uint32_t(cbuf[t + 1 + q]) << (8 * q);
        t += 1 + nb;
      }
      len = x + 1;
      if (len == 0 || len > bl - t || len > ulen - d) { status = TSG_E_CORRUPT; break; }
      for (uint32_t j = lane; j < len; j += kFindThreads) obuf[d + j] = cbuf[t + j];
      t += len;
      d += len;
      continue;
    }
    if ((tag & 3) == 1) {
      if (t + 2 > bl) { status = TSG_E_CORRUPT; break; }
      len = 4 + ((tag >> 2) & 7);
      off = ((tag & 0xe0) << 3) | cbuf[t + 1];
      t += 2;
    } else if ((tag & 3) == 2) {
      if (t + 3 > bl) { status = TSG_E_CORRUPT; break; }
      len = 1 + (tag >> 2);
      off = uint32_t(cbuf[t + 1]) | uint32_t(cbuf[t + 2]) << 8;
      t += 3;
    } else {
      if (t + 5 > bl) { status = TSG_E_CORRUPT; break; }
      len = 1 + (tag >> 2);
      off = uint32_t(cbuf[t + 1]) | uint32_t(cbuf[t + 2]) << 8 | uint32_t(cbuf[t + 3]) << 16 |
            uint32_t(cbuf[t + 4]) << 24;
      t += 5;
    }
    if (off == 0 || off > d || len > ulen - d) { status = TSG_E_CORRUPT; break; }
    // LZ77 copy: out[d + j] = out[d - off + j % off] (periodic when off < len)
    if (off >= len) {
      for (uint32_t j = lane; j < len; j += kFindThreads) obuf[d + j] = obuf[d - off + j];
    } else {
      for (uint32_t j = lane; j < len; j += kFindThreads) obuf[d + j] = obuf[d - off + j % off];
    }
    d += len;
  }
  if (status == TSG_OK && d != ulen) status = TSG_E_CORRUPT;
  return status;
}

// CRC-32C of obuf[0 .. ulen), ulen <= 64 KiB, on every lane: 1 KiB per lane, combined on lane 0
__device__ uint32_t wave_crc32c(const uint8_t *obuf, uint32_t ulen, const uint32_t *tab, uint32_t *lane_crc,
                                const CrcArgs *crc, int lane) {
  uint32_t r = 0;  // raw register from state 0
  const uint32_t lo = uint32_t(lane) * 1024, hi = min(ulen, lo + 1024);
  for (uint32_t i = lo; i < hi; i++) r = tab[(r ^ obuf[i]) & 0xff] ^ (r >> 8);
  lane_crc[lane] = r;
  __syncthreads();
  if (lane == 0) {
    uint32_t acc = 0xffffffffu;
    const uint32_t nseg = (ulen + 1023) / 1024;
    for (uint32_t g = 0; g < nseg; g++) {
      const uint32_t sl = min(ulen - g * 1024, 1024u);
      uint32_t z = 0;
      if (sl == 1024) {  // advance by 1024 zero bytes: linear map, precomputed columns
        for (int bb = 0; bb < 32; bb++)
          if ((acc >> bb) & 1u) z ^= crc->z1024[bb];
      } else {
        z = acc;
        for (uint32_t i = 0; i < sl; i++) z = tab[z & 0xff] ^ (z >> 8);
      }
      acc = z ^ lane_crc[g];
    }
    lane_crc[0] = ~acc;
  }
  __syncthreads();
  const uint32_t c = lane_crc[0];
  __syncthreads();
  return c;
}

extern "C" __global__ void __launch_bounds__(kFindThreads) find_decode_kernel(FindPage *pages, uint8_t *arena,
                                                                            const CrcArgs *crc) {
  __shared__ uint8_t cbuf[snapdev::kMaxChunk + 8];
  __shared__ uint8_t obuf[snapdev::kMaxBlock + 8];
  __shared__ uint32_t tab[256];
  __shared__ uint32_t lane_crc[kFindThreads];
  const int lane = threadIdx.x;
  FindPage &P = pages[blockIdx.x];
  const PageCodec codec = P.codec();
  if (P.status != TSG_OK || (codec != PageCodec::None && codec != PageCodec::Snappy)) return;  // (zstd, lz4: their own kernels)
  for (int i = lane; i < 256; i += kFindThreads) tab[i] = crc->table[i];
  const auto [b, n, out] = page_io(P, arena);
  if (codec == PageCodec::None) {
    for (uint32_t i = lane; i < n; i += kFindThreads) out[i] = b[i];
    return;
  }
  __syncthreads();
  snapdev::ChunkWalk w;  // (the size pass accepted the framing already)
  uint32_t pos = 0;
  int32_t status = TSG_OK;
  while (status == TSG_OK) {
    const int r = w.next(b, n);
    if (r <= 0) {
      if (r < 0) status = TSG_E_CORRUPT;
      break;
    }
    const uint32_t ulen = w.ulen;
    if (w.type == 0x01) {  // uncompressed chunk: copy into obuf for the checksum
      for (uint32_t i = lane; i < ulen; i += kFindThreads) obuf[i] = b[w.data + i];
    } else {
      // stage the compressed block, then decode it in lockstep
      for (uint32_t i = lane; i < w.size; i += kFindThreads) cbuf[i] = b[w.data + i];
      __syncthreads();
      status = snap_block_wave(cbuf, w.block - w.data, w.size, obuf, ulen, lane);
    }
    __syncthreads();
    if (status != TSG_OK) break;
    if (snapdev::crc_mask(wave_crc32c(obuf, ulen, tab, lane_crc, crc, lane)) != w.crc) status = TSG_E_CORRUPT;
    if (status != TSG_OK || pos + ulen > P.out_len) { status = TSG_E_CORRUPT; break; }
    for (uint32_t i = lane; i < ulen; i += kFindThreads) out[pos + i] = obuf[i];
    pos += ulen;
    __syncthreads();
  }
  if (lane == 0 && (status != TSG_OK || pos != P.out_len)) P.status = status != TSG_OK ? status : TSG_E_CORRUPT;
}

// (3') zstd pages: one lane decodes the page (tables and literals in LDS)
extern "C" __global__ void __launch_bounds__(64) find_decode_zstd_kernel(FindPage *pages, uint8_t *arena) {
  __shared__ zdev::Work W;
  FindPage &P = pages[blockIdx.x];
  if (P.status != TSG_OK || P.codec() != PageCodec::Zstd || threadIdx.x != 0) return;
  uint64_t len = 0;
  const auto [b, n, out] = page_io(P, arena);
  const int st = zdev::zstd_decode(b, n, out, P.out_len, len, W);
  if (st != TSG_OK) P.status = st;
  else P.out_len = uint32_t(len);  // (the size pass may hold an upper bound)
}

// (3'z) zstd pages, the default: one wave per page (zstd_dev.hpp, the wave decoder). Lane 0 parses
// the headers and table descriptions and decodes the FSE sequence stream in batches of 256
// triples into LDS; 4 lanes decode the 4 Huffman streams; all 64 lanes execute the batches, 64
// bytes a step. A match's source is the arena itself, since a match may reach back anywhere in
// the page: a lane loads a byte another lane stored only after the wave has waited for its
// stores (s_waitcnt vmcnt(0)) since that byte was written, with plain loads (zstd_dev.hpp
// keeps `settled`, the position below which every byte has reached memory, and waits only
// before a step that reads at or above it). LDS: zdev::Work (the block's literals and the
// tables) + zdev::WaveWork (a batch); DESIGN.md §7 has the figures.
extern "C" __global__ void __launch_bounds__(kFindThreads) find_decode_zstd_wave_kernel(FindPage *pages, uint8_t *arena) {
  __shared__ zdev::Work W;
  __shared__ zdev::WaveWork X;
  FindPage &P = pages[blockIdx.x];
  if (P.status != TSG_OK || P.codec() != PageCodec::Zstd) return;
  uint64_t len = 0;
  const auto [b, n, out] = page_io(P, arena);
  const int st = zdev::zstd_decode_wave(b, n, out, P.out_len, len, W, X, threadIdx.x);
  if (threadIdx.x != 0) return;
  if (st != TSG_OK) P.status = st;
  else P.out_len = uint32_t(len);  // (the size pass may hold an upper bound)
}

// (3'') lz4 pages: one wave per page, the frame's blocks one after the other. A block's
// sequences are parsed once for the wave from compressed bytes staged in LDS in slices of
// kLzIn; literals and matches are copied by all 64 lanes into a ring of the last 64 KiB of
// output (the format's window: a match reaches back 65 535 bytes at most), which is written
// to the arena every 32 KiB. A match is copied 64 bytes a step: with offset o >= 64 byte j is
// out[d + j - o], written by an earlier step; with o < 64 the 64 bytes of a step repeat the o
// bytes before it (byte j = out[d - o + j % o], the snappy decoder's form, re-based at every
// step). Each step reads, meets the wave, writes and meets again, so a lane never reads a
// byte another lane has yet to write or has already overwritten (the ring position of
// d + j is that of d + j - 65536, which the step's own reads may still name when o > 65472).
// Lanes hand bytes to each other through LDS only. The arena is read back only for the
// optional xxh32 checksums (frames of the reference Writer carry none), by the workgroup that
// stored those bytes and after a __syncthreads(): its workgroup-scope release / acquire waits
// for the stores, and one workgroup's waves share the CU's L1, so the loads see them.
// Linked blocks (never written by the reference): TSG_E_UNSUPPORTED for the page's hits.
constexpr uint32_t kLzRing = 65536, kLzMask = kLzRing - 1, kLzIn = 16384, kLzChunk = 16384, kLzFlush = 32768;

// xxh32 of p[0 .. n): lanes 0..3 run the four accumulators over the stripes
__device__ uint32_t lz_wave_xxh32(const uint8_t *p, uint64_t n, int lane) {
  uint32_t v = lane == 0 ? lz4dev::kP1 + lz4dev::kP2 : lane == 1 ? lz4dev::kP2 : lane == 2 ? 0u : 0u - lz4dev::kP1;
  const uint64_t ns = n / 16;
  if (lane < 4)
    for (uint64_t i = 0; i < ns; i++) v = lz4dev::xxh_round(v, rd32(p + 16 * i + 4 * lane));
  const uint32_t v0 = __shfl(v, 0, 64), v1 = __shfl(v, 1, 64), v2 = __shfl(v, 2, 64), v3 = __shfl(v, 3, 64);
  return lz4dev::xxh_finish(n >= 16 ? lz4dev::xxh_merge(v0, v1, v2, v3) : lz4dev::kP5, p + 16 * ns, n);
}

// one compressed block src[0 .. n) -> dst[0 .. cap); every value that steers control is wave-uniform
__device__ int32_t lz_block_wave(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap, uint32_t &len,
                                 uint8_t *ring, uint8_t *ibuf, int lane) {
  len = 0;
  if (n == 0) return TSG_OK;
  uint32_t ib0 = 0, ibn = 0;  // ibuf holds src[ib0 .. ib0 + ibn)
  auto byte = [&](uint32_t t) -> uint32_t {  // t < n, never behind ib0
    if (t >= ib0 + ibn) {
      __syncthreads();
      ib0 = t;
      ibn = min(n - t, kLzIn);
      for (uint32_t i = lane; i < ibn; i += kFindThreads) ibuf[i] = src[t + i];
      __syncthreads();
    }
    return uint32_t(__builtin_amdgcn_readfirstlane(int(ibuf[t - ib0])));
  };
  uint32_t s = 0, d = 0, flushed = 0;
  auto flush = [&](uint32_t upto) {  // (the ring's bytes are complete: callers have met the wave)
    for (uint32_t i = flushed + lane; i < upto; i += kFindThreads) dst[i] = ring[i & kLzMask];
    flushed = upto;
    __syncthreads();
  };
  for (;;) {
    if (s >= n) return TSG_E_CORRUPT;
    const uint32_t tok = byte(s++);
    uint32_t ll = tok >> 4;  // (n <= 4 MiB: a length stays below 2^31)
    if (ll == 15) {
      uint32_t x;
      do {
        if (s >= n) return TSG_E_CORRUPT;
        x = byte(s++);
        ll += x;
      } while (x == 255);
    }
    if (ll > n - s || ll > cap - d) return TSG_E_CORRUPT;
    while (ll) {
      const uint32_t c = min(ll, kLzChunk);
      if (s >= ib0 && s + c <= ib0 + ibn) {
        for (uint32_t j = lane; j < c; j += kFindThreads) ring[(d + j) & kLzMask] = ibuf[s - ib0 + j];
      } else {  // (past the staged slice: straight from the page)
        for (uint32_t j = lane; j < c; j += kFindThreads) ring[(d + j) & kLzMask] = src[s + j];
      }
      s += c;
      d += c;
      ll -= c;
      __syncthreads();
      if (d - flushed >= kLzFlush) flush(d);
    }
    if (s == n) break;  // a block ends with literals
    if (n - s < 2) return TSG_E_CORRUPT;
    uint32_t off = byte(s);  // (two statements: byte() may restage the slice, in input order only)
    off |= byte(s + 1) << 8;
    s += 2;
    if (off == 0 || off > d) return TSG_E_CORRUPT;
    uint32_t ml = 4 + (tok & 15);
    if ((tok & 15) == 15) {
      uint32_t x;
      do {
        if (s >= n) return TSG_E_CORRUPT;
        x = byte(s++);
        ml += x;
      } while (x == 255);
    }
    if (ml > cap - d) return TSG_E_CORRUPT;
    // lane L of a step copies from `back` bytes behind its byte: o, or with o < 64 the byte
    // L % o of the o bytes before the step
    const uint32_t back = off >= uint32_t(kFindThreads) ? off : off + uint32_t(lane) - uint32_t(lane) % off;
    while (ml) {
      const uint32_t c = min(ml, kLzChunk);
      for (uint32_t j0 = 0; j0 < c; j0 += kFindThreads) {
        const uint32_t j = j0 + lane;
        uint8_t v = 0;
        if (j < c) v = ring[(d + j - back) & kLzMask];
        __syncthreads();
        if (j < c) ring[(d + j) & kLzMask] = v;
        __syncthreads();
      }
      d += c;
      ml -= c;
      if (d - flushed >= kLzFlush) flush(d);
    }
  }
  flush(d);
  len = d;
  return TSG_OK;
}

extern "C" __global__ void __launch_bounds__(kFindThreads) find_decode_lz4_kernel(FindPage *pages, uint8_t *arena) {
  __shared__ uint8_t ring[kLzRing];
  __shared__ uint8_t ibuf[kLzIn];
  const int lane = threadIdx.x;
  FindPage &P = pages[blockIdx.x];
  if (P.status != TSG_OK || P.codec() != PageCodec::Lz4) return;
  const auto [b, n, out] = page_io(P, arena);
  lz4dev::Frame f;
  int32_t status = lz4dev::lz4_header(b, n, f);  // (accepted by the size pass already)
  if (status == TSG_OK && !(f.flags & lz4dev::kFlagIndep)) status = TSG_E_UNSUPPORTED;
  lz4dev::BlockWalk w;
  w.s = f.pos;
  uint32_t pos = 0;
  while (status == TSG_OK) {
    const int r = w.next(b, n, f);
    if (r <= 0) {
      if (r < 0) status = TSG_E_CORRUPT;
      break;
    }
    uint32_t ulen = w.size;
    if (w.stored) {
      if (ulen > P.out_len - pos) {
        status = TSG_E_CORRUPT;
        break;
      }
      for (uint32_t i = lane; i < ulen; i += kFindThreads) out[pos + i] = b[w.data + i];
    } else {
      status = lz_block_wave(b + w.data, w.size, out + pos, min(f.bmax, P.out_len - pos), ulen, ring, ibuf, lane);
      if (status != TSG_OK) break;
    }
    if (f.flags & lz4dev::kFlagBlockSum) {  // over the decoded bytes (reference) or the stored ones (format)
      __syncthreads();
      if (lz_wave_xxh32(out + pos, ulen, lane) != w.sum && lz_wave_xxh32(b + w.data, w.size, lane) != w.sum) {
        status = TSG_E_CORRUPT;
        break;
      }
    }
    pos += ulen;
  }
  if (status == TSG_OK && (f.flags & lz4dev::kFlagContentSum)) {
    __syncthreads();
    if (n - w.s < 4 || rd32(b + w.s) != lz_wave_xxh32(out, pos, lane)) status = TSG_E_CORRUPT;
  }
  if (status == TSG_OK && pos != P.out_len) status = TSG_E_CORRUPT;
  if (lane == 0 && status != TSG_OK) P.status = status;
}

// (4) the page's objects against its pending ids (hit_ids[hit0 .. hit0 + nhit), 16 bytes
// each): per hit the object's offset (into the arena) and length, or not found. The
// objects are read as findOne's iterator reads them (object.UnmarshalObjectFromReader
// over a bytes.Reader, object.go:49-80): the page ends cleanly where a header would start
// at its end (or with 4 or 8 bytes left: the next read hits EOF), a short read or an id
// length past the object is an error for every id not found before it.
struct FindHitOut {
  uint64_t off;
  uint32_t len;
  int32_t status;  // TSG_OK found, TSG_E_NOT_FOUND none (findOne returns nil), else the page error
};
constexpr int kFindPer = 4;  // pending ids held in registers per lane and pass
extern "C" __global__ void __launch_bounds__(kFindThreads) find_scan_kernel(const FindPage *pages, const uint8_t *arena,
                                                                          const uint8_t *hit_ids, FindHitOut *res) {
  __shared__ uint8_t win[kFindWindow + 16];
  const int lane = threadIdx.x;
  const FindPage &P = pages[blockIdx.x];
  const int32_t init = P.status == TSG_OK ? TSG_E_NOT_FOUND : P.status;
  for (uint32_t h = lane; h < P.nhit; h += kFindThreads) res[P.hit0 + h] = FindHitOut{0, 0, init};
  if (P.status != TSG_OK) return;
  const uint8_t *pg = arena + P.out_off;
  const uint32_t L = P.out_len;
  for (uint32_t base = 0; base < P.nhit; base += kFindPer * kFindThreads) {
    uint32_t id[kFindPer][4];
    bool pend[kFindPer];
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kFindPer; k++) {
      const uint32_t h = base + uint32_t(k) * kFindThreads + lane;
      pend[k] = h < P.nhit;
#pragma unroll
      for (int q = 0; q < 4; q++) id[k][q] = pend[k] ? rd32(hit_ids + uint64_t(P.hit0 + h) * 16 + 4 * q) : 0u;
      mine += pend[k] ? 1u : 0u;
    }
    uint32_t remaining = mine;
    for (int dd = 32; dd > 0; dd >>= 1) remaining += __shfl_xor(remaining, dd, 64);
    int32_t err = TSG_OK;
    uint32_t p = 0;  // window start (page offset): always an object start
    while (remaining && err == TSG_OK) {
      const uint32_t wl = min(L - p, kFindWindow);
      __syncthreads();
      for (uint32_t i = lane; i < wl; i += kFindThreads) win[i] = pg[p + i];
      __syncthreads();
      uint32_t w = 0;
      bool end = false;
      for (;;) {
        const uint32_t R = L - (p + w);  // bytes left in the page
        if (R == 0 || R == 4) {          // io.EOF at a header read
          end = true;
          break;
        }
        if (R < 8) {  // io.ErrUnexpectedEOF
          err = TSG_E_CORRUPT;
          break;
        }
        if (wl - w < 8) break;  // (the window ends before the page does) slide
        const uint32_t total = rd32(win + w), il = rd32(win + w + 4);
        if (R == 8) {  // reading the object bytes at EOF: io.EOF
          end = true;
          break;
        }
        if (total < 8 || total - 8 > R - 8 || il > total - 8) {  // short read / id past the object
          err = TSG_E_CORRUPT;
          break;
        }
        if (il == 16) {
          if (wl - w < 24) break;  // slide
          uint32_t oid[4];
#pragma unroll
          for (int q = 0; q < 4; q++) oid[q] = rd32(win + w + 8 + 4 * q);
          bool got = false;
#pragma unroll
          for (int k = 0; k < kFindPer; k++)
            if (pend[k] && id[k][0] == oid[0] && id[k][1] == oid[1] && id[k][2] == oid[2] && id[k][3] == oid[3]) {
              const uint32_t h = base + uint32_t(k) * kFindThreads + lane;
              res[P.hit0 + h] = FindHitOut{P.out_off + p + w + 24, total - 24, TSG_OK};
              pend[k] = false;
              mine--;
              got = true;
            }
          if (__ballot(got)) {
            remaining = mine;
            for (int dd = 32; dd > 0; dd >>= 1) remaining += __shfl_xor(remaining, dd, 64);
            if (!remaining) break;
          }
        }
        const uint64_t next = uint64_t(w) + total;  // (<= L - p: total <= R)
        w = uint32_t(next);
        if (next >= wl) break;  // next object beyond this window
      }
      if (end || err != TSG_OK) break;
      p += w;
    }
    if (err != TSG_OK)  // findOne returns the error for every id it had not found yet
#pragma unroll
      for (int k = 0; k < kFindPer; k++)
        if (pend[k]) res[P.hit0 + base + uint32_t(k) * kFindThreads + lane].status = err;
  }
}

// (5) found objects into one arena
extern "C" __global__ void __launch_bounds__(256) find_gather_kernel(const FindHitOut *res, const uint64_t *dst_off,
                                                                   uint32_t nhits, const uint8_t *arena,
                                                                   uint8_t *dst) {
  const uint32_t h = blockIdx.x;
  if (h >= nhits || res[h].status != TSG_OK) return;
  const uint8_t *src = arena + res[h].off;
  uint8_t *d = dst + dst_off[h];
  for (uint32_t i = threadIdx.x; i < res[h].len; i += blockDim.x) d[i] = src[i];
}

// ---- host -------------------------------------------------------------------------------
static std::atomic<bool> g_zstd_lane{false};  // test hook (tsg_debug_set "zstd_find_lane"): the one-lane zstd decoder
void find_zstd_lane(bool on) { g_zstd_lane.store(on); }

static void crc_tables(CrcArgs &c) {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t r = i;
    for (int k = 0; k < 8; k++) r = (r >> 1) ^ (0x82f63b78u & (0u - (r & 1u)));
    c.table[i] = r;
  }
  for (int b = 0; b < 32; b++) {
    uint32_t z = 1u << b;
    for (int i = 0; i < 1024; i++) z = c.table[z & 0xff] ^ (z >> 8);
    c.z1024[b] = z;
  }
}

// ---- pages of blocks whose data file stays on disk (TSG_V2_DATA_ON_DEMAND) ---------------------
// A round's pages (find_rounds.hpp) are read with pread into a pinned buffer by at most
// kFindReaders threads, each taking the next page not yet taken. The threads of round k + 1
// run while round k's kernels do.
constexpr unsigned kFindReaders = 8;
struct StagePage {
  int fd;
  uint64_t start, off;  // in the file, in the staging buffer
  uint32_t len;
  uint32_t page;  // index into the batch's pages
  int err;        // 0, the read's errno, or -1: the file ended inside the page
};
struct RoundRead {
  std::vector<StagePage> pages;
  uint8_t *dst = nullptr;
  std::atomic<size_t> next{0};
  std::vector<std::thread> th;
  void work() {
    for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < pages.size();) {
      StagePage &p = pages[i];
      uint32_t got = 0;
      while (got < p.len) {
        const ssize_t r = ::pread(p.fd, dst + p.off + got, p.len - got, off_t(p.start + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          p.err = r < 0 ? errno : -1;
          break;
        }
        got += uint32_t(r);
      }
    }
  }
  void start(uint64_t bytes) {  // a thread per MiB to read, kFindReaders at the most
    const size_t nt = std::min<size_t>({kFindReaders, pages.size(), size_t(bytes >> 20) + 1});
    for (size_t t = 0; t < nt; t++) th.emplace_back([this] { work(); });
  }
  void wait() {
    for (auto &t : th) t.join();
    th.clear();
  }
  ~RoundRead() { wait(); }
};

static uint64_t find_stage_cap() {
  if (const uint64_t v = g_find_stage_bytes.load(std::memory_order_relaxed)) return v;
  static const uint64_t env = [] {
    const char *e = std::getenv("TSG_FIND_STAGE_BYTES");
    return e ? uint64_t(std::strtoull(e, nullptr, 10)) : 0;
  }();
  return env ? env : kFindStageDefault;
}

// One round on the device: steps (2) to (5) over `pages`, whose hit ranges index `hid` (16 bytes
// per hit) and `res`. stage: the round's staged bytes (pinned), copied to dc.fstage first (the
// pages' src already point there). The objects found are appended to `bytes` in hit order; doff
// is where each lies in `bytes`. Returns the device time (ns). dc.mu is held.
static uint64_t find_round(DeviceCtx &dc, std::vector<FindPage> &pages, const std::vector<uint8_t> &hid,
                           const uint8_t *stage, uint64_t stage_bytes, const CrcArgs &crc, std::vector<FindHitOut> &res,
                           std::vector<uint64_t> &doff, std::vector<uint8_t> &bytes) {
  const uint32_t np = uint32_t(pages.size());
  const size_t nh = hid.size() / 16;
  res.assign(nh, FindHitOut{0, 0, TSG_E_NOT_FOUND});
  doff.assign(nh, 0);
  if (np == 0) return 0;
  hipStream_t s = dc.stream;
  HIP_OK(hipEventRecord(dc.ev0, s));
  if (stage_bytes) HIP_OK(hipMemcpyAsync(dc.fstage.p, stage, stage_bytes, hipMemcpyHostToDevice, s));
  // (2) sizes
  DevBuf &dpages = dc.fpages, &dhid = dc.fhits, &dres = dc.fres, &darena = dc.farena;
  dpages.ensure(size_t(np) * sizeof(FindPage));
  HIP_OK(hipMemcpyAsync(dpages.p, pages.data(), size_t(np) * sizeof(FindPage), hipMemcpyHostToDevice, s));
  find_size_kernel<<<(np + 255) / 256, 256, 0, s>>>(static_cast<FindPage *>(dpages.p), np);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(pages.data(), dpages.p, size_t(np) * sizeof(FindPage), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  uint64_t total = 0;
  for (auto &pg : pages) {
    pg.out_off = total;
    total += (pg.out_len + 15) / 16 * 16;
  }
  darena.ensure(std::max<uint64_t>(total, 16));
  HIP_OK(hipMemcpyAsync(dpages.p, pages.data(), size_t(np) * sizeof(FindPage), hipMemcpyHostToDevice, s));
  // (3) decode
  dc.fcrc.ensure(sizeof(CrcArgs));
  HIP_OK(hipMemcpyAsync(dc.fcrc.p, &crc, sizeof(CrcArgs), hipMemcpyHostToDevice, s));
  find_decode_kernel<<<np, kFindThreads, 0, s>>>(static_cast<FindPage *>(dpages.p), static_cast<uint8_t *>(darena.p),
                                               static_cast<const CrcArgs *>(dc.fcrc.p));
  HIP_OK(hipGetLastError());
  auto any = [&](PageCodec c) {  // a page of that codec the size pass accepted
    return std::any_of(pages.begin(), pages.end(), [c](const FindPage &pg) { return pg.status == TSG_OK && pg.codec() == c; });
  };
  if (any(PageCodec::Zstd)) {
    if (g_zstd_lane.load(std::memory_order_relaxed))
      find_decode_zstd_kernel<<<np, 64, 0, s>>>(static_cast<FindPage *>(dpages.p), static_cast<uint8_t *>(darena.p));
    else
      find_decode_zstd_wave_kernel<<<np, kFindThreads, 0, s>>>(static_cast<FindPage *>(dpages.p),
                                                               static_cast<uint8_t *>(darena.p));
    HIP_OK(hipGetLastError());
  }
  if (any(PageCodec::Lz4)) {
    find_decode_lz4_kernel<<<np, kFindThreads, 0, s>>>(static_cast<FindPage *>(dpages.p),
                                                       static_cast<uint8_t *>(darena.p));
    HIP_OK(hipGetLastError());
  }
  // (4) objects
  dhid.ensure(hid.size());
  HIP_OK(hipMemcpyAsync(dhid.p, hid.data(), hid.size(), hipMemcpyHostToDevice, s));
  dres.ensure(nh * sizeof(FindHitOut));
  find_scan_kernel<<<np, kFindThreads, 0, s>>>(static_cast<const FindPage *>(dpages.p),
                                               static_cast<const uint8_t *>(darena.p),
                                               static_cast<const uint8_t *>(dhid.p), static_cast<FindHitOut *>(dres.p));
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(res.data(), dres.p, nh * sizeof(FindHitOut), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  // (5) gather the found objects
  uint64_t obytes = 0;
  for (size_t k = 0; k < nh; k++) {
    doff[k] = obytes;
    if (res[k].status == TSG_OK) obytes += res[k].len;
  }
  const uint64_t base = bytes.size();
  bytes.resize(base + obytes);
  if (obytes) {
    dc.fdst.ensure(obytes);
    dc.foff.ensure(nh * 8);
    HIP_OK(hipMemcpyAsync(dc.foff.p, doff.data(), nh * 8, hipMemcpyHostToDevice, s));
    find_gather_kernel<<<uint32_t(nh), 256, 0, s>>>(static_cast<const FindHitOut *>(dres.p),
                                                    static_cast<const uint64_t *>(dc.foff.p), uint32_t(nh),
                                                    static_cast<const uint8_t *>(darena.p),
                                                    static_cast<uint8_t *>(dc.fdst.p));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(bytes.data() + base, dc.fdst.p, obytes, hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipEventRecord(dc.ev1, s));
  HIP_OK(hipStreamSynchronize(s));
  for (auto &o : doff) o += base;
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, dc.ev0, dc.ev1));
  return uint64_t(double(ms) * 1e6);
}

void device_find(DeviceCtx &dc, const std::vector<std::pair<uint32_t, V2Block *>> &blocks, const uint8_t (*ids)[16],
                 size_t nids, const tsg_lookup_opts *opts, FindOut &out) {
  LookupOut lk;
  device_lookup(dc, blocks, ids, nids, opts, lk);
  out = FindOut();
  const size_t nh = lk.id_idx.size();
  out.id_idx.assign(lk.id_idx.begin(), lk.id_idx.end());
  out.block_idx.assign(lk.block_idx.begin(), lk.block_idx.end());
  out.status.assign(nh, TSG_E_NOT_FOUND);
  out.obj_off.assign(nh, 0);
  out.obj_len.assign(nh, 0);
  out.kernel_ns = lk.kernel_ns;
  if (nh == 0) return;
  std::unordered_map<uint32_t, const V2Block *> by_idx;
  for (auto &bp : blocks) by_idx[bp.first] = bp.second;
  // (1) distinct pages, hits grouped by page
  std::vector<uint32_t> order(nh);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return lk.block_idx[a] != lk.block_idx[b] ? lk.block_idx[a] < lk.block_idx[b] : lk.rec[a] < lk.rec[b];
  });
  std::vector<FindPage> pages;
  std::vector<uint8_t> hid(nh * 16, 0);  // ids in page order
  std::vector<uint32_t> slot(nh);        // page order -> hit
  std::vector<StagePage> od;             // the pages to read from their files, in page order
  std::vector<uint32_t> od_len;
  for (size_t k = 0; k < nh; k++) {
    const uint32_t h = order[k];
    const V2Block *b = by_idx.at(lk.block_idx[h]);
    if (pages.empty() || k == 0 || lk.block_idx[order[k - 1]] != lk.block_idx[h] || lk.rec[order[k - 1]] != lk.rec[h]) {
      FindPage pg{};
      pg.hit0 = uint32_t(k);
      if (!b->d_data && b->data_fd < 0) {
        pg.status = TSG_E_UNSUPPORTED;  // data file neither resident nor held open
      } else if (lk.start[h] + lk.len[h] > b->data_len) {
        pg.status = TSG_E_CORRUPT;  // ReadAt past the end of the data file
      } else {
        pg.len = lk.len[h];
        pg.enc = uint32_t(b->enc);
        pg.status = TSG_OK;
        if (b->d_data) {
          pg.src = b->d_data + lk.start[h];
        } else {  // (src: once its round's staging offset is known)
          od.push_back(StagePage{b->data_fd, lk.start[h], 0, lk.len[h], uint32_t(pages.size()), 0});
          od_len.push_back(lk.len[h]);
        }
      }
      pages.push_back(pg);
    }
    pages.back().nhit++;
    std::memcpy(&hid[k * 16], ids[lk.id_idx[h]], 16);
    slot[k] = h;
  }
  FindRoundPlan plan;
  plan_find_rounds(od_len.data(), od_len.size(), find_stage_cap(), plan);
  for (size_t i = 0; i < od.size(); i++) od[i].off = plan.offsets[i];
  const size_t nr = plan.rounds.size();
  uint64_t stage_max = 0;
  for (auto &r : plan.rounds) stage_max = std::max(stage_max, r.bytes);
  static const CrcArgs crc = [] {
    CrcArgs c;
    crc_tables(c);
    return c;
  }();
  // The pinned buffers and their readers. They have a lock of their own, taken before dc.mu:
  // round 0 is read from the files before the device is taken from its other callers and the
  // resident search launch is told to leave, so a cold file holds up other finds over on-demand
  // blocks of this device only. (Later rounds are read while the call's own kernels run.)
  std::unique_lock<std::mutex> stage_lk(dc.fstage_mu, std::defer_lock);
  RoundRead rd[2];
  auto start_read = [&](size_t r) {
    RoundRead &R = rd[r & 1];
    const FindRound &fr = plan.rounds[r];
    R.pages.assign(od.begin() + fr.first, od.begin() + fr.first + fr.count);
    R.dst = static_cast<uint8_t *>(dc.fstage_host[r & 1].p);
    R.next.store(0);
    R.start(fr.bytes);
  };
  if (!od.empty()) {
    stage_lk.lock();
    HIP_OK(hipSetDevice(dc.ordinal));
    // sized once for the call's largest round (+ 64: a decoder's wide load past a page's last
    // byte stays inside)
    for (size_t i = 0; i < std::min<size_t>(nr, 2); i++) dc.fstage_host[i].ensure(stage_max + 64);
    start_read(0);
    rd[0].wait();
  }
  std::lock_guard<std::mutex> lkd(dc.mu);
  resident_quit(dc);  // (the resident search launch holds every CU's LDS)
  HIP_OK(hipSetDevice(dc.ordinal));
  std::vector<FindHitOut> res(nh);  // per hit in page order
  std::vector<uint64_t> doff(nh, 0);
  if (od.empty()) {  // every page resident: one round over the batch as it stands
    out.kernel_ns += find_round(dc, pages, hid, nullptr, 0, crc, res, doff, out.bytes);
    dc.find_rounds++;
  } else {
    dc.fstage.ensure(stage_max + 64);
    std::vector<uint8_t> is_od(pages.size(), 0);
    for (auto &p : od) is_od[p.page] = 1;
    // round r: its on-demand pages, and in round 0 every other page too, in page order. Every
    // round's objects are gathered straight behind the earlier rounds' in out.bytes.
    std::vector<uint32_t> hits;  // the rounds' hits one after the other: page-order hit of each
    std::vector<FindHitOut> rres;
    std::vector<uint64_t> rdoff;
    std::vector<std::pair<FindHitOut, uint64_t>> got(nh);  // per page-order hit: its result, where its object lies
    for (size_t r = 0; r < nr; r++) {
      const FindRound &fr = plan.rounds[r];
      std::vector<uint32_t> take;  // page indexes
      if (r == 0) {
        const uint32_t end = fr.first + fr.count < od.size() ? od[fr.first + fr.count].page : uint32_t(pages.size());
        for (uint32_t p = 0; p < pages.size(); p++)
          if (!is_od[p] || p < end) take.push_back(p);
      } else {
        for (uint32_t i = fr.first; i < fr.first + fr.count; i++) take.push_back(od[i].page);
      }
      RoundRead &R = rd[r & 1];
      R.wait();
      if (r + 1 < nr) start_read(r + 1);  // (its buffer: round r - 1's copy has completed)
      for (const StagePage &p : R.pages) {
        FindPage &pg = pages[p.page];
        pg.src = static_cast<const uint8_t *>(dc.fstage.p) + p.off;
        if (!p.err) dc.find_read_bytes += p.len;
        if (p.err) {
          pg.status = TSG_E_CORRUPT;
          out.read_error = "data file: page at " + std::to_string(p.start) + " (" + std::to_string(p.len) +
                           " bytes): " + (p.err > 0 ? std::strerror(p.err) : "the file ends inside the page");
        }
      }
      std::vector<FindPage> rp;
      std::vector<uint8_t> rhid;
      const size_t h0 = hits.size();
      for (uint32_t p : take) {
        FindPage pg = pages[p];
        for (uint32_t j = 0; j < pg.nhit; j++) hits.push_back(pg.hit0 + j);
        rhid.insert(rhid.end(), hid.begin() + size_t(pg.hit0) * 16, hid.begin() + size_t(pg.hit0 + pg.nhit) * 16);
        pg.hit0 = uint32_t(hits.size() - h0) - pg.nhit;
        rp.push_back(pg);
      }
      out.kernel_ns += find_round(dc, rp, rhid, R.dst, fr.bytes, crc, rres, rdoff, out.bytes);
      dc.find_rounds++;
      for (size_t j = 0; j < rres.size(); j++) got[hits[h0 + j]] = {rres[j], rdoff[j]};
    }
    // Page order, as one round would have left the objects. The rounds' hits follow each other in
    // page order already unless resident pages, which ride in round 0, lie behind staged pages of
    // a later round: only then the objects are moved.
    bool sorted = true;
    for (size_t k = 0; k < nh && sorted; k++) sorted = hits[k] == k;
    std::vector<uint8_t> moved;
    if (!sorted) moved.resize(out.bytes.size());
    uint64_t obytes = 0;
    for (size_t k = 0; k < nh; k++) {
      res[k] = got[k].first;
      doff[k] = sorted ? got[k].second : obytes;
      if (res[k].status != TSG_OK) continue;
      if (!sorted && res[k].len) std::memcpy(&moved[obytes], &out.bytes[got[k].second], res[k].len);
      obytes += res[k].len;
    }
    if (!sorted) out.bytes.swap(moved);
  }
  for (size_t k = 0; k < nh; k++) {
    const uint32_t h = slot[k];
    out.status[h] = res[k].status;
    out.obj_off[h] = doff[k];
    out.obj_len[h] = res[k].status == TSG_OK ? res[k].len : 0;
  }
}

}  // namespace tsg
