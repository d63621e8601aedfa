// lz4_dev.hpp — LZ4 frame parsing and block decoding for v2 pages written at the lz4
// encodings (backend.Encoding 2..5: lz4-64k / lz4-256k / lz4-1M / lz4), compiled for the
// host (common.cpp, tools/lz4_host_check.cpp) and for the device (find.hip).
//
//   reader          vendor/github.com/pierrec/lz4/v4/reader.go:81-196
//   frame header    internal/lz4stream/frame.go:80-131,169-200
//   block framing   internal/lz4stream/block.go:279-340
//   block format    internal/lz4block/decode_other.go
//
// What the reference Reader does, and so what is done here: leading skippable frames are
// skipped; the descriptor is FLG, BD and the content size when flagged (version, reserved
// bits and the dictionary-id flag are not looked at), closed by the header checksum
// (xxh32(descriptor) >> 8); the block maximum comes from BD; a block larger than the maximum
// (stored or compressed, or decoding to more) is an error; linked blocks see the previous
// output of the frame; exactly one frame is read and whatever follows it is ignored.
// Checksums: the content checksum is xxh32 of the decoded frame. For the block checksum the
// reference (v4.1.12) hashes the block's decoded bytes where the LZ4 frame format hashes the
// block's bytes as stored; both are accepted (liblz4 writes the second form).
// A content size in the header is checked against what was decoded.
// Legacy frames (magic 0x184C2102) are answered with TSG_E_UNSUPPORTED.
//
// Every length comes from untrusted bytes: each read is checked against the input's end
// and each write against the output's capacity before it is made.
#pragma once
#ifndef TSG_LZ4_HOST
#include <hip/hip_runtime.h>
#endif
#include <cstdint>

namespace tsg {
namespace lz4dev {

constexpr uint32_t kMagic = 0x184D2204u, kMagicSkip = 0x184D2A50u, kMagicLegacy = 0x184C2102u;
constexpr uint32_t kFlagContentSum = 1u << 2, kFlagSize = 1u << 3, kFlagBlockSum = 1u << 4, kFlagIndep = 1u << 5;
constexpr uint32_t kMaxOffset = 65535;

__device__ __forceinline__ uint32_t rd32(const uint8_t *p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// ---- xxh32 (xxHash specification, 32-bit variant) ---------------------------------------
constexpr uint32_t kP1 = 2654435761u, kP2 = 2246822519u, kP3 = 3266489917u, kP4 = 668265263u, kP5 = 374761393u;
__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t xxh_round(uint32_t acc, uint32_t lane) { return rotl(acc + lane * kP2, 13) * kP1; }
// the accumulators v[0..3] after the n / 16 whole stripes are merged by the caller (n >= 16)
__device__ __forceinline__ uint32_t xxh_merge(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
  return rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
}
// h: merged accumulators (or seed + kP5 when n < 16); tail: the n % 16 bytes after the stripes
__device__ __forceinline__ uint32_t xxh_finish(uint32_t h, const uint8_t *tail, uint64_t n) {
  h += uint32_t(n);
  uint32_t r = uint32_t(n & 15);
  for (; r >= 4; r -= 4, tail += 4) h = rotl(h + rd32(tail) * kP3, 17) * kP4;
  for (; r > 0; r--, tail++) h = rotl(h + uint32_t(*tail) * kP5, 11) * kP1;
  h ^= h >> 15;
  h *= kP2;
  h ^= h >> 13;
  h *= kP3;
  h ^= h >> 16;
  return h;
}
// streaming state, so a frame's content checksum can be fed block by block (whole stripes
// are consumed from a 16-byte carry)
struct Xxh32 {
  uint32_t v[4];
  uint8_t buf[16];
  uint32_t fill;
  uint64_t total;
  __device__ void init() {
    v[0] = kP1 + kP2;
    v[1] = kP2;
    v[2] = 0;
    v[3] = 0u - kP1;
    fill = 0;
    total = 0;
  }
  __device__ void stripe(const uint8_t *p) {
    for (int q = 0; q < 4; q++) v[q] = xxh_round(v[q], rd32(p + 4 * q));
  }
  __device__ void update(const uint8_t *p, uint64_t n) {
    total += n;
    if (fill) {
      while (n && fill < 16) {
        buf[fill++] = *p++;
        n--;
      }
      if (fill < 16) return;
      stripe(buf);
      fill = 0;
    }
    for (; n >= 16; n -= 16, p += 16) stripe(p);
    while (n) {
      buf[fill++] = *p++;
      n--;
    }
  }
  __device__ uint32_t digest() const {
    const uint32_t h = total >= 16 ? xxh_merge(v[0], v[1], v[2], v[3]) : kP5;  // seed 0
    return xxh_finish(h, buf, total);
  }
};
__device__ inline uint32_t xxh32(const uint8_t *p, uint64_t n) {
  Xxh32 s;
  s.init();
  s.update(p, n);
  return s.digest();
}

// ---- frame header ------------------------------------------------------------------------
struct Frame {
  uint32_t flags;  // FLG
  uint32_t bmax;   // block maximum (BD)
  uint64_t csize;  // content size (kFlagSize)
  uint32_t pos;    // offset of the first block's size word
};
__device__ inline int lz4_header(const uint8_t *p, uint32_t n, Frame &f) {
  uint32_t s = 0;
  for (;;) {
    if (n - s < 4) return TSG_E_CORRUPT;
    const uint32_t m = rd32(p + s);
    s += 4;
    if (m == kMagic) break;
    if (m == kMagicLegacy) return TSG_E_UNSUPPORTED;
    if ((m >> 8) != (kMagicSkip >> 8)) return TSG_E_CORRUPT;  // (frame.go:94 compares the top 24 bits)
    if (n - s < 4) return TSG_E_CORRUPT;
    const uint32_t skip = rd32(p + s);
    s += 4;
    if (skip > n - s) return TSG_E_CORRUPT;
    s += skip;
  }
  if (n - s < 3) return TSG_E_CORRUPT;
  f.flags = p[s];
  const uint32_t bd = p[s + 1];
  uint32_t dl = 2;
  f.csize = 0;
  if (f.flags & kFlagSize) {
    if (n - s < 11) return TSG_E_CORRUPT;
    f.csize = uint64_t(rd32(p + s + 2)) | uint64_t(rd32(p + s + 6)) << 32;
    dl = 10;
  }
  if (p[s + dl] != uint8_t(xxh32(p + s, dl) >> 8)) return TSG_E_CORRUPT;
  const uint32_t idx = (bd >> 4) & 7;
  if (idx < 4) return TSG_E_CORRUPT;
  f.bmax = 1u << (8 + 2 * idx);  // 64 KiB, 256 KiB, 1 MiB, 4 MiB
  f.pos = s + dl + 1;
  return TSG_OK;
}

// ---- blocks ------------------------------------------------------------------------------
// One block's sequences. kCopy = false only measures. The output is dst[0 .. cap); the block
// starts at dst[base] and a match may reach back to dst[0] (base > 0 with linked blocks:
// the frame's earlier output is the dictionary). len: the block's decoded length.
template <bool kCopy>
__device__ inline int lz4_block(const uint8_t *src, uint32_t n, uint8_t *dst, uint64_t base, uint64_t cap,
                                uint32_t &len) {
  len = 0;
  if (n == 0) return TSG_OK;  // (UncompressBlock: empty source, nothing decoded)
  uint64_t d = base;
  uint32_t s = 0;
  for (;;) {
    if (s >= n) return TSG_E_CORRUPT;
    const uint32_t tok = src[s++];
    uint64_t ll = tok >> 4;
    if (ll == 15) {
      uint32_t x;
      do {
        if (s >= n) return TSG_E_CORRUPT;
        x = src[s++];
        ll += x;
      } while (x == 255);
    }
    if (ll > n - s || ll > cap - d) return TSG_E_CORRUPT;
    if (kCopy)
      for (uint64_t j = 0; j < ll; j++) dst[d + j] = src[s + j];
    s += uint32_t(ll);
    d += ll;
    if (s == n) break;  // a block ends with literals
    if (n - s < 2) return TSG_E_CORRUPT;
    const uint32_t off = uint32_t(src[s]) | uint32_t(src[s + 1]) << 8;
    s += 2;
    if (off == 0 || off > d) return TSG_E_CORRUPT;
    uint64_t ml = 4 + (tok & 15);
    if ((tok & 15) == 15) {
      uint32_t x;
      do {
        if (s >= n) return TSG_E_CORRUPT;
        x = src[s++];
        ml += x;
      } while (x == 255);
    }
    if (ml > cap - d) return TSG_E_CORRUPT;
    if (kCopy)
      for (uint64_t j = 0; j < ml; j++) dst[d + j] = dst[d + j - off];
    d += ml;
  }
  len = uint32_t(d - base);
  return TSG_OK;
}

// The walk over a frame's blocks: next() gives one block header at a time.
struct BlockWalk {
  uint32_t s;       // offset of the next block's size word
  uint32_t data;    // this block's bytes
  uint32_t size;    // and their count
  bool stored;
  uint32_t sum;     // block checksum (kFlagBlockSum)
  // 1: a block, 0: end mark (s is past it), -1: framing error
  __device__ int next(const uint8_t *p, uint32_t n, const Frame &f) {
    if (n - s < 4) return -1;
    const uint32_t x = rd32(p + s);
    s += 4;
    if (x == 0) return 0;
    stored = (x >> 31) != 0;
    size = x & 0x7fffffffu;
    if (size > f.bmax || size > n - s) return -1;
    data = s;
    s += size;
    sum = 0;
    if (f.flags & kFlagBlockSum) {
      if (n - s < 4) return -1;
      sum = rd32(p + s);
      s += 4;
    }
    return 1;
  }
};

// The exact decoded length of the frame at p: the header's content size when it has one
// (verified by the decode), else the sum over the blocks (tokens walked, nothing copied).
__device__ inline int lz4_size(const uint8_t *p, uint32_t n, uint64_t &size) {
  Frame f;
  size = 0;
  int st = lz4_header(p, n, f);
  if (st != TSG_OK) return st;
  if (f.flags & kFlagSize) {
    // bounded by what the block headers allow before anything is sized from it: a stored block
    // gives its own length, a compressed one at most the block maximum and at most 255-fold
    BlockWalk w;
    w.s = f.pos;
    uint64_t bound = 0;
    for (;;) {
      st = w.next(p, n, f);
      if (st < 0) return TSG_E_CORRUPT;
      if (st == 0) break;
      const uint64_t grow = 255ull * w.size;
      bound += w.stored ? w.size : (grow < f.bmax ? grow : f.bmax);
    }
    if (f.csize > bound) return TSG_E_CORRUPT;
    size = f.csize;
    return size >= (1ull << 31) ? TSG_E_UNSUPPORTED : TSG_OK;
  }
  BlockWalk w;
  w.s = f.pos;
  uint64_t total = 0;
  for (;;) {
    st = w.next(p, n, f);
    if (st < 0) return TSG_E_CORRUPT;
    if (st == 0) break;
    uint32_t len = w.size;
    if (!w.stored) {
      // (a linked block may reach back into the frame's earlier output)
      const uint64_t back = (f.flags & kFlagIndep) ? 0 : total;
      st = lz4_block<false>(p + w.data, w.size, nullptr, back, back + f.bmax, len);
      if (st != TSG_OK) return st;
    }
    total += len;
    if (total >= (1ull << 31)) return TSG_E_UNSUPPORTED;
  }
  size = total;
  return TSG_OK;
}

// Decode the frame at p into out[0 .. cap); len: bytes decoded. cap is lz4_size()'s answer:
// a frame that decodes to anything else is an error.
__device__ inline int lz4_decode(const uint8_t *p, uint32_t n, uint8_t *out, uint64_t cap, uint64_t &len) {
  Frame f;
  len = 0;
  int st = lz4_header(p, n, f);
  if (st != TSG_OK) return st;
  BlockWalk w;
  w.s = f.pos;
  uint64_t d = 0;
  for (;;) {
    st = w.next(p, n, f);
    if (st < 0) return TSG_E_CORRUPT;
    if (st == 0) break;
    uint32_t bl = w.size;
    if (w.stored) {
      if (bl > cap - d) return TSG_E_CORRUPT;
      for (uint32_t j = 0; j < bl; j++) out[d + j] = p[w.data + j];
    } else {
      const uint64_t lim = cap - d < f.bmax ? cap : d + f.bmax;
      if (f.flags & kFlagIndep) st = lz4_block<true>(p + w.data, w.size, out + d, 0, lim - d, bl);
      else st = lz4_block<true>(p + w.data, w.size, out, d, lim, bl);
      if (st != TSG_OK) return st;
    }
    if ((f.flags & kFlagBlockSum) && xxh32(out + d, bl) != w.sum && xxh32(p + w.data, w.size) != w.sum)
      return TSG_E_CORRUPT;
    d += bl;
  }
  if (f.flags & kFlagContentSum) {
    if (n - w.s < 4 || rd32(p + w.s) != xxh32(out, d)) return TSG_E_CORRUPT;
  }
  if (d != cap) return TSG_E_CORRUPT;  // (content size that disagrees, or a size pass that does)
  len = d;
  return TSG_OK;
}

}  // namespace lz4dev
}  // namespace tsg
