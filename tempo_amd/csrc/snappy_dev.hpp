// snappy_dev.hpp — the snappy framing format of v2 pages written at the snappy encoding
// (backend.Encoding 6, the default), compiled for the host (common.cpp) and for the device
// (find.hip).
//
//   Reader.fill       vendor/github.com/golang/snappy/decode.go:121-232
//   decodedLen        decode.go:32-43 (binary.Uvarint, encoding/binary/varint.go)
//   sizes, checksum   snappy.go:54-64,91-95
//
// What the reference Reader does, and so what is done here: the first chunk is the stream
// identifier, and every identifier chunk carries the same six bytes; a chunk longer than the
// Reader's buffer or than the bytes left is an error, as is a partial chunk header at the end;
// compressed (0x00) and uncompressed (0x01) chunks open with the masked CRC-32C of their decoded
// bytes and decode to at most 64 KiB; a compressed chunk's block opens with its decoded length, a
// varint of at most 10 bytes; chunk types 0x02..0x7f are errors, 0x80..0xfe are skipped. The
// block's tags are decoded by the walk's users: snappy_block_decode in common.cpp (the loaders'
// copy loops), snap_block_wave in find.hip (one wave in lockstep).
// Every length comes from untrusted bytes: each read is checked against the chunk's end.
#pragma once
#ifndef TSG_SNAPPY_HOST
#include <hip/hip_runtime.h>
#endif
#include <cstdint>

namespace tsg {
namespace snapdev {

constexpr uint32_t kMaxBlock = 65536;      // maxBlockSize: the most a chunk decodes to
constexpr uint32_t kMaxChunk = 76490 + 4;  // maxEncodedLenOfMaxBlockSize + checksumSize: Reader.buf

__device__ __forceinline__ uint32_t rd32(const uint8_t *p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}  // (lz4dev has the same: each codec header stands alone)
// the stored form of a chunk's CRC-32C (snappy.go:91-95)
__device__ __forceinline__ uint32_t crc_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// binary.Uvarint over p[0 .. n): the bytes used, or 0 when the input ends inside the value or
// the value overflows 64 bits (an 11th byte, or a 10th above 1)
__device__ inline uint32_t uvarint(const uint8_t *p, uint32_t n, uint64_t &v) {
  v = 0;
  for (uint32_t i = 0; i < n && i < 10; i++) {
    const uint32_t c = p[i];
    if (c < 0x80) {
      if (i == 9 && c > 1) return 0;
      v |= uint64_t(c) << (7 * i);
      return i + 1;
    }
    v |= uint64_t(c & 0x7f) << (7 * i);
  }
  return 0;
}

// The walk over a stream's chunks: next() gives one data chunk at a time.
struct ChunkWalk {
  enum Err { kHeader = -1, kNoIdent = -2, kTooLarge = -3, kTruncated = -4, kNoSum = -5, kVarint = -6,
             kBlockTooLarge = -7, kIdent = -8, kReserved = -9 };
  uint32_t s = 0;     // offset of the next chunk header
  bool ident = false; // the stream identifier has been seen
  uint32_t type;      // 0x00 compressed, 0x01 uncompressed
  uint32_t data;      // the chunk's bytes after the checksum
  uint32_t size;      // and their count
  uint32_t crc;       // the stored (masked) checksum
  uint32_t ulen;      // decoded length: declared (compressed) or size (uncompressed)
  uint32_t block;     // compressed: the first tag, after the varint (block .. data + size)
  // 1: a data chunk, 0: the stream ended at a chunk boundary, < 0: an Err
  __device__ int next(const uint8_t *b, uint32_t n) {
    while (s < n) {
      if (n - s < 4) return kHeader;
      const uint32_t ct = b[s], cl = rd32(b + s) >> 8;
      s += 4;
      if (!ident && ct != 0xff) return kNoIdent;
      ident = true;
      if (cl > kMaxChunk) return kTooLarge;
      if (cl > n - s) return kTruncated;
      const uint32_t at = s;
      s += cl;
      if (ct == 0x00 || ct == 0x01) {
        if (cl < 4) return kNoSum;
        type = ct;
        crc = rd32(b + at);
        data = block = at + 4;
        size = ulen = cl - 4;
        if (ct == 0x00) {
          uint64_t v;
          const uint32_t k = uvarint(b + data, size, v);
          if (k == 0) return kVarint;
          ulen = uint32_t(v);
          block = data + k;
          if (v > kMaxBlock) return kBlockTooLarge;
        } else if (size > kMaxBlock) {
          return kBlockTooLarge;
        }
        return 1;
      }
      if (ct == 0xff) {
        for (uint32_t q = 0; q < 6; q++)
          if (cl != 6 || b[at + q] != uint8_t("sNaPpY"[q])) return kIdent;
      } else if (ct <= 0x7f)
        return kReserved;
    }
    return 0;
  }
};

// The decoded length of the stream at b: a full walk of its chunks, their declared lengths summed.
__device__ inline int snappy_size(const uint8_t *b, uint32_t n, uint64_t &size) {
  ChunkWalk w;
  size = 0;
  for (int r; (r = w.next(b, n)) != 0; size += w.ulen)
    if (r < 0) return TSG_E_CORRUPT;  // (size: what the chunks before the bad one declare)
  return size >= (1ull << 31) ? TSG_E_UNSUPPORTED : TSG_OK;
}

}  // namespace snapdev
}  // namespace tsg
