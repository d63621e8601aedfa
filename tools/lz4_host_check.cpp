// lz4_host_check.cpp — builds the lz4 frame decoder (tempo_amd/csrc/lz4_dev.hpp) for the host
// and decodes every page of a file of v2 pages ([u32 total][u16 0][lz4 frame]), writing the
// decoded pages to stdout as [u32 len][bytes] (or [u32 0xffffffff][i32 status]) so a test can
// compare them with an independent lz4 (pyarrow / liblz4). Each frame is copied into a heap
// block of exactly its length, so a sanitizer build sees any read past its end.
// Test tooling: the product runs the same parser on the GPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "../include/tsg.h"
#define TSG_LZ4_HOST
#include "../tempo_amd/csrc/lz4_dev.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> d;
  uint8_t buf[65536];
  size_t r;
  while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + r);
  std::fclose(f);
  size_t off = 0;
  while (off + 6 <= d.size()) {
    uint32_t tl;
    std::memcpy(&tl, d.data() + off, 4);
    if (tl < 6 || tl > d.size() - off) return 3;
    const uint32_t n = tl - 6;
    uint8_t *p = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    std::memcpy(p, d.data() + off + 6, n);
    uint64_t size = 0, len = 0;
    int st = tsg::lz4dev::lz4_size(p, n, size);
    uint8_t *out = static_cast<uint8_t *>(std::malloc(size ? size : 1));
    if (st == TSG_OK) st = tsg::lz4dev::lz4_decode(p, n, out, size, len);
    if (st != TSG_OK) {
      const uint32_t m = 0xffffffffu;
      std::fwrite(&m, 4, 1, stdout);
      std::fwrite(&st, 4, 1, stdout);
    } else {
      const uint32_t l = uint32_t(len);
      std::fwrite(&l, 4, 1, stdout);
      std::fwrite(out, 1, len, stdout);
    }
    std::free(out);
    std::free(p);
    off += tl;
  }
  return 0;
}
