// zstd_host_check.cpp — builds the device zstd decoders (tempo_amd/csrc/zstd_dev.hpp: the one-lane
// decoder and the wave decoder with one lane) and the writer's compressor (zstd_enc.hpp) for the
// host. Test tooling: the product runs the same decoders on the GPU.
//
//   zcheck FILE                 decode every page of a v2 data file ([u32 total][u16 0][frames]; a
//                               file named *.zst is one bare payload) with both decoders, which
//                               must agree (exit 4), writing the pages to stdout as [u32 len][bytes]
//                               (or [u32 0xffffffff][i32 status]) for a test to compare with an
//                               independent zstd (pyarrow / libzstd)
//   zcheck --stats FILE         one JSON line per page: the forms its frames use
//   zcheck --encode FLAGS IN OUT  IN compressed by the writer (zenc flag bits) into OUT
//   zcheck --fuzz N SEED FILE.. on every page: the last 10 bytes cut, the first block header's size
//                               raised past the page, the frame content size off by one; then N
//                               single-byte and truncation mutations of random pages. Each must end
//                               in bytes, TSG_E_CORRUPT or TSG_E_UNSUPPORTED, the same from both
//                               decoders (exit 5 otherwise); built with -fsanitize=address,undefined
//                               this is the decoders' memory-safety check (8 bytes of slack on
//                               either side of a payload: the bit reader loads aligned words).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#define __device__
#define __constant__
#define __forceinline__ inline
static inline int __clz(uint32_t x) { return x ? __builtin_clz(x) : 32; }
#include "../include/tsg.h"
struct ZStat {
  uint32_t block[4], lit[4], streams[2], weights[2], seq_mode[4], repeats, max_off;
};
static ZStat g_zstat;
#define ZDEV_STAT(...) __VA_ARGS__
#define TSG_ZSTD_HOST
#include "../tempo_amd/csrc/zstd_dev.hpp"
#include "../tempo_amd/csrc/zstd_enc.hpp"

using Bytes = std::vector<uint8_t>;

static bool read_all(const char *path, Bytes &d) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t r;
  while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + r);
  std::fclose(f);
  return true;
}
static bool pages_of(const char *path, std::vector<Bytes> &pages) {
  Bytes d;
  if (!read_all(path, d)) return false;
  const std::string name(path);
  if (name.size() > 4 && name.substr(name.size() - 4) == ".zst") {
    pages.push_back(d);
    return true;
  }
  size_t off = 0;
  while (off + 6 <= d.size()) {
    uint32_t tl;
    std::memcpy(&tl, d.data() + off, 4);
    if (tl < 6 || tl > d.size() - off) return false;
    pages.emplace_back(d.begin() + long(off) + 6, d.begin() + long(off + tl));
    off += tl;
  }
  return true;
}

static tsg::zdev::Work *W = new tsg::zdev::Work;
static tsg::zdev::WaveWork *X = new tsg::zdev::WaveWork;

// one payload through one decoder, from a heap block of its own with 8 bytes of slack either side
static int decode(const Bytes &page, bool wave, Bytes &out) {
  const uint32_t n = uint32_t(page.size());
  uint8_t *blk = static_cast<uint8_t *>(std::calloc(size_t(n) + 16, 1));
  uint8_t *p = blk + 8;
  std::memcpy(p, page.data(), n);
  uint64_t bound = 0, len = 0;
  int st = tsg::zdev::zstd_size(p, n, bound);
  if (st != TSG_OK) bound = 0;  // (an error leaves a partial sum there)
  uint8_t *o = static_cast<uint8_t *>(std::malloc(bound ? bound : 1));
  if (st == TSG_OK)
    st = wave ? tsg::zdev::zstd_decode_wave(p, n, o, bound, len, *W, *X, 0) : tsg::zdev::zstd_decode(p, n, o, bound, len, *W);
  out.assign(o, o + (st == TSG_OK ? len : 0));
  std::free(o);
  std::free(blk);
  return st;
}
// both decoders; -1000 when they disagree
static int decode_both(const Bytes &page, Bytes &out) {
  Bytes a;
  const int s1 = decode(page, false, a), s2 = decode(page, true, out);
  return s1 == s2 && a == out ? s1 : -1000;
}

static int fuzz(int argc, char **argv) {
  const long iters = std::atol(argv[2]);
  uint64_t x = std::strtoull(argv[3], nullptr, 10) * 2654435761u + 88172645463325252ull;
  auto rnd = [&]() {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    return x;
  };
  std::vector<Bytes> pages;
  for (int i = 4; i < argc; i++)
    if (!pages_of(argv[i], pages)) return 2;
  if (pages.empty()) return 2;
  long okc = 0, corrupt = 0, unsup = 0, fixed = 0;
  Bytes out;
  auto run = [&](const Bytes &m) {
    const int st = decode_both(m, out);
    if (st == TSG_OK) okc++;
    else if (st == TSG_E_CORRUPT) corrupt++;
    else if (st == TSG_E_UNSUPPORTED) unsup++;
    else {
      std::fprintf(stderr, "unexpected status %d\n", st);
      std::exit(5);
    }
    return st;
  };
  for (const Bytes &pg : pages) {
    if (run(pg) != TSG_OK) {
      std::fprintf(stderr, "a page as shipped does not decode\n");
      return 5;
    }
    if (pg.size() < 20 || pg[0] != 0x28 || (pg[4] & 0x20)) continue;  // (the fixed patterns: frames with a Window_Descriptor)
    Bytes m(pg.begin(), pg.end() - 10);  // the last 10 bytes cut
    int bad = run(m) == TSG_E_CORRUPT ? 1 : 0;
    const uint32_t fcs_bytes = (pg[4] >> 6) == 0 ? 0 : 1u << (pg[4] >> 6), did = (pg[4] & 3) == 3 ? 4 : (pg[4] & 3);
    const size_t bh = 6 + did + fcs_bytes;
    m = pg;  // the first block header's size beyond the page
    m[bh + 1] = 0xff, m[bh + 2] = 0xff;
    bad += run(m) == TSG_E_CORRUPT ? 1 : 0;
    if (fcs_bytes) {  // the content size off by one
      m = pg;
      m[6 + did] ^= 1;
      bad += run(m) == TSG_E_CORRUPT ? 1 : 0;
    } else {
      bad++;
    }
    if (bad != 3) {
      std::fprintf(stderr, "a fixed damage pattern was not reported as corrupt\n");
      return 5;
    }
    fixed += 3;
  }
  for (long it = 0; it < iters; it++) {
    Bytes m = pages[rnd() % pages.size()];
    if (m.empty()) continue;
    if (rnd() % 4 == 0) m.resize(rnd() % m.size());
    else m[rnd() % m.size()] ^= uint8_t(1u << (rnd() % 8));
    run(m);
  }
  std::printf("{\"pages\": %zu, \"fixed\": %ld, \"mutations\": %ld, \"ok\": %ld, \"corrupt\": %ld, \"unsupported\": %ld}\n",
              pages.size(), fixed, iters, okc, corrupt, unsup);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string mode(argv[1]);
  if (mode == "--encode") {
    if (argc < 5) return 2;
    Bytes in, out;
    if (!read_all(argv[3], in)) return 2;
    tsg::zenc::zstd_frame_encode(in.data(), in.size(), uint32_t(std::atoi(argv[2])), out);
    FILE *f = std::fopen(argv[4], "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 1, out.size(), f);
    std::fclose(f);
    return 0;
  }
  if (mode == "--fuzz") return argc < 5 ? 2 : fuzz(argc, argv);
  const bool stats = mode == "--stats";
  if (stats && argc < 3) return 2;
  std::vector<Bytes> pages;
  if (!pages_of(argv[stats ? 2 : 1], pages)) return 3;
  for (const Bytes &pg : pages) {
    Bytes out;
    if (stats) {
      g_zstat = ZStat();
      const int st = decode(pg, true, out);
      const ZStat &z = g_zstat;
      std::printf("{\"status\": %d, \"bytes\": %zu, \"blocks\": {\"raw\": %u, \"rle\": %u, \"compressed\": %u}, "
                  "\"literals\": {\"raw\": %u, \"rle\": %u, \"huffman\": %u, \"treeless\": %u}, "
                  "\"streams\": {\"1\": %u, \"4\": %u}, \"weights\": {\"fse\": %u, \"direct\": %u}, "
                  "\"seq_tables\": {\"predefined\": %u, \"rle\": %u, \"fse\": %u, \"repeat\": %u}, "
                  "\"repeat_offsets\": %u, \"max_offset\": %u}\n",
                  st, out.size(), z.block[0], z.block[1], z.block[2], z.lit[0], z.lit[1], z.lit[2], z.lit[3], z.streams[0],
                  z.streams[1], z.weights[0], z.weights[1], z.seq_mode[0], z.seq_mode[1], z.seq_mode[2], z.seq_mode[3],
                  z.repeats, z.max_off);
      continue;
    }
    const int st = decode_both(pg, out);
    if (st == -1000) return 4;
    if (st != TSG_OK) {
      const uint32_t m = 0xffffffffu;
      std::fwrite(&m, 4, 1, stdout);
      std::fwrite(&st, 4, 1, stdout);
    } else {
      const uint32_t l = uint32_t(out.size());
      std::fwrite(&l, 4, 1, stdout);
      if (l) std::fwrite(out.data(), 1, out.size(), stdout);
    }
  }
  return 0;
}
