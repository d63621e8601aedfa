// zstd_enc.hpp — a Zstandard frame compressor written from RFC 8878, for the block writers
// (writer.cpp: tooling for synthetic data and test fixtures; not on the search path). The
// reference writes zstd pages through klauspost/compress/zstd (tempodb/encoding/v2/pool.go);
// any conforming frame is read back the same way, so this writer makes its own choices:
//
//   frame (3.1.1)       Window_Descriptor covering the whole input (at least 1 KiB), a 4-byte
//                       Frame_Content_Size, optional Content_Checksum (XXH64, low 32 bits)
//   blocks (3.1.1.2)    <= 128 KiB of input each: RLE for a run of one byte, raw where the
//                       compressed form does not save 1/64th of the block, else compressed
//   matching            greedy, one probe of a 4-byte hash over the whole input, so an offset
//                       may reach back past 64 KiB and into earlier blocks
//   literals (3.1.1.3.1) RLE when all equal, Huffman (4.2; 1 stream below 256 literals, 4 from
//                       there on; weights direct or FSE-compressed, the smaller) where it pays,
//                       else raw
//   sequences (3.1.1.3.2) predefined tables (or, by flag, FSE-described ones; RLE mode for a
//                       table of one symbol), repeat offsets (3.1.1.5)
// The flag bits (tsg_debug_set "zstd_writer_flags") let a test force each form.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tsg {
namespace zenc {

enum : uint32_t {
  kChecksum = 1,       // Content_Checksum
  kRawLiterals = 2,    // never Huffman
  kDirectWeights = 4,  // Huffman weights as 4-bit fields (where <= 128 of them)
  kFseWeights = 8,     // Huffman weights FSE-compressed
  kFseSeqTables = 16,  // FSE_Compressed_Mode tables in blocks of >= 32 sequences
  kLiteralsOnly = 32,  // no matches and no raw / RLE blocks: compressed blocks of literals (<= 64 KiB)
};

constexpr uint32_t kLLBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,   15,    16,    18,
                                  20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
constexpr uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr uint32_t kMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,  17,  18,  19,   20,
                                  21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,  35,  37,  39,   41,
                                  43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
constexpr uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
// predefined distributions (3.1.1.3.2.2)
constexpr int16_t kLLDef[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int16_t kMLDef[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
constexpr int16_t kOFDef[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

inline int hibit(uint32_t x) { return 31 - __builtin_clz(x); }  // x > 0
inline uint32_t rd32(const uint8_t *p) {
  uint32_t v;
  std::memcpy(&v, p, 4);
  return v;
}

// little-endian bit writer; a backward stream (4.1, 4.2.2) is one of these closed with a 1 bit
struct BitW {
  std::vector<uint8_t> &o;
  uint64_t acc = 0;
  int nb = 0;
  explicit BitW(std::vector<uint8_t> &out) : o(out) {}
  void add(uint64_t v, int n) {  // n <= 32
    if (!n) return;
    acc |= (v & ((1ull << n) - 1)) << nb;
    nb += n;
    for (; nb >= 8; nb -= 8, acc >>= 8) o.push_back(uint8_t(acc));
  }
  void align() {
    if (nb) o.push_back(uint8_t(acc));
    acc = 0;
    nb = 0;
  }
  void close() {
    add(1, 1);
    align();
  }
};

// ---- FSE (4.1) ------------------------------------------------------------------------------
// The decoding table as the decoder builds it, and its inverse: a decoder in state X of symbol
// s reads nb[X] bits b and moves to Y = base[X] + b, so the encoder, which walks the symbols
// backwards and knows Y, emits s by finding the one state X of s whose range holds Y.
struct Fse {
  int al = 0;
  std::vector<uint8_t> sym, nb;
  std::vector<uint16_t> base;
  std::vector<std::vector<uint16_t>> from;  // from[s][Y] = X
  std::vector<int> first;                   // the state of s that reads the most bits (the final state)
  uint32_t encode(uint32_t s, uint32_t y, BitW &w) const {
    const uint32_t x = from[s][y];
    w.add(y - base[x], nb[x]);
    return x;
  }
};
inline void fse_build(Fse &t, const int16_t *norm, int nsym, int al) {
  const uint32_t size = 1u << al;
  t.al = al;
  t.sym.assign(size, 0);
  t.nb.assign(size, 0);
  t.base.assign(size, 0);
  std::vector<uint32_t> next(size_t(nsym), 0);
  uint32_t high = size;
  for (int s = 0; s < nsym; s++)
    if (norm[s] == -1) {
      t.sym[--high] = uint8_t(s);
      next[s] = 1;
    }
  const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
  uint32_t pos = 0;
  for (int s = 0; s < nsym; s++) {
    if (norm[s] <= 0) continue;
    next[s] = uint32_t(norm[s]);
    for (int i = 0; i < norm[s]; i++) {
      t.sym[pos] = uint8_t(s);
      do pos = (pos + step) & mask;
      while (pos >= high);
    }
  }
  t.from.assign(size_t(nsym), {});
  t.first.assign(size_t(nsym), -1);
  for (uint32_t x = 0; x < size; x++) {
    const uint32_t s = t.sym[x], n = next[s]++;
    t.nb[x] = uint8_t(al - hibit(n));
    t.base[x] = uint16_t((n << t.nb[x]) - size);
    if (t.from[s].empty()) t.from[s].assign(size, 0);
    if (t.first[s] < 0) t.first[s] = int(x);
    for (uint32_t y = t.base[x]; y < uint32_t(t.base[x]) + (1u << t.nb[x]); y++) t.from[s][y] = uint16_t(x);
  }
}
inline void fse_rle(Fse &t, uint8_t s) {  // RLE_Mode: one state, no bits
  t.al = 0;
  t.sym.assign(1, s);
  t.nb.assign(1, 0);
  t.base.assign(1, 0);
  t.from.assign(size_t(s) + 1, {});
  t.from[s].assign(1, 0);
  t.first.assign(size_t(s) + 1, 0);
}
// counts -> probabilities summing to 1 << al, every present symbol >= 1
inline void fse_normalize(const std::vector<uint32_t> &cnt, int al, std::vector<int16_t> &norm) {
  const int64_t size = 1ll << al;
  uint64_t total = 0;
  for (uint32_t c : cnt) total += c;
  norm.assign(cnt.size(), 0);
  int64_t sum = 0;
  for (size_t s = 0; s < cnt.size(); s++)
    if (cnt[s]) {
      norm[s] = int16_t(std::max<int64_t>(1, int64_t(uint64_t(cnt[s]) * uint64_t(size) / total)));
      sum += norm[s];
    }
  for (; sum != size; sum += sum < size ? 1 : -1) {  // the rounding error goes to the largest symbol
    const size_t big = size_t(std::max_element(norm.begin(), norm.end()) - norm.begin());
    norm[big] = int16_t(norm[big] + (sum < size ? 1 : -1));
  }
}
// FSE_Table_Description (4.1.1), byte aligned at its end
inline void fse_write_description(const std::vector<int16_t> &norm, int al, std::vector<uint8_t> &out) {
  BitW w(out);
  w.add(uint32_t(al - 5), 4);
  int32_t remaining = 1 << al;
  size_t s = 0;
  while (remaining > 0) {
    const int bits = hibit(uint32_t(remaining + 1)) + 1;
    const uint32_t lower = (1u << (bits - 1)) - 1, thr = (1u << bits) - 1 - uint32_t(remaining + 1);
    const uint32_t v = uint32_t(norm[s] + 1);
    if (v < thr) w.add(v, bits - 1);
    else w.add(v > lower ? v + thr : v, bits);
    remaining -= norm[s] < 0 ? 1 : norm[s];
    const bool zero = norm[s] == 0;
    s++;
    if (zero) {  // repeat flags: how many more zeros follow
      size_t run = 0;
      while (s + run < norm.size() && norm[s + run] == 0) run++;
      s += run;
      for (; run >= 3; run -= 3) w.add(3, 2);
      w.add(run, 2);
    }
  }
  w.align();
}

// ---- Huffman (4.2) ----------------------------------------------------------------------------
struct Huf {
  int maxb = 0, last = 0;  // last: the highest symbol present (its weight is implied)
  uint8_t len[256] = {0};
  uint16_t code[256] = {0};
};
// code lengths <= 11 of the present symbols (>= 2 of them): a Huffman tree, the counts halved
// until it is shallow enough
inline void huf_lengths(const uint32_t *cnt_in, uint8_t *len) {
  uint32_t cnt[256];
  std::memcpy(cnt, cnt_in, sizeof cnt);
  for (;;) {
    struct Node {
      uint64_t w;
      int l, r;
    };
    std::vector<Node> nodes;
    std::vector<int> live;
    for (int s = 0; s < 256; s++)
      if (cnt[s]) {
        live.push_back(int(nodes.size()));
        nodes.push_back({cnt[s], -1, s});
      }
    while (live.size() > 1) {
      std::sort(live.begin(), live.end(), [&](int a, int b) { return nodes[a].w > nodes[b].w; });
      const int a = live.back();
      live.pop_back();
      const int b = live.back();
      live.pop_back();
      live.push_back(int(nodes.size()));
      nodes.push_back({nodes[a].w + nodes[b].w, a, b});
    }
    std::memset(len, 0, 256);
    int deepest = 0;
    std::vector<std::pair<int, int>> st{{live[0], 0}};
    while (!st.empty()) {
      const auto [n, d] = st.back();
      st.pop_back();
      if (nodes[n].l < 0) {
        len[nodes[n].r] = uint8_t(d);
        deepest = std::max(deepest, d);
      } else {
        st.push_back({nodes[n].l, d + 1});
        st.push_back({nodes[n].r, d + 1});
      }
    }
    if (deepest <= 11) return;
    for (int s = 0; s < 256; s++)
      if (cnt[s]) cnt[s] = (cnt[s] + 1) / 2;
  }
}
// the canonical codes as the decoder's table lays them out (4.2.1): longest codes first,
// symbols ascending within a length; a symbol's code is the top len bits of its table index
inline void huf_codes(Huf &h) {
  h.maxb = 0;
  for (int s = 0; s < 256; s++)
    if (h.len[s]) {
      h.maxb = std::max<int>(h.maxb, h.len[s]);
      h.last = s;
    }
  uint32_t count[13] = {0}, idx[13] = {0};
  for (int s = 0; s < 256; s++)
    if (h.len[s]) count[h.len[s]]++;
  idx[h.maxb] = 0;
  for (int b = h.maxb; b >= 1; b--) idx[b - 1] = idx[b] + count[b] * (1u << (h.maxb - b));
  for (int s = 0; s < 256; s++) {
    const int b = h.len[s];
    if (!b) continue;
    h.code[s] = uint16_t(idx[b] >> (h.maxb - b));
    idx[b] += 1u << (h.maxb - b);
  }
}
// Huffman_Tree_Description (4.2.1): false when this form cannot hold the weights
inline bool huf_write_direct(const Huf &h, std::vector<uint8_t> &out) {
  const int n = h.last;  // weights of symbols 0 .. last - 1
  if (n > 128) return false;
  out.push_back(uint8_t(127 + n));
  for (int i = 0; i < n; i += 2) {
    const int w0 = h.len[i] ? h.maxb + 1 - h.len[i] : 0;
    const int w1 = i + 1 < n && h.len[i + 1] ? h.maxb + 1 - h.len[i + 1] : 0;
    out.push_back(uint8_t(w0 << 4 | w1));
  }
  return true;
}
inline bool huf_write_fse(const Huf &h, std::vector<uint8_t> &out) {
  const int n = h.last;
  if (n < 2) return false;
  std::vector<uint8_t> w(size_t(n), 0);
  std::vector<uint32_t> cnt(13, 0);
  for (int i = 0; i < n; i++) {
    w[i] = uint8_t(h.len[i] ? h.maxb + 1 - h.len[i] : 0);
    cnt[w[i]]++;
  }
  if (std::count_if(cnt.begin(), cnt.end(), [](uint32_t c) { return c != 0; }) < 2) return false;
  const int al = n >= 48 ? 6 : 5;
  std::vector<int16_t> norm;
  fse_normalize(cnt, al, norm);
  std::vector<uint8_t> body;
  fse_write_description(norm, al, body);
  Fse t;
  fse_build(t, norm.data(), int(norm.size()), al);
  // two interleaved states: even symbols on the first, odd ones on the second; the last two
  // symbols are the final states, which read past the stream's start (4.2.1.2)
  uint32_t st[2];
  st[(n - 1) & 1] = uint32_t(t.first[w[n - 1]]);
  st[(n - 2) & 1] = uint32_t(t.first[w[n - 2]]);
  BitW bw(body);
  for (int i = n - 3; i >= 0; i--) st[i & 1] = t.encode(w[i], st[i & 1], bw);
  bw.add(st[1], al);
  bw.add(st[0], al);
  bw.close();
  if (body.size() >= 128) return false;
  out.push_back(uint8_t(body.size()));
  out.insert(out.end(), body.begin(), body.end());
  return true;
}
inline void huf_stream(const Huf &h, const uint8_t *p, size_t n, std::vector<uint8_t> &out) {
  BitW w(out);
  for (size_t i = n; i-- > 0;) w.add(h.code[p[i]], h.len[p[i]]);
  w.close();
}

// Literals_Section (3.1.1.3.1)
inline void put_bits_le(std::vector<uint8_t> &o, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) o.push_back(uint8_t(v >> (8 * i)));
}
inline void literals_plain(const uint8_t *lit, size_t n, bool rle, std::vector<uint8_t> &out) {
  const uint32_t type = rle ? 1 : 0;
  if (n < 32) put_bits_le(out, n << 3 | type, 1);
  else if (n < 4096) put_bits_le(out, n << 4 | 1 << 2 | type, 2);
  else put_bits_le(out, n << 4 | 3 << 2 | type, 3);
  if (rle) out.push_back(lit[0]);
  else out.insert(out.end(), lit, lit + n);
}
inline void literals_section(const uint8_t *lit, size_t n, uint32_t flags, std::vector<uint8_t> &out) {
  if (n > 1 && std::all_of(lit, lit + n, [&](uint8_t c) { return c == lit[0]; })) return literals_plain(lit, n, true, out);
  if (n < 32 || (flags & kRawLiterals)) return literals_plain(lit, n, false, out);
  uint32_t cnt[256] = {0};
  for (size_t i = 0; i < n; i++) cnt[lit[i]]++;
  Huf h;
  huf_lengths(cnt, h.len);
  huf_codes(h);
  std::vector<uint8_t> direct, fse, body;
  const bool okd = !(flags & kFseWeights) && huf_write_direct(h, direct);
  const bool okf = !(flags & kDirectWeights) && huf_write_fse(h, fse);
  if (!okd && !okf) return literals_plain(lit, n, false, out);
  body = okd && (!okf || direct.size() <= fse.size()) ? direct : fse;
  if (n < 256) {
    huf_stream(h, lit, n, body);
  } else {  // 4 streams behind a jump table of the first three sizes
    const size_t seg = (n + 3) / 4, at = body.size();
    body.resize(at + 6);
    for (int q = 0; q < 4; q++) {
      const size_t before = body.size(), lo = size_t(q) * seg;
      huf_stream(h, lit + lo, q < 3 ? seg : n - 3 * seg, body);
      const size_t sz = body.size() - before;
      if (sz > 65535) return literals_plain(lit, n, false, out);
      if (q < 3) {
        body[at + 2 * q] = uint8_t(sz);
        body[at + 2 * q + 1] = uint8_t(sz >> 8);
      }
    }
  }
  const size_t cs = body.size();
  if (cs >= n) return literals_plain(lit, n, false, out);  // does not pay
  if (n < 256) put_bits_le(out, 2 | 0 << 2 | uint64_t(n) << 4 | uint64_t(cs) << 14, 3);
  else if (n < 1024) put_bits_le(out, 2 | 1 << 2 | uint64_t(n) << 4 | uint64_t(cs) << 14, 3);
  else if (n < 16384) put_bits_le(out, 2 | 2 << 2 | uint64_t(n) << 4 | uint64_t(cs) << 18, 4);
  else put_bits_le(out, 2 | 3 << 2 | uint64_t(n) << 4 | uint64_t(cs) << 22, 5);
  out.insert(out.end(), body.begin(), body.end());
}

// ---- sequences (3.1.1.3.2) --------------------------------------------------------------------
struct Seq {
  uint32_t ll, ml, off;
};
struct Coded {  // a sequence as its three codes and their extra bits
  uint8_t llc, mlc, ofc;
  uint32_t llx, mlx, ofx;
};
inline int code_of(const uint32_t *base, int n, uint32_t v) {
  int c = n - 1;
  while (base[c] > v) c--;
  return c;
}
// Offset_Value with the repeat offsets of 3.1.1.5, and their update
inline uint32_t offset_value(uint32_t off, uint32_t ll, uint32_t rep[3]) {
  uint32_t ofv = off + 3;
  if (ll) {
    if (off == rep[0]) ofv = 1;
    else if (off == rep[1]) ofv = 2;
    else if (off == rep[2]) ofv = 3;
  } else {
    if (off == rep[1]) ofv = 1;
    else if (off == rep[2]) ofv = 2;
    else if (rep[0] > 1 && off == rep[0] - 1) ofv = 3;
  }
  if (ofv > 3) {
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = off;
  } else {
    const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
    if (idx) {
      if (idx > 1) rep[2] = rep[1];
      rep[1] = rep[0];
      rep[0] = off;
    }
  }
  return ofv;
}
// one table of the three: its mode bits, its description into `desc`, the table into t
inline uint32_t seq_table(Fse &t, const std::vector<uint8_t> &codes, int nsym, const int16_t *def, int defn, int defal,
                          int lo_al, int max_al, bool described, std::vector<uint8_t> &desc) {
  if (!described) {
    fse_build(t, def, defn, defal);
    return 0;  // Predefined_Mode
  }
  std::vector<uint32_t> cnt(size_t(nsym), 0);
  for (uint8_t c : codes) cnt[c]++;
  if (std::count_if(cnt.begin(), cnt.end(), [](uint32_t c) { return c != 0; }) == 1) {
    fse_rle(t, codes[0]);
    desc.push_back(codes[0]);
    return 1;  // RLE_Mode
  }
  const int al = std::min(max_al, std::max(lo_al, hibit(uint32_t(codes.size()))));
  std::vector<int16_t> norm;
  fse_normalize(cnt, al, norm);
  fse_write_description(norm, al, desc);
  fse_build(t, norm.data(), nsym, al);
  return 2;  // FSE_Compressed_Mode
}
inline void sequences_section(const std::vector<Seq> &seqs, uint32_t flags, uint32_t rep[3], std::vector<uint8_t> &out) {
  const size_t n = seqs.size();
  if (n < 128) out.push_back(uint8_t(n));
  else if (n < 0x7F00) {
    out.push_back(uint8_t((n >> 8) + 128));
    out.push_back(uint8_t(n));
  } else {
    out.push_back(255);
    put_bits_le(out, n - 0x7F00, 2);
  }
  if (!n) return;
  std::vector<Coded> cs(n);
  std::vector<uint8_t> llc(n), mlc(n), ofc(n);
  for (size_t i = 0; i < n; i++) {
    const Seq &s = seqs[i];
    Coded &c = cs[i];
    const uint32_t ofv = offset_value(s.off, s.ll, rep);
    llc[i] = c.llc = uint8_t(code_of(kLLBase, 36, s.ll));
    mlc[i] = c.mlc = uint8_t(code_of(kMLBase, 53, s.ml));
    ofc[i] = c.ofc = uint8_t(hibit(ofv));
    c.llx = s.ll - kLLBase[c.llc];
    c.mlx = s.ml - kMLBase[c.mlc];
    c.ofx = ofv - (1u << c.ofc);
  }
  const bool described = (flags & kFseSeqTables) && n >= 32;
  Fse ll, of, ml;
  std::vector<uint8_t> desc;
  uint32_t modes = seq_table(ll, llc, 36, kLLDef, 36, 6, 6, 9, described, desc) << 6;
  modes |= seq_table(of, ofc, 32, kOFDef, 29, 5, 5, 8, described, desc) << 4;
  modes |= seq_table(ml, mlc, 53, kMLDef, 53, 6, 6, 9, described, desc) << 2;
  out.push_back(uint8_t(modes));
  out.insert(out.end(), desc.begin(), desc.end());
  // the bitstream is read backwards: written here from the last sequence to the first (4.1)
  BitW w(out);
  const Coded &z = cs[n - 1];
  uint32_t sll = uint32_t(ll.first[z.llc]), sof = uint32_t(of.first[z.ofc]), sml = uint32_t(ml.first[z.mlc]);
  w.add(z.llx, kLLBits[z.llc]);
  w.add(z.mlx, kMLBits[z.mlc]);
  w.add(z.ofx, z.ofc);
  for (size_t i = n - 1; i-- > 0;) {
    const Coded &c = cs[i];
    sof = of.encode(c.ofc, sof, w);
    sml = ml.encode(c.mlc, sml, w);
    sll = ll.encode(c.llc, sll, w);
    w.add(c.llx, kLLBits[c.llc]);
    w.add(c.mlx, kMLBits[c.mlc]);
    w.add(c.ofx, c.ofc);
  }
  w.add(sml, ml.al);
  w.add(sof, of.al);
  w.add(sll, ll.al);
  w.close();
}

// ---- XXH64 (the content checksum) ---------------------------------------------------------------
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t rd64(const uint8_t *p) {
  uint64_t v;
  std::memcpy(&v, p, 8);
  return v;
}
inline uint64_t xxh64(const uint8_t *p, uint64_t n) {
  const uint64_t P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P3 = 1609587929392839161ull,
                 P4 = 9650029242287828579ull, P5 = 2870177450012600261ull;
  uint64_t h, i = 0;
  if (n >= 32) {
    uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
    for (; i + 32 <= n; i += 32)
      for (int k = 0; k < 4; k++) v[k] = rotl64(v[k] + rd64(p + i + 8 * k) * P2, 31) * P1;
    h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
    for (int k = 0; k < 4; k++) h = (h ^ (rotl64(v[k] * P2, 31) * P1)) * P1 + P4;
  } else {
    h = P5;
  }
  h += n;
  for (; i + 8 <= n; i += 8) h = rotl64(h ^ (rotl64(rd64(p + i) * P2, 31) * P1), 27) * P1 + P4;
  if (i + 4 <= n) {
    h = rotl64(h ^ (uint64_t(rd32(p + i)) * P1), 23) * P2 + P3;
    i += 4;
  }
  for (; i < n; i++) h = rotl64(h ^ (uint64_t(p[i]) * P5), 11) * P1;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

// ---- the frame (3.1.1) ----------------------------------------------------------------------------
inline void block_header(std::vector<uint8_t> &out, bool last, uint32_t type, uint32_t size) {
  put_bits_le(out, (last ? 1u : 0u) | type << 1 | size << 3, 3);
}
inline void zstd_frame_encode(const uint8_t *src, size_t n, uint32_t flags, std::vector<uint8_t> &out) {
  put_bits_le(out, 0xFD2FB528u, 4);
  out.push_back(uint8_t(2u << 6 | ((flags & kChecksum) ? 4u : 0u)));  // 4-byte content size, a window, no dictionary
  {  // Window_Descriptor (3.1.1.1.2): the smallest window >= n + 16 (and >= 1 KiB)
    const uint64_t need = uint64_t(n) + 16;
    uint32_t e = 0, m = 0;
    for (;; m == 7 ? (m = 0, e++) : m++) {
      const uint64_t base = 1ull << (10 + e);
      if (base + base / 8 * m >= need) break;
    }
    out.push_back(uint8_t(e << 3 | m));
  }
  put_bits_le(out, n, 4);
  const size_t block_in = (flags & kLiteralsOnly) ? 65536 : 131072;
  std::vector<uint32_t> head(1u << 16, 0);  // position + 1 of the last 4 bytes seen with this hash
  auto hash = [](uint32_t v) { return (v * 2654435761u) >> 16; };
  uint32_t rep[3] = {1, 4, 8};
  std::vector<Seq> seqs;
  std::vector<uint8_t> lits, blk;
  size_t b0 = 0;
  do {
    const size_t b1 = std::min(n, b0 + block_in), len = b1 - b0;
    const bool last = b1 == n;
    const bool forced = (flags & kLiteralsOnly) != 0;
    if (!forced && len > 0 && std::all_of(src + b0, src + b1, [&](uint8_t c) { return c == src[b0]; })) {
      // (the positions of an RLE block stay out of the hash table: later blocks match elsewhere)
      block_header(out, last, 1, uint32_t(len));
      out.push_back(src[b0]);
      b0 = b1;
      continue;
    }
    seqs.clear();
    lits.clear();
    size_t i = b0, anchor = b0;
    while (!forced && i + 4 <= b1) {
      const uint32_t v = rd32(src + i), hh = hash(v), c = head[hh];
      head[hh] = uint32_t(i + 1);
      if (!c || rd32(src + c - 1) != v) {
        i++;
        continue;
      }
      const size_t from = c - 1;
      size_t ml = 4;
      while (i + ml < b1 && src[from + ml] == src[i + ml]) ml++;
      lits.insert(lits.end(), src + anchor, src + i);
      seqs.push_back({uint32_t(i - anchor), uint32_t(ml), uint32_t(i - from)});
      for (size_t k = i + 1; k < i + ml && k + 4 <= n; k++) head[hash(rd32(src + k))] = uint32_t(k + 1);
      i += ml;
      anchor = i;
    }
    lits.insert(lits.end(), src + anchor, src + b1);
    blk.clear();
    uint32_t r[3] = {rep[0], rep[1], rep[2]};
    literals_section(lits.data(), lits.size(), flags, blk);
    sequences_section(seqs, flags, r, blk);
    if (forced || blk.size() + (len >> 6) + 2 <= len) {  // (compressed only for a gain of 1/64th and 2 bytes)
      block_header(out, last, 2, uint32_t(blk.size()));
      out.insert(out.end(), blk.begin(), blk.end());
      std::memcpy(rep, r, sizeof rep);  // (a raw or RLE block leaves the repeat offsets alone)
    } else {
      block_header(out, last, 0, uint32_t(len));
      out.insert(out.end(), src + b0, src + b1);
    }
    b0 = b1;
  } while (b0 < n);
  if (flags & kChecksum) put_bits_le(out, uint32_t(xxh64(src, n)), 4);
}

}  // namespace zenc
}  // namespace tsg
