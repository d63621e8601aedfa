// san_wal_refresh.cpp — TEST INFRASTRUCTURE ONLY: the host half of tsg_wal_block_refresh
// (block.cpp: the tail replay and plan_wal_refresh) under AddressSanitizer / UBSan, with its
// own main, no device and no libtsg.so (tests/test_wal_refresh_host.py compiles and runs it).
//
// For every case a WAL file is written in two or three stages (each a prefix of the next).
// The first stage is decoded; every later one is reached by a refresh, whose plan is applied
// here on the host exactly as wal_merge_kernel applies it on the device (the delta's
// positions, the old entry a position reads, the per-key renumbering tables, all-ones kept),
// and the result is compared with a fresh decode of that stage: every entry's record fields,
// every key's value set per entry by its values' bytes, the narrow keys' dictionaries and
// columns id for id (they are canonical), the mutable header, and the replay state itself.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tempo_amd/csrc/block.hpp"
#include "../../tempo_amd/csrc/writer.hpp"

namespace tsg {
void set_last_error(const std::string &) {}
}  // namespace tsg

using namespace tsg;

static int g_fail = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
      std::printf(__VA_ARGS__);                         \
      std::printf("\n");                                \
      g_fail++;                                         \
    }                                                   \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

static std::string g_dir;

static std::vector<uint8_t> wal_bytes(const std::vector<SearchEntryIn> &e, int enc) {
  const std::string p = g_dir + "/wal.tmp";
  write_wal_search(p, e, enc);
  std::vector<uint8_t> out;
  if (!read_file(p, out)) fail(TSG_E_IO, "wal.tmp missing");
  return out;
}

static SearchEntryIn entry(Rng &r, uint32_t i) {
  SearchEntryIn e;
  e.id.resize(16);
  for (auto &b : e.id) b = uint8_t(r.next());
  e.start = 1700000000ull * 1000000000ull + uint64_t(r.below(3600)) * 1000000000ull + r.below(1000000000);
  e.end = e.start + uint64_t(r.below(5000)) * 1000000ull + r.below(1000000);
  const uint32_t nk = 1 + r.below(5);
  for (uint32_t k = 0; k < nk; k++) {
    const std::string key = "k" + std::to_string(r.below(6));
    const uint32_t nv = 1 + (r.below(4) == 0 ? r.below(3) : 0);
    for (uint32_t v = 0; v < nv; v++) e.tags[key].insert("v" + std::to_string(r.below(8)));
  }
  if (r.below(5) == 0) e.tags["K" + std::to_string(r.below(6))].insert("V-" + std::to_string(r.below(4)));  // key order broken
  e.tags["root.service.name"].insert("svc-" + std::to_string(r.below(5)));
  if (r.below(3)) e.tags["root.name"].insert("op-" + std::to_string(r.below(40)));
  e.tags["wide"].insert("w" + std::to_string(i * 7919u % 100000u));  // > 255 value sets: a two-byte column
  return e;
}

// entry -> key -> the values of the set its column holds ("\x01" "absent" when the key is absent)
static std::string set_text(const HostBlock &h, size_t k, uint32_t sid) {
  if (sid == kNone) return "\x01" "absent";
  const KeyColumn &kc = h.keys[k];
  std::string t;
  for (uint32_t i = kc.set_off[sid]; i < kc.set_off[sid + 1]; i++) {
    t += std::string(h.dict_value(int(k), kc.set_vals[i]));
    t += '\x02';
  }
  return t;
}
static std::string value_text(const HostBlock &h, int key, uint32_t vid) {
  return key < 0 || vid == kNone ? "\x01" "absent" : std::string(h.dict_value(key, vid));
}

// The plan applied as the device applies it: `o` is the old block with its columns, `nb` the
// new block's host side as plan_wal_refresh left it; returns nb's key columns.
static std::vector<std::vector<uint32_t>> apply_plan(const HostBlock &o, const HostBlock &nb, const WalRefreshPlan &p) {
  const size_t nd = p.ndelta();
  std::vector<uint32_t> dpos(nd);
  for (size_t d = 0; d < nd; d++) dpos[d] = p.dlo[d] + p.dins[d];
  std::vector<std::vector<uint32_t>> cols(nb.keys.size(), std::vector<uint32_t>(size_t(p.n_new), 0xdeadbeefu));
  for (uint64_t j = 0; j < p.n_new; j++) {
    size_t lo = 0, hi = nd;
    while (lo < hi) {
      const size_t m = (lo + hi) >> 1;
      if (dpos[m] < j) lo = m + 1;
      else hi = m;
    }
    const bool from_delta = lo < nd && dpos[lo] == j;
    const uint64_t idx = from_delta ? lo : j - p.dins[lo];
    CHECK(from_delta || idx < p.n_old, "entry %llu reads old entry %llu of %llu", (unsigned long long)j,
          (unsigned long long)idx, (unsigned long long)p.n_old);
    if (!from_delta && idx >= p.n_old) continue;
    for (size_t k = 0; k < nb.keys.size(); k++) {
      uint32_t v;
      if (from_delta) {
        v = p.dcol[k][idx];
      } else if (k >= o.keys.size()) {
        v = kNone;
      } else {
        v = o.keys[k].col[idx];
        if (v != kNone && !p.set_lut[k].empty()) {
          CHECK(v < p.set_lut[k].size(), "set id %u outside the table of key %zu", v, k);
          v = v < p.set_lut[k].size() ? p.set_lut[k][v] : kNone;
        }
      }
      // the width the device stores it in holds it
      const int w = nb.keys[k].width();
      CHECK(v == kNone || (w == 1 ? v < 0xff : w == 2 ? v < 0xffff : true), "set id %u does not fit width %d", v, w);
      cols[k][j] = v;
    }
  }
  return cols;
}

static void compare(const char *what, const HostBlock &nb, const std::vector<std::vector<uint32_t>> &cols,
                    const HostBlock &f) {
  CHECK(nb.n == f.n, "%s: entries %llu vs %llu", what, (unsigned long long)nb.n, (unsigned long long)f.n);
  if (nb.n != f.n) return;
  CHECK(nb.partial == f.partial, "%s: partial", what);
  CHECK(nb.fb_bytes == f.fb_bytes, "%s: fb_bytes %llu vs %llu", what, (unsigned long long)nb.fb_bytes, (unsigned long long)f.fb_bytes);
  CHECK(nb.min_dur == f.min_dur && nb.max_dur == f.max_dur, "%s: header durations", what);
  CHECK(nb.stream_tags == f.stream_tags, "%s: mutable header tags", what);
  CHECK(nb.ids == f.ids && nb.id_len == f.id_len, "%s: ids", what);
  CHECK(nb.start == f.start && nb.end == f.end, "%s: times", what);
  CHECK(nb.page_fb_bytes == f.page_fb_bytes && nb.page_entries == f.page_entries && nb.page_first == f.page_first, "%s: pages", what);
  CHECK(nb.keys.size() == f.keys.size(), "%s: keys %zu vs %zu", what, nb.keys.size(), f.keys.size());
  CHECK(nb.wal && f.wal && nb.wal->consumed == f.wal->consumed && nb.wal->last_off == f.wal->last_off &&
            nb.wal->last_hash == f.wal->last_hash,
        "%s: replay state", what);
  CHECK(nb.wal->rid == f.wal->rid && nb.wal->rid_off == f.wal->rid_off, "%s: record ids", what);
  CHECK(nb.wal->objs.size() == f.wal->objs.size(), "%s: objects", what);
  for (size_t e = 0; e < nb.wal->objs.size() && e < f.wal->objs.size(); e++)
    CHECK(*nb.wal->objs[e] == *f.wal->objs[e], "%s: object of entry %zu", what, e);
  for (size_t e = 0; e < nb.n; e++) {
    CHECK(value_text(nb, nb.svc_key, nb.svc_vid[e]) == value_text(f, f.svc_key, f.svc_vid[e]), "%s: service name of %zu", what, e);
    CHECK(value_text(nb, nb.name_key, nb.name_vid[e]) == value_text(f, f.name_key, f.name_vid[e]), "%s: root name of %zu", what, e);
  }
  for (size_t k = 0; k < nb.keys.size(); k++) {
    auto it = f.key_index.find(nb.keys[k].name);
    CHECK(it != f.key_index.end(), "%s: key %s", what, nb.keys[k].name.c_str());
    if (it == f.key_index.end()) continue;
    const size_t fk = size_t(it->second);
    const KeyColumn &a = nb.keys[k], &b = f.keys[fk];
    // (a replaced entry's value sets stay in the refreshed dictionary when no entry uses them
    // any more; a fresh decode never saw them. Its values all live on in the combined entry.)
    CHECK(a.nvals() == b.nvals() && a.nsets() >= b.nsets() && a.identity == b.identity, "%s: key %s shape", what, a.name.c_str());
    for (size_t e = 0; e < nb.n; e++)
      if (set_text(nb, k, cols[k][e]) != set_text(f, fk, b.col[e])) {
        CHECK(false, "%s: key %s entry %zu", what, a.name.c_str(), e);
        break;
      }
    if (a.width() == 1 && a.nsets() == b.nsets()) {  // canonical: the same ids, the same dictionary (interned once per context)
      CHECK(cols[k] == b.col, "%s: narrow key %s column ids", what, a.name.c_str());
      CHECK(a.dict_bytes == b.dict_bytes && a.dict_off == b.dict_off && a.set_off == b.set_off && a.set_vals == b.set_vals,
            "%s: narrow key %s dictionary", what, a.name.c_str());
    }
  }
}

// old (with columns) + file -> the refreshed block with its columns put back, as `out`
static int refresh(const HostBlock &old, const std::vector<uint8_t> &file, bool window, HostBlock &out, WalRefreshPlan &plan) {
  const uint64_t base = window ? std::min<uint64_t>(old.wal->last_off, file.size()) : 0;
  plan_wal_refresh(old, file.data() + base, base, file.size(), out, plan);
  if (plan.mode != 1) return plan.mode;
  auto cols = apply_plan(old, out, plan);
  for (size_t k = 0; k < out.keys.size(); k++) out.keys[k].col = std::move(cols[k]);
  return 1;
}
static std::vector<std::vector<uint32_t>> cols_of(const HostBlock &h) {
  std::vector<std::vector<uint32_t>> c;
  for (auto &k : h.keys) c.push_back(k.col);
  return c;
}

static void run_stages(const char *what, const std::vector<std::vector<SearchEntryIn>> &stages, int enc, bool window) {
  std::vector<SearchEntryIn> all;
  HostBlock cur;
  size_t prev_len = 0;
  for (size_t s = 0; s < stages.size(); s++) {
    all.insert(all.end(), stages[s].begin(), stages[s].end());
    const std::vector<uint8_t> file = wal_bytes(all, enc);
    HostBlock fresh;
    decode_wal_search_block(file.data(), file.size(), enc, fresh);
    if (s == 0) {
      cur = std::move(fresh);
    } else {
      HostBlock nb;
      WalRefreshPlan plan;
      const int mode = refresh(cur, file, window, nb, plan);
      CHECK(mode == 1, "%s stage %zu: mode %d", what, s, mode);
      if (mode != 1) return;
      CHECK(plan.bytes_replayed == file.size() - prev_len, "%s stage %zu: replayed %llu of %zu appended bytes", what, s,
            (unsigned long long)plan.bytes_replayed, file.size() - prev_len);
      CHECK(plan.pages_replayed == stages[s].size(), "%s stage %zu: pages", what, s);
      CHECK(plan.entries_added == nb.n - cur.n && plan.entries_added + plan.entries_combined == plan.pages_replayed,
            "%s stage %zu: added %llu combined %llu", what, s, (unsigned long long)plan.entries_added,
            (unsigned long long)plan.entries_combined);
      const std::string tag = std::string(what) + " stage " + std::to_string(s);
      compare(tag.c_str(), nb, cols_of(nb), fresh);
      cur = std::move(nb);
    }
    prev_len = file.size();
  }
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: san_wal_refresh <scratch dir>\n");
    return 2;
  }
  g_dir = argv[1];
  try {
    for (int enc : {0, 2}) {  // none, snappy
      Rng r{uint64_t(17 + enc)};
      // 1. inserts in front of, between and behind; then ids met again (twice in one tail too)
      std::vector<SearchEntryIn> a, b, c;
      for (uint32_t i = 0; i < 300; i++) a.push_back(entry(r, i));
      for (uint32_t i = 0; i < 60; i++) b.push_back(entry(r, 300 + i));
      b[0].id.assign(16, 0x00);
      b[1].id.assign(16, 0xff);
      b[2].id = {0x01, 0x02};  // (a short id: sorts by bytes, right aligned in the column)
      for (uint32_t i = 0; i < 12; i++) {
        SearchEntryIn d = entry(r, 1000 + i);
        d.id = i < 6 ? a[i * 31 % a.size()].id : b[i].id;
        d.start -= 70000ull * 1000000000ull;  // the combined span passes 65535 s
        c.push_back(d);
      }
      c.push_back(c[3]);  // the same id twice in one tail
      c.back().tags["late"].insert("only-in-the-tail");
      for (uint32_t i = 0; i < 20; i++) c.push_back(entry(r, 2000 + i));
      run_stages("mixed", {a, b, c}, enc, enc == 2);
      // 2. a key that outgrows its one-byte column (250 -> 260 value sets), ids renumbered on the way
      std::vector<SearchEntryIn> g0, g1;
      for (uint32_t i = 0; i < 250; i++) {
        SearchEntryIn e = entry(r, i);
        e.tags.erase("wide");
        e.tags["grow"].insert("g" + std::to_string(1000 - 2 * i));
        g0.push_back(e);
      }
      std::vector<SearchEntryIn> g01;  // 250 -> 253: stays narrow, renumbered
      for (uint32_t i = 0; i < 3; i++) {
        SearchEntryIn e = entry(r, 300 + i);
        e.tags["grow"].insert("g" + std::to_string(1001 - 100 * i));
        g01.push_back(e);
      }
      for (uint32_t i = 0; i < 7; i++) {
        SearchEntryIn e = entry(r, 400 + i);
        e.tags["grow"].insert("g" + std::to_string(1003 - 100 * i));
        g1.push_back(e);
      }
      run_stages("widen", {g0, g01, g1}, enc, false);
      // 3. crossing the 512-entry unit, from 511 and from exactly 512
      for (uint32_t n0 : {511u, 512u}) {
        std::vector<SearchEntryIn> p0, p1;
        for (uint32_t i = 0; i < n0; i++) p0.push_back(entry(r, i));
        for (uint32_t i = 0; i < 513 - n0 + (n0 == 512); i++) p1.push_back(entry(r, 600 + i));
        run_stages("unit", {p0, p1}, enc, true);
      }
    }
    // 4. nothing new, a damaged appended page, a changed prefix, a shorter file
    {
      Rng r{99};
      std::vector<SearchEntryIn> a, ab;
      for (uint32_t i = 0; i < 40; i++) a.push_back(entry(r, i));
      ab = a;
      for (uint32_t i = 0; i < 10; i++) ab.push_back(entry(r, 100 + i));
      const auto fa = wal_bytes(a, 2), fab = wal_bytes(ab, 2);
      CHECK(fab.size() > fa.size() && std::memcmp(fa.data(), fab.data(), fa.size()) == 0, "a stage is a prefix of the next");
      HostBlock old, nb;
      WalRefreshPlan plan;
      decode_wal_search_block(fa.data(), fa.size(), 2, old);
      CHECK(refresh(old, fa, false, nb, plan) == 0 && plan.bytes_replayed == 0, "nothing new: mode %d", plan.mode);
      // the 4th appended page's header checksum flipped (page: u32 total | u16 header length | header | payload)
      std::vector<uint8_t> bad = fab;
      size_t off = fa.size();
      for (int i = 0; i < 3; i++) off += le32(bad.data() + off);
      const size_t good_end = off;
      bad[off + 6] ^= 0x5a;
      HostBlock fresh;
      decode_wal_search_block(bad.data(), bad.size(), 2, fresh);
      CHECK(fresh.partial && fresh.n == 43, "the damaged file opens partial with 43 entries (%llu)", (unsigned long long)fresh.n);
      CHECK(refresh(old, bad, true, nb, plan) == 1, "damaged tail: mode %d", plan.mode);
      CHECK(plan.bytes_replayed == good_end - fa.size() && plan.pages_replayed == 3, "damaged tail: the pages before it are kept");
      compare("damaged tail", nb, cols_of(nb), fresh);
      HostBlock nb2;
      CHECK(refresh(nb, bad, true, nb2, plan) == 0, "a partial block whose page is still damaged: mode %d", plan.mode);
      // the damage directly behind the old block: no new entry, but the result is partial
      std::vector<uint8_t> bad0 = fab;
      bad0[fa.size() + 6] ^= 0x5a;
      decode_wal_search_block(bad0.data(), bad0.size(), 2, fresh);
      CHECK(refresh(old, bad0, false, nb, plan) == 1 && plan.ndelta() == 0, "damage at once: mode %d", plan.mode);
      compare("damage at once", nb, cols_of(nb), fresh);
      // ... and repaired since (a page that was torn when the block was opened): replayed now
      decode_wal_search_block(fab.data(), fab.size(), 2, fresh);
      CHECK(refresh(nb, fab, true, nb2, plan) == 1 && plan.pages_replayed == 10, "repaired page: mode %d", plan.mode);
      compare("repaired page", nb2, cols_of(nb2), fresh);
      // prefix changed (same length), shorter file
      std::vector<uint8_t> other = fab;
      other[old.wal->last_off + 9] ^= 1;
      CHECK(refresh(old, other, false, nb, plan) == 2 && !plan.reason.empty(), "changed prefix: mode %d", plan.mode);
      std::vector<uint8_t> shorter(fa.begin(), fa.end() - 5);
      CHECK(refresh(old, shorter, true, nb, plan) == 2 && !plan.reason.empty(), "shorter file: mode %d", plan.mode);
      // not a WAL block
      HostBlock backend;
      backend.has_meta = true;
      int code = 0;
      try {
        plan_wal_refresh(backend, fa.data(), 0, fa.size(), nb, plan);
      } catch (const Error &e) {
        code = e.code;
      }
      CHECK(code == TSG_E_UNSUPPORTED, "a backend block: code %d", code);
    }
  } catch (const Error &e) {
    std::printf("FAIL: error %d: %s\n", e.code, e.what());
    return 1;
  }
  if (g_fail) {
    std::printf("san_wal_refresh: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("san_wal_refresh: ok\n");
  return 0;
}
