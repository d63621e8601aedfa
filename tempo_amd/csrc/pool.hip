// pool.hip — MI355X (gfx950) pool search: narrow full scans (limit 0) of Tempo search
// blocks with one workgroup per CU and a CU-wide work pool. The same predicates,
// records and result order as search_fast_kernel (search.hip); see DESIGN.md §4.
#include <dirent.h>
#include <fcntl.h>
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <sys/file.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <map>
#include <mutex>
#include <thread>
#include <vector>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <string>
#include <cstring>

#include <type_traits>

#include "aql.hpp"
#include "pool_kernels.hpp"
#include "search_common.hpp"
#include "terms_first.hpp"

namespace tsg {

// ------------------------------------------------------------------------------------
// host: the kernels' instances
//
// A query's shape (terms clamped to 4, duration filter, time range, non-temporal loads, terms
// first) as compile-time constants: f(nt, dur, range, ntl, tf) is called with
// std::integral_constants. Terms first exists only for shapes with a term and a filter on the scan
// word (kTermsFirstShape): any other shape resolves to the instance it always had.
static bool terms_first_shape(uint32_t nterms, bool dur, bool range) { return nterms > 0 && (dur || range); }
template <class F>
static auto with_shape(uint32_t nterms, bool dur, bool range, bool ntl, bool tf, F &&f) {
  auto flag = [](bool v, auto &&g) { return v ? g(std::true_type{}) : g(std::false_type{}); };
  auto flags = [&](auto nt) {
    return flag(dur, [&](auto d) {
      return flag(range, [&](auto r) {
        return flag(ntl, [&](auto n) {
          if constexpr (kTermsFirstShape<nt(), d(), r()>) {
            if (tf) return f(nt, d, r, n, std::true_type{});
          }
          return f(nt, d, r, n, std::false_type{});
        });
      });
    });
  };
  switch (nterms) {
    case 0: return flags(std::integral_constant<int, 0>{});
    case 1: return flags(std::integral_constant<int, 1>{});
    case 2: return flags(std::integral_constant<int, 2>{});
    case 3: return flags(std::integral_constant<int, 3>{});
    default: return flags(std::integral_constant<int, 4>{});
  }
}
enum class Kernel { pool, stat, resident };
using PoolFn = void (*)(PoolArgs);
static PoolFn pool_fn(Kernel kind, uint32_t nterms, bool dur, bool range, bool ntl, bool tf) {
  return with_shape(nterms, dur, range, ntl, tf, [&](auto nt, auto d, auto r, auto n, auto t) -> PoolFn {
    if (kind == Kernel::stat) return search_static_kernel<nt(), d(), r(), n(), t()>;
    return search_pool_kernel<nt(), d(), r(), n(), t()>;
  });
}
// (every resident instantiation referenced, so that the code object beside libtsg.so holds them
// all: the resident kernel is launched by symbol through the AQL queue only)
[[maybe_unused]] static void *resident_fn(uint32_t nterms, bool dur, bool range, bool ntl, bool tf) {
  return with_shape(nterms, dur, range, ntl, tf, [](auto nt, auto d, auto r, auto n, auto t) {
    return reinterpret_cast<void *>(search_resident_kernel<nt(), d(), r(), n(), t()>);
  });
}
// the device symbol of a kernel instance (Itanium mangling of the template)
static std::string kernel_symbol(Kernel kind, uint32_t nterms, bool dur, bool range, bool ntl, bool tf) {
  static const char *const name[] = {"18search_pool_kernel", "20search_static_kernel", "22search_resident_kernel"};
  char b[128];
  std::snprintf(b, sizeof b, "_ZN3tsg%sILi%uELb%dELb%dELb%dELb%dEEEvNS_%sE", name[int(kind)], std::min(nterms, 4u), int(dur),
                int(range), int(ntl), int(tf && terms_first_shape(nterms, dur, range)),
                kind == Kernel::resident ? "12ResidentArgs" : "8PoolArgs");
  return b;
}
// the argument ranges a query uses (arg_range), as the parts res_post and aql_dispatch copy
static const std::vector<std::pair<uint32_t, uint32_t>> &used_parts(uint32_t nsegs, uint32_t nbms) {
  thread_local std::vector<std::pair<uint32_t, uint32_t>> parts;
  parts.clear();
  for (int i = 0; i < kArgRanges; i++) {
    const ArgRange r = arg_range(i, nsegs, nbms);
    if (r.len) parts.push_back({r.off, r.len});
  }
  return parts;
}

// ---- resident search: host side -------------------------------------------------------
constexpr size_t kResDoorBytes = 256;  // the doorbell word's page ahead of the slots

// Device contexts open in this process, by device ordinal. A resident launch fills every CU
// of its device; a second context on the same device (the bench's concurrent streams, a
// second engine) would wait behind it, so resident launches run only while a context is
// alone on its device, and opening a second one ends the first one's launch.
static std::mutex g_ctx_mu;
// held by context_opened while it ends other contexts' launches and by context_closed before a
// context leaves the table: a context being shut down is never touched after it left (ADVICE r5;
// order: g_life_mu, then a context's mu — nothing holding a context's mu takes g_life_mu)
static std::mutex g_life_mu;
static std::multimap<int, DeviceCtx *> g_ctxs;
int contexts_on(int ordinal) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  return int(g_ctxs.count(ordinal));
}

// ---- other processes on the device. A resident launch holds every CU: a second
// process's kernels on the same GPU would wait behind it until its idle exit, or starve while it
// stays busy. Each process with a context on a GPU holds an flock on a file of its own named after
// the GPU's PCI bus id (TSG_COTENANT_DIR, default /dev/shm, else /tmp) and bumps a generation word
// in a shared page of that GPU; the resident path runs only while no other live process is
// registered on the GPU, re-counted (a directory scan; a file whose lock can be taken is a dead
// process's, removed) whenever the generation word has moved. TSG_COTENANT=0: no check.
struct CoTenant {
  int refs = 0, gen_fd = -1, live_fd = -1;
  uint32_t *gen = nullptr;
  std::string dir, prefix, live_path;
};
static std::mutex g_cot_mu;
static std::map<std::string, CoTenant> g_cot;
static std::string bus_id(int ordinal) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, ordinal) != hipSuccess) return std::string();
  for (char *c = bus; *c; c++) *c = char(std::tolower(uint8_t(*c)));
  return bus;
}
static void cotenant_register(DeviceCtx &dc) {
  if (DeviceCtx::env_u32("TSG_COTENANT", 1, 0, 1) == 0) return;
  const std::string bus = bus_id(dc.ordinal);
  if (bus.empty()) return;
  std::lock_guard<std::mutex> lk(g_cot_mu);
  CoTenant &ct = g_cot[bus];
  struct Publish {  // (every context of the GPU in this process reads the same registration)
    DeviceCtx &dc;
    CoTenant &ct;
    ~Publish() {
      dc.cot_gen = ct.gen;
      dc.cot_dir = ct.dir;
      dc.cot_prefix = ct.prefix;
    }
  } publish{dc, ct};
  if (ct.refs++ > 0) return;
  const char *e = std::getenv("TSG_COTENANT_DIR");
  ct.dir = e && *e ? e : access("/dev/shm", W_OK) == 0 ? "/dev/shm" : "/tmp";
  ct.prefix = "tsg-gpu-" + bus + ".";
  const std::string gpath = ct.dir + "/" + ct.prefix + "gen";
  ct.gen_fd = open(gpath.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
  if (ct.gen_fd < 0) return;
  (void)fchmod(ct.gen_fd, 0666);  // (another user's process shares the GPU too)
  struct stat st;
  if (fstat(ct.gen_fd, &st) == 0 && st.st_size < 4096 && ftruncate(ct.gen_fd, 4096) != 0) {
    close(ct.gen_fd);
    ct.gen_fd = -1;
    return;
  }
  void *m = mmap(nullptr, 4096, PROT_READ | PROT_WRITE, MAP_SHARED, ct.gen_fd, 0);
  if (m == MAP_FAILED) {
    close(ct.gen_fd);
    ct.gen_fd = -1;
    return;
  }
  ct.gen = static_cast<uint32_t *>(m);
  ct.live_path = ct.dir + "/" + ct.prefix + std::to_string(getpid());
  ct.live_fd = open(ct.live_path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0644);
  if (ct.live_fd >= 0 && flock(ct.live_fd, LOCK_EX | LOCK_NB) != 0) {
    close(ct.live_fd);
    ct.live_fd = -1;
  }
  __atomic_fetch_add(ct.gen, 1u, __ATOMIC_SEQ_CST);
}
static void cotenant_unregister(DeviceCtx &dc) {
  if (!dc.cot_gen) return;
  dc.cot_gen = nullptr;
  const std::string bus = bus_id(dc.ordinal);
  std::lock_guard<std::mutex> lk(g_cot_mu);
  auto it = g_cot.find(bus);
  if (it == g_cot.end() || --it->second.refs > 0) return;
  CoTenant &ct = it->second;
  if (ct.live_fd >= 0) {
    (void)unlink(ct.live_path.c_str());
    close(ct.live_fd);  // (the lock goes with it)
  }
  if (ct.gen) {
    __atomic_fetch_add(ct.gen, 1u, __ATOMIC_SEQ_CST);
    munmap(ct.gen, 4096);
  }
  if (ct.gen_fd >= 0) close(ct.gen_fd);
  g_cot.erase(it);
}
// other live processes registered on dc's GPU (0 when the check is off or unavailable)
static int cotenant_others(DeviceCtx &dc) {
  uint32_t *gen = dc.cot_gen;  // (mapped while this context is registered)
  if (!gen) return 0;
  const uint32_t g = __atomic_load_n(gen, __ATOMIC_ACQUIRE);
  if (dc.res_cotenant >= 0 && g == dc.res_cotenant_gen) return dc.res_cotenant;
  const std::string &dir = dc.cot_dir, &prefix = dc.cot_prefix, mine = prefix + std::to_string(getpid());
  int others = 0;
  if (DIR *d = opendir(dir.c_str())) {
    while (dirent *de = readdir(d)) {
      const std::string name = de->d_name;
      if (name.compare(0, prefix.size(), prefix) != 0 || name == prefix + "gen" || name == mine) continue;
      const std::string path = dir + "/" + name;
      const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
      if (fd < 0) continue;
      if (flock(fd, LOCK_EX | LOCK_NB) == 0) {  // nobody holds it: a process that died registered
        (void)unlink(path.c_str());
      } else {
        others++;
      }
      close(fd);
    }
    closedir(d);
  }
  dc.res_cotenant = others;
  dc.res_cotenant_gen = g;
  return others;
}

void context_opened(DeviceCtx &dc) {
  cotenant_register(dc);
  std::lock_guard<std::mutex> life(g_life_mu);
  std::vector<DeviceCtx *> others;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto r = g_ctxs.equal_range(dc.ordinal);
    for (auto it = r.first; it != r.second; ++it) others.push_back(it->second);
    g_ctxs.emplace(dc.ordinal, &dc);
  }
  for (DeviceCtx *o : others) {
    std::lock_guard<std::mutex> lk(o->mu);
    resident_quit(*o);
  }
}
void context_closed(DeviceCtx &dc) {
  {
    std::lock_guard<std::mutex> life(g_life_mu);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto r = g_ctxs.equal_range(dc.ordinal);
    for (auto it = r.first; it != r.second; ++it)
      if (it->second == &dc) {
        g_ctxs.erase(it);
        break;
      }
  }
  cotenant_unregister(dc);
}

// A query (or a quit) into mailbox slot seq % kResSlots: the argument words the query uses
// (`parts`: the same words res_word_used names, summed for the checksum), then the header
// whose sequence number the kernel polls — write-combined stores drained by sfence, pushed past
// the host data path by a posted HDP flush (the kernel re-reads a slot whose checksum does not
// match yet).
std::atomic<uint32_t> g_res_torn{0};  // test hook (tsg_debug_set "res_torn"): posts left to tear
static void res_post(DeviceCtx &dc, uint32_t seq, uint32_t cmd, const PoolArgs *PA,
                     const std::vector<std::pair<uint32_t, uint32_t>> *parts) {
  uint8_t *slot = dc.res_mem + kResDoorBytes + size_t(seq % kResSlots) * kResSlotBytes;
  uint32_t h0 = res_mix(cmd, kResCmdWord, seq, kResKey0), h1 = res_mix(cmd, kResCmdWord, seq, kResKey1);
  const auto *src = reinterpret_cast<const uint8_t *>(PA);
  if (PA) {
    for (const auto &pt : *parts) {
      std::memcpy(slot + kResHdrBytes + pt.first, src + pt.first, pt.second);
      for (uint32_t o = 0; o < pt.second; o += 4) {
        uint32_t v;
        std::memcpy(&v, src + pt.first + o, 4);
        h0 += res_mix(v, (pt.first + o) / 4, seq, kResKey0);
        h1 += res_mix(v, (pt.first + o) / 4, seq, kResKey1);
      }
    }
  }
  // test hook: the slot as a read that caught the host's writes half landed would see it — two
  // used words moved by +-d (the plain sum of the words unchanged: the additive check of round 5
  // accepted it) — repaired after 200 us; the kernel must re-read, not run it
  uint32_t torn = g_res_torn.load(std::memory_order_relaxed);
  const bool tear = PA && cmd == kResSearch && torn && g_res_torn.compare_exchange_strong(torn, torn - 1);
  const uint32_t o_s = uint32_t(offsetof(PoolArgs, start_s)), o_e = uint32_t(offsetof(PoolArgs, end_s));
  if (tear) {
    uint32_t a, b;
    std::memcpy(&a, src + o_s, 4);
    std::memcpy(&b, src + o_e, 4);
    a += 0x01000000u;
    b -= 0x01000000u;
    std::memcpy(slot + kResHdrBytes + o_s, &a, 4);
    std::memcpy(slot + kResHdrBytes + o_e, &b, 4);
  }
  __builtin_ia32_sfence();
  // the header's check words, then (after an sfence: posted writes arrive in order) its sequence
  // number, so a read that sees the new seq sees the new check words with it
  const ResHeader h{seq - 1, cmd, h0, h1};
  std::memcpy(slot + 4, reinterpret_cast<const uint8_t *>(&h) + 4, sizeof h - 4);
  __builtin_ia32_sfence();
  std::memcpy(slot, &seq, 4);
  __builtin_ia32_sfence();
  aql_hdp_flush(dc.aql);
  if (tear) {
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(200)) __builtin_ia32_pause();
    std::memcpy(slot + kResHdrBytes + o_s, src + o_s, 4);
    std::memcpy(slot + kResHdrBytes + o_e, src + o_e, 4);
    __builtin_ia32_sfence();
    aql_hdp_flush(dc.aql);
  }
}

// A resident launch of kernel `sym` serving queries from `first_seq` on. false: unavailable.
// `profiled`: the dispatch gets a completion signal with dispatch timestamps of its own
// (tsg_search_batch: the launch's device time, the clock rocprofv3's kernel trace reads).
static bool resident_launch(DeviceCtx &dc, const std::string &sym, uint32_t threads, uint32_t W, uint32_t first_seq) {
  if (!dc.res_mem) {
    void *p = nullptr;
    const size_t bytes = kResDoorBytes + size_t(kResSlots) * kResSlotBytes;
    if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) != hipSuccess) return false;
    HIP_OK(hipMemsetAsync(p, 0, bytes, dc.stream));
    HIP_OK(hipStreamSynchronize(dc.stream));
    dc.res_mem = static_cast<uint8_t *>(p);
    *reinterpret_cast<volatile uint32_t *>(dc.res_mem) = dc.res_seq;
  }
  const AqlKernel ak = aql_kernel(dc.aql, sym.c_str(), uint32_t(sizeof(ResidentArgs)));
  if (!ak.kobj) return false;
  dc.res_host.ensure(64);
  auto *err = static_cast<uint32_t *>(dc.res_host.p);
  __atomic_store_n(err, 0u, __ATOMIC_RELEASE);
  ResidentArgs RA{};
  RA.door = reinterpret_cast<const uint32_t *>(dc.res_mem);
  RA.slots = dc.res_mem + kResDoorBytes;
  RA.err = err;
  RA.first_seq = first_seq;
  RA.idle_ticks = DeviceCtx::env_u32("TSG_RESIDENT_IDLE_US", 10000, 100, 10000000) * 100u;  // (s_memrealtime: 100 MHz)
  RA.nthreads = threads;
  RA.ngroups = W;
  RA.mode = DeviceCtx::env_u32("TSG_RES_MODE", 0, 0, 255);
  const std::vector<std::pair<uint32_t, uint32_t>> parts{{0u, uint32_t(sizeof RA)}};
  const bool prof = dc.res_profile_next;
  dc.res_profile_next = false;
  const int ps = aql_dispatch(dc.aql, ak, W, threads, uint32_t(kPoolLds), &RA, parts, prof);
  if (prof) dc.res_profile_slot = ps;
  dc.res_alive = true;
  dc.res_kernel = sym;
  dc.res_threads = threads;
  dc.res_groups = W;
  dc.res_epoch = dc.mem_epoch;
  dc.res_launches++;
  return true;
}

void resident_quit(DeviceCtx &dc) {
  if (!dc.res_alive) return;
  dc.res_alive = false;
  if (!dc.aql || aql_done(dc.aql)) return;  // (left on its own: idle)
  const uint32_t seq = ++dc.res_seq;
  res_post(dc, seq, kResQuit, nullptr, nullptr);
  dc.res_quits++;
  // (the launch serves every query posted before the quit first: their callers may be waiting)
  const auto t0 = std::chrono::steady_clock::now();
  while (!aql_done(dc.aql)) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5))
      fail(TSG_E_DEVICE, "resident search kernel did not leave after a quit (5 s)");
    __builtin_ia32_pause();
  }
}

void resident_release(DeviceCtx &dc) {
  resident_quit(dc);
  if (dc.res_mem) (void)hipFree(dc.res_mem);
  dc.res_mem = nullptr;
  dc.res_host.release();
  for (auto &a : dc.res_areas) a.buf.release();
  dc.res_areas.clear();
  for (auto &b : dc.res_quarantine) b.release();
  dc.res_quarantine.clear();
}

uint64_t resident_batch_begin(DeviceCtx &dc) {
  std::lock_guard<std::mutex> lk(dc.mu);
  resident_quit(dc);
  dc.res_profile_next = true;
  dc.res_profile_slot = -1;
  return dc.res_launches;
}
uint64_t resident_batch_end(DeviceCtx &dc, uint64_t launches_before) {
  std::lock_guard<std::mutex> lk(dc.mu);
  const bool one = dc.res_launches == launches_before + 1 && dc.res_profile_slot >= 0;
  resident_quit(dc);  // (the dispatch completes: its end timestamp is written)
  dc.res_profile_next = false;
  const uint64_t ns = one && dc.aql ? aql_time_ns(dc.aql, dc.res_profile_slot) : 0;
  dc.res_profile_slot = -1;
  return ns;
}
static std::atomic<uint32_t> g_groups{0};
// (off by default: equalising the XCDs' mean ends raised every XCD's time per unit, span 24.9 vs
// 24.2 us in paired runs, profiles/r06_xsplit; TSG_RES_XSPLIT=1 turns it on)
static std::atomic<bool> g_xsplit{DeviceCtx::env_u32("TSG_RES_XSPLIT", 0, 0, 1) != 0};
static std::atomic<uint32_t> g_lb_bitmap{DeviceCtx::env_u32("TSG_LB_BITMAP", 2, 0, 2)};
// "terms_first": 0 off, 1 forced (where the instance exists), 2 auto (the default; TSG_TERMS_FIRST)
static std::atomic<int> g_terms_first{int(DeviceCtx::env_u32("TSG_TERMS_FIRST", 2, 0, 2))};
uint32_t debug_groups() { return g_groups.load(std::memory_order_relaxed); }
uint32_t debug_lb_bitmap() { return g_lb_bitmap.load(std::memory_order_relaxed); }
bool debug_xsplit() { return g_xsplit.load(std::memory_order_relaxed); }
int debug_set(const char *name, int64_t value) {
  if (!name) return TSG_E_INVALID;
  if (!std::strcmp(name, "res_torn")) {
    g_res_torn.store(uint32_t(std::max<int64_t>(0, value)));
    return TSG_OK;
  }
  if (!std::strcmp(name, "groups")) {
    g_groups.store(uint32_t(std::min<int64_t>(4096, std::max<int64_t>(0, value))));
    return TSG_OK;
  }
  if (!std::strcmp(name, "terms_first")) {
    g_terms_first.store(int(std::min<int64_t>(2, std::max<int64_t>(0, value))));
    return TSG_OK;
  }
  if (!std::strcmp(name, "xsplit")) {
    g_xsplit.store(value != 0);
    return TSG_OK;
  }
  if (!std::strcmp(name, "zstd_find_lane")) {  // (find.hip: 1 = the one-lane zstd page decoder)
    find_zstd_lane(value != 0);
    return TSG_OK;
  }
  if (!std::strcmp(name, "proto_batch_jobs")) {  // (proto_scan.hip: jobs per batched launch, 0 = default)
    proto_batch_cap(uint32_t(std::min<int64_t>(1 << 30, std::max<int64_t>(0, value))));
    return TSG_OK;
  }
  if (!std::strcmp(name, "lb_bitmap")) {
    g_lb_bitmap.store(uint32_t(std::min<int64_t>(2, std::max<int64_t>(0, value))));
    return TSG_OK;
  }
  if (!std::strcmp(name, "dict_stream_min")) {  // (search.hip: dictionaries above this many bytes stream, 0 = 1 MiB)
    dict_stream_min(uint64_t(std::max<int64_t>(0, value)));
    return TSG_OK;
  }
  if (!std::strcmp(name, "dict_stream_span"))  // (search.hip: bytes per wave, a multiple of 1024 up to 64 KiB, 0 = planned)
    return value >= 0 && dict_stream_span(uint64_t(value)) ? TSG_OK : TSG_E_INVALID;
  return TSG_E_INVALID;
}

// A query's result area (pinned, device-written): [256 B header | counts, cstride words per
// workgroup | stamps, 2 x u64 per workgroup | records, seg_cap per workgroup]. Queries in flight
// at once (concurrent callers, tsg_search_batch) hold one each; an area is reused only after its
// query's records were read.
static constexpr uint32_t kResCountStride = 16;  // one 64-byte line per workgroup's count
static size_t res_area_bytes(uint32_t W, uint32_t seg) {
  return 256 + align_up(size_t(W) * 4 * kResCountStride, 256) + align_up(size_t(W) * 8 * kResStampStride, 256) +
         size_t(W) * seg * sizeof(MatchRec);
}

// The oldest posted query whose counts are not all in, when the launch is gone (it left on its
// idle timeout just as queries were posted): launched again from that query with its kernel; it
// serves the posted queries from their slots (identical results). Queries that completed are never
// served again: their areas may have been reused. Caller holds dc.mu.
static void res_relaunch_inflight(DeviceCtx &dc) {
  if (!dc.aql || !aql_done(dc.aql)) return;
  for (const auto &kv : dc.res_inflight) {
    const DeviceCtx::ResArea &a = dc.res_areas[kv.second];
    const auto *counts = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(a.buf.p) + 256);
    bool complete = true;
    for (uint32_t w = 0; w < a.W && complete; w++)
      complete = __atomic_load_n(counts + size_t(w) * kResCountStride, __ATOMIC_ACQUIRE) != kCountPending;
    if (complete) continue;
    if (!resident_launch(dc, a.sym, dc.res_threads ? dc.res_threads : kResThreads, a.W, kv.first))
      fail(TSG_E_DEVICE, "resident search relaunch failed");
    dc.res_relaunches++;
    return;
  }
}

// Wait, with dc.mu released, until pred() holds (pred is evaluated with dc.mu held).
template <class P>
static void res_wait_unlocked(DeviceCtx &dc, std::unique_lock<std::mutex> &lk, P &&pred, const char *what) {
  const auto t0 = std::chrono::steady_clock::now();
  while (!pred()) {
    res_relaunch_inflight(dc);
    lk.unlock();
    for (int i = 0; i < 64; i++) __builtin_ia32_pause();
    std::this_thread::yield();
    lk.lock();
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) fail(TSG_E_DEVICE, what);
  }
}

// The XCD-weighted split of U units over W workgroups (W = 8 x G): XCD x's share of the units from
// the measured rates (res_xf), each XCD's share even over its G workgroups. Off (even runs) for
// small queries, W not a multiple of 8, or TSG_RES_XSPLIT=0.
static void res_split(const DeviceCtx &dc, PoolArgs &PA, uint32_t U, uint32_t W) {
  PA.xsplit = 0;
  if (!debug_xsplit() || W % 8 || U < 16u * W) return;
  const uint32_t G = W / 8;
  uint32_t T[8], sum = 0;
  for (int x = 0; x < 8; x++) {
    T[x] = uint32_t(double(U) * dc.res_xf[x]);
    sum += T[x];
  }
  for (int x = 0; sum < U; x = (x + 1) & 7, sum++) T[x]++;  // (rounding: a unit each, in XCD order)
  for (int x = 0; x < 8 && sum > U; x = (x + 1) & 7)
    if (T[x]) T[x]--, sum--;
  for (int x = 0; x < 8; x++) {
    PA.xn[x] = T[x] / G;
    PA.xr[x] = T[x] % G;
  }
  PA.xsplit = 1;
}
static uint32_t res_max_run(const PoolArgs &PA, uint32_t U, uint32_t W) {
  if (!PA.xsplit) return (U + W - 1) / W;
  uint32_t m = 0;
  for (int x = 0; x < 8; x++) m = std::max(m, PA.xn[x] + (PA.xr[x] ? 1u : 0u));
  return m;
}

// One query's workgroup stamps {seen, end} -> the XCDs' shares for the next queries. XCD x's
// workgroups took E_x (mean end after the first seen) for n_x units; its rate n_x / (E_x - c) with
// c ~ 2 us of fixed cost (first loads, output) moves the shares toward equal ends — the fixed point
// of the update is E_x equal whatever c is. Shares are smoothed (half old, half new) and kept
// within +-15 % of even. Queries below 32 units per workgroup are not used (their ends are fixed cost).
static void res_calibrate(DeviceCtx &dc, const unsigned long long *qst, const PoolArgs &PA, uint32_t U, uint32_t W) {
  if (W % 8 || U < 32u * W) return;
  unsigned long long lo = ~0ull;
  for (uint32_t w = 0; w < W; w++) lo = std::min(lo, qst[size_t(w) * kResStampStride]);
  double E[8] = {}, n[8] = {};
  uint32_t cnt[8] = {};
  for (uint32_t w = 0; w < W; w++) {
    const uint32_t x = w & 7u, i = w >> 3;
    const unsigned long long e = qst[size_t(w) * kResStampStride + 1];
    if (e < lo || e - lo > 100000000ull) return;  // (a stamp not written: skip the sample)
    E[x] += double(e - lo);
    n[x] += PA.xsplit ? double(PA.xn[x] + (i < PA.xr[x] ? 1u : 0u)) : double(PA.wq + (w < PA.wr ? 1u : 0u));
    cnt[x]++;
  }
  double r[8], rs = 0;
  for (int x = 0; x < 8; x++) {
    if (!cnt[x]) return;
    const double ex = E[x] / cnt[x], nx = n[x] / cnt[x];
    r[x] = nx / std::max(ex - 200.0, 0.25 * ex);  // (100 MHz ticks: 200 = 2 us)
    rs += r[x];
  }
  double fs = 0;
  for (int x = 0; x < 8; x++) {
    const double f = 0.5 * dc.res_xf[x] + 0.5 * r[x] / rs;
    dc.res_xf[x] = std::min(0.125 * 1.15, std::max(0.125 * 0.85, f));
    fs += dc.res_xf[x];
  }
  for (int x = 0; x < 8; x++) dc.res_xf[x] /= fs;
  dc.res_xsamples++;
}

// The host segments (dc.pool_seg records per workgroup, adaptive: the records of a sparse query
// stay on a few pages of pinned memory) against the largest workgroup count of a query that ran
// with seg_cap. A workgroup keeps at most min(seg_cap, rec_cap) records (its LDS buffer can be the
// smaller one, TSG_POOL_REC). dense: more than the LDS buffer holds, so this query (and its next
// few searches) take the other paths. grow: more than its segment held, so the query runs again
// with larger segments (doubled, with headroom: the next launch's split differs; at most the LDS
// buffer). fits: done, and when sparse again, smaller segments from the next query on.
enum class SegFit { fits, grow, dense };
static SegFit seg_fit(DeviceCtx &dc, const tsg_query &q, uint32_t maxc, uint32_t seg_cap, uint32_t rec_cap) {
  if (maxc > rec_cap) {
    dc.pool_skip = 16;
    dc.pool_skip_key = pool_query_key(q);
    return SegFit::dense;
  }
  if (maxc > seg_cap) {
    uint32_t want = 2 * seg_cap;
    while (want < maxc) want <<= 1;
    dc.pool_seg = std::min(want, rec_cap);
    return SegFit::grow;
  }
  if (dc.pool_seg > 32 && uint64_t(maxc) * 8 < dc.pool_seg) dc.pool_seg >>= 1;
  return SegFit::fits;
}

// block index -> the block's slot in the launch (a record names its block by index)
static const std::vector<uint32_t> &block_slots(const std::vector<ScanSeg> &segs) {
  thread_local std::vector<uint32_t> pos;
  uint32_t max_idx = 0;
  for (const auto &sg : segs) max_idx = std::max(max_idx, sg.block_idx);
  pos.assign(size_t(max_idx) + 1, 0);
  for (uint32_t i = 0; i < uint32_t(segs.size()); i++) pos[segs[i].block_idx] = i;
  return pos;
}
static uint32_t slot_of(const std::vector<uint32_t> &pos, const SearchOut::Rec &r) {
  const uint32_t bi = r.block_il & 0xffffffu;
  return bi < pos.size() ? pos[bi] : 0;
}

// The tail of a narrow search: `each(f)` calls f on the query's `total` records in the reference
// order (a block's records contiguous, in scan order). limit L: each block's part keeps its first
// L matches in scan order (the records of a part all lie in its range [e0, e1)), a prefix of the
// block's run. Fills out.recs, the blocks' counts and the bytes moved.
template <class Each>
static void finish_records(SearchOut &out, const std::vector<uint32_t> &pos, const std::vector<ScanSeg> &segs,
                           const std::vector<std::pair<uint32_t, Block *>> &blocks, uint32_t limit, uint64_t total,
                           uint32_t W, bool has_dur, bool has_range, bool terms_first, Each &&each) {
  thread_local std::vector<uint64_t> per;
  per.assign(segs.size(), 0);
  out.recs.resize(total);
  uint64_t kept = 0, run = 0, ps = ~0ull, cut = 0;
  each([&](const SearchOut::Rec &r) {
    const uint64_t s_i = slot_of(pos, r);
    if (s_i != ps) {
      ps = s_i;
      run = 0;
      cut = limit ? std::min<uint64_t>(limit, segs[s_i].cap) : segs[s_i].cap;
    }
    if (run++ < cut) {
      out.recs[kept++] = r;
      per[s_i]++;
    }
  });
  out.recs.resize(kept);
  for (size_t i = 0; i < segs.size(); i++)
    for (size_t bi = 0; bi < blocks.size(); bi++)
      if (blocks[bi].first == segs[i].block_idx) out.block_counts[bi] = per[i];
  out.scan_bytes += uint64_t(W) * 4 + kept * 32;  // + workgroup counts, + id/start/end of each record
  // (the caller counted 4 B of duration + 8 B of start / end per entry; these kernels read
  // the one 4 B packed scan word (ds_word.hpp) when either filter is on)
  // terms first: the term bytes only. The scan words (and the exact columns behind them) that the
  // lanes holding a term-passing entry load, 16 B per lane and step, are not counted: they are rare
  // where this mode is chosen, and their number is the data's, not the plan's.
  const uint64_t counted = (has_dur ? 4u : 0u) + (has_range ? 8u : 0u), read = counted && !terms_first ? 4u : 0u;
  for (const auto &sg : segs) out.scan_bytes -= (counted - read) * (sg.n - sg.e0);
}

// The resident path of pool_search: 1 = served (out filled), 0 = the records overflowed (the
// caller runs the segment / look-back path), -1 = not available (normal launches). dc.mu (lk) is
// released while the query runs: other callers plan and post their queries meanwhile, and the
// launch serves them back to back.
static int resident_search(DeviceCtx &dc, std::unique_lock<std::mutex> &lk, PoolArgs &PA,
                           const std::vector<ScanSeg> &segs, const std::vector<std::pair<uint32_t, Block *>> &blocks,
                           const tsg_query &q, uint32_t limit, uint32_t flags, bool has_dur, bool tf, uint32_t threads,
                           uint32_t W, uint32_t rec_cap, Tracer &tr, SearchOut &out) {
  const std::string sym = kernel_symbol(Kernel::resident, q.nterms, has_dur, q.has_range, dc.pool_nt, tf);
  const uint32_t U = PA.units;
  res_split(dc, PA, U, W);
  if (res_max_run(PA, U, W) > kResMaxUnits) return -1;
  // a free result area (D = TSG_RES_DEPTH queries in flight; a caller beyond that waits for one)
  static const uint32_t depth = DeviceCtx::env_u32("TSG_RES_DEPTH", 16, 1, kResSlots - 1);
  if (dc.res_areas.size() < depth) dc.res_areas.resize(depth);
  auto free_area = [&]() -> int {
    for (size_t i = 0; i < dc.res_areas.size(); i++)
      if (!dc.res_areas[i].busy) return int(i);
    return -1;
  };
  if (free_area() < 0)
    res_wait_unlocked(dc, lk, [&] { return free_area() >= 0; }, "resident search: no result area freed (5 s)");
  const int ai = free_area();
  DeviceCtx::ResArea &area = dc.res_areas[size_t(ai)];
  area.busy = true;
  area.sym = sym;
  area.W = W;
  struct AreaRelease {  // (the area and the in-flight entry go back on every exit; under dc.mu)
    DeviceCtx &dc;
    DeviceCtx::ResArea &area;
    std::unique_lock<std::mutex> &lk;
    uint32_t seq = 0;
    bool posted = false;
    ~AreaRelease() {
      if (!lk.owns_lock()) lk.lock();
      if (posted) dc.res_inflight.erase(seq);
      area.busy = false;
    }
  } rel{dc, area, lk};
  // the live launch must serve this shape from the next sequence number: another shape, new
  // block memory, or a launch that left, and no query of another caller still in flight ->
  // quit / launch; queries in flight are served first (a quit is posted behind them)
  for (;;) {
    const bool dead = dc.res_alive && aql_done(dc.aql);
    if (dc.res_alive && !dead && dc.res_kernel == sym && dc.res_groups == W && dc.res_epoch == dc.mem_epoch) break;
    if (dc.res_inflight.empty()) {
      resident_quit(dc);
      if (!resident_launch(dc, sym, threads, W, dc.res_seq + 1)) return -1;
      break;
    }
    res_wait_unlocked(dc, lk, [&] { return dc.res_inflight.empty(); }, "resident search: queries in flight never completed (5 s)");
  }
  const auto &parts = used_parts(PA.nsegs, PA.nbms);
  hipEvent_t e0, e1;
  const bool timed = (flags & TSG_SEARCH_TIME_DEFER) && dc.defer_slot(e0, e1);
  const size_t tslot = timed ? dc.tring_used - 1 : 0;
  // workgroup stamps: timed queries, and every 16th query for the XCD split (the first 8 all)
  // full workgroup stamps only for the diagnostics that read them per workgroup (a timed query's
  // span comes from the count lines: each carries its workgroup's seen / end stamps' low 32 bits)
  static const bool dump_stamps = std::getenv("TSG_RES_DUMP") != nullptr;
  const bool stamp = (timed && dump_stamps) || (debug_xsplit() && (dc.res_xsamples < 8 || dc.res_qn % 16 == 0));
  dc.res_qn++;
  const uint32_t cs = kResCountStride;
  const size_t hdr = 256, cntb = align_up(size_t(W) * 4 * cs, 256), stb = align_up(size_t(W) * 8 * kResStampStride, 256);
  uint32_t *counts = nullptr;
  unsigned long long *qst = nullptr;
  const uint8_t *recs = nullptr;
  auto post = [&] {
    PA.seg_cap = dc.pool_seg;
    area.buf.ensure(res_area_bytes(W, PA.seg_cap));
    uint8_t *base = static_cast<uint8_t *>(area.buf.p);
    counts = reinterpret_cast<uint32_t *>(base + hdr);
    qst = reinterpret_cast<unsigned long long *>(base + hdr + cntb);
    recs = base + hdr + cntb + stb;
    PA.counts = counts;
    PA.recs = base + hdr + cntb + stb;
    PA.err = reinterpret_cast<uint32_t *>(base);
    PA.qstamps = stamp ? qst : nullptr;
    PA.cstride = cs;
    for (uint32_t w = 0; w < W; w++) counts[size_t(w) * cs] = kCountPending;
    if (stamp)  // (the stamps land after the counts: 0 = not yet)
      for (uint32_t x = 0; x < W; x++) qst[size_t(x) * kResStampStride] = qst[size_t(x) * kResStampStride + 1] = 0;
    if (rel.posted) dc.res_inflight.erase(rel.seq);
    rel.seq = ++dc.res_seq;
    rel.posted = true;
    dc.res_inflight[rel.seq] = uint32_t(ai);
    res_post(dc, rel.seq, kResSearch, &PA, &parts);
    dc.res_queries++;
    if (tf) dc.tf_queries++;
  };
  // every workgroup's count (stored after its records), with dc.mu released; a launch that ended
  // first (it left on an idle timeout just as this query was posted) is launched again from the
  // oldest query not served (res_relaunch_inflight)
  auto wait = [&] {
    const auto t0 = std::chrono::steady_clock::now();
    const bool prof = prof_on();
    thread_local std::vector<uint8_t> seen;
    seen.assign(W, 0);
    uint32_t lo = 0, nseen = 0;
    const uint32_t seg = PA.seg_cap;
    static const bool prefetch = DeviceCtx::env_u32("TSG_RES_PREFETCH", 1, 0, 1) != 0;
    lk.unlock();
    for (uint32_t it = 1;; it++) {
      // counts not seen yet; a finished workgroup's records are pulled into this core's
      // caches while the others still run (the copy after the wait then hits them)
      for (uint32_t w = lo; w < W; w++) {
        if (seen[w]) {
          if (w == lo) lo++;
          continue;
        }
        const uint32_t c = __atomic_load_n(counts + size_t(w) * cs, __ATOMIC_ACQUIRE);
        if (c == kCountPending) continue;
        seen[w] = 1;
        if (prof && nseen == 0)
          prof_add("res.first_count", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        nseen++;
        if (w == lo) lo++;
        if (prefetch) {
          const uint8_t *p0 = recs + uint64_t(w) * seg * sizeof(MatchRec);
          for (uint64_t o = 0; o < uint64_t(std::min(c, seg)) * sizeof(MatchRec); o += 64) __builtin_prefetch(p0 + o);
          if (stamp) __builtin_prefetch(qst + uint64_t(w) * kResStampStride);  // (a timed query's stamps)
        }
      }
      if (lo == W) {
        if (prof)
          prof_add("res.last_count", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        if (stamp) {  // a timed query's stamps, stored after each workgroup's count (bounded: a missing one reads 0)
          const auto ts = std::chrono::steady_clock::now();
          for (uint32_t x = 0; x < W; x++)
            while ((__atomic_load_n(qst + size_t(x) * kResStampStride, __ATOMIC_ACQUIRE) == 0 ||
                    __atomic_load_n(qst + size_t(x) * kResStampStride + 1, __ATOMIC_ACQUIRE) == 0) &&
                   std::chrono::steady_clock::now() - ts < std::chrono::milliseconds(2))
              __builtin_ia32_pause();
        }
        lk.lock();
        return;
      }
      if ((it & 0xfffffu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
        lk.lock();
        fail(TSG_E_DEVICE, "resident search: no answer in 5 s");
      }
      if ((it & 255u) == 0) {
        lk.lock();
        if (__atomic_load_n(static_cast<uint32_t *>(dc.res_host.p), __ATOMIC_ACQUIRE))
          fail(TSG_E_DEVICE, "resident search: a mailbox slot never verified");
        res_relaunch_inflight(dc);
        lk.unlock();
      }
      __builtin_ia32_pause();
    }
  };
  auto scan = [&](uint64_t &total, uint32_t &maxc) {
    total = 0;
    maxc = 0;
    for (uint32_t w = 0; w < W; w++) {
      total += counts[size_t(w) * cs];
      maxc = std::max(maxc, counts[size_t(w) * cs]);
    }
  };
  uint64_t total = 0;
  uint32_t maxc = 0, reruns = 0;
  try {
    tr.mark("plan");
    post();
    tr.mark("search");
    wait();
    tr.mark("sync");
    scan(total, maxc);
    // a workgroup's records exceed its host segment: a larger segment and the query again; more
    // than its LDS regions hold: the other paths
    SegFit fit;
    while ((fit = seg_fit(dc, q, maxc, PA.seg_cap, rec_cap)) == SegFit::grow) {
      post();
      wait();
      reruns++;
      scan(total, maxc);
    }
    if (fit == SegFit::dense) return 0;
  } catch (...) {
    //  the launch may still write into this area: it is set aside until shutdown, the
    // launch is ended (bounded) and the next query starts a new one
    if (!lk.owns_lock()) lk.lock();
    dc.res_quarantine.push_back(area.buf);
    area.buf = DeviceCtx::ResArea().buf;
    try {
      resident_quit(dc);
    } catch (...) {
    }
    dc.res_alive = false;
    throw;
  }
  if (const uint32_t rj = __atomic_exchange_n(static_cast<uint32_t *>(dc.res_host.p) + kResRejectWord, 0u, __ATOMIC_ACQ_REL))
    dc.res_rejects += rj;
  if (stamp) {
    if (debug_xsplit()) res_calibrate(dc, qst, PA, U, W);
  }
  if (timed) {  // the query's span on the device: first workgroup to see it .. last to finish
    // (from the count lines: the stamps' low 32 bits, 100 MHz: relative to workgroup 0's seen)
    const uint32_t ref = counts[1];
    int64_t dlo = INT64_MAX, dhi = INT64_MIN;
    for (uint32_t w = 0; w < W; w++) {
      dlo = std::min<int64_t>(dlo, int32_t(counts[size_t(w) * cs + 1] - ref));
      dhi = std::max<int64_t>(dhi, int32_t(counts[size_t(w) * cs + 2] - ref));
    }
    const unsigned long long span = dhi > dlo ? uint64_t(dhi - dlo) : 0;
    static const bool dump = std::getenv("TSG_RES_DUMP") != nullptr;
    if (dump) {  // spread of the workgroups' {seen, end} stamps (us after the first seen)
      unsigned long long lo = ~0ull;  // (the full stamps' first seen)
      for (uint32_t w = 0; w < W; w++) lo = std::min(lo, qst[size_t(w) * kResStampStride]);
      std::vector<double> sn(W), en(W);
      for (uint32_t w = 0; w < W; w++) {
        sn[w] = double(qst[size_t(w) * kResStampStride] - lo) / 100.0;
        en[w] = double(qst[size_t(w) * kResStampStride + 1] - lo) / 100.0;
      }
      static const bool raw = std::getenv("TSG_RES_DUMP")[0] == '2';
      if (raw) {  // every workgroup's end (0.01 us after the first seen), workgroup order
        std::string line = "[tsg] resident xsplit:";
        for (int x = 0; x < 8; x++) line += " " + std::to_string(PA.xsplit ? dc.res_xf[x] : 0.125);
        line += "\n[tsg] resident runs:";
        for (uint32_t w = 0; w < W; w++)
          line += " " + std::to_string(PA.xsplit ? PA.xn[w & 7] + ((w >> 3) < PA.xr[w & 7] ? 1u : 0u) : PA.wq + (w < PA.wr ? 1u : 0u));
        line += "\n[tsg] resident seen:";
        for (uint32_t w = 0; w < W; w++) line += " " + std::to_string(qst[size_t(w) * kResStampStride] - lo);
        line += "\n[tsg] resident ends:";
        for (uint32_t w = 0; w < W; w++) line += " " + std::to_string(qst[size_t(w) * kResStampStride + 1] - lo);
        line += "\n[tsg] resident counts:";
        for (uint32_t w = 0; w < W; w++) line += " " + std::to_string(counts[size_t(w) * cs]);
        std::fprintf(stderr, "%s\n", line.c_str());
      }
      std::sort(sn.begin(), sn.end());
      std::sort(en.begin(), en.end());
      std::fprintf(stderr, "[tsg] resident stamps us: seen p50 %.2f p90 %.2f max %.2f | end min %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f\n",
                   sn[W / 2], sn[W * 9 / 10], sn[W - 1], en[0], en[W / 10], en[W / 2], en[W * 9 / 10], en[W - 1]);
    }
    if (dc.tring_res.size() < dc.tring_used) dc.tring_res.resize(dc.tring_used);
    dc.tring_aql[tslot] = -3;
    dc.tring_res[tslot] = span * 10ull;  // (100 MHz ticks)
  }
  out.kernel_ns = out.scan_ns = 0;
  out.reruns = reruns;
  out.resident = true;
  tr.mark("events");
  // records: the segments in workgroup order are the reference order (static runs, each
  // wave's matches in scan order); a limit keeps each block part's first L
  const uint32_t seg = PA.seg_cap;
  const auto *prec = reinterpret_cast<const SearchOut::Rec *>(recs);
  finish_records(out, block_slots(segs), segs, blocks, limit, total, W, has_dur, q.has_range != 0, tf, [&](auto &&f) {
    for (uint32_t w = 0; w < W; w++) {
      const SearchOut::Rec *r = prec + uint64_t(w) * seg;
      for (uint32_t i = 0, c = counts[size_t(w) * cs]; i < c; i++) f(r[i]);
    }
  });
  tr.mark("post");
  return 1;
}

// Terms first or not for this launch (terms_first.hpp): the shapes without the instance never;
// "terms_first" 0 / 1 as told; auto from the blocks' per-set counts and the terms' bitmaps, off
// when a block has no counts, and off for a launch of fewer than kTermsFirstMinUnits units per
// workgroup (a limit query's first waves, a small block): with its 12 or 16 waves a workgroup then
// holds at most a unit per wave, the launch's time is latencies in a row and not bytes, and the
// gated load adds one more behind the term columns' (the crossover was measured on 76 units per
// workgroup; the limit-20 leg, 2 units per workgroup, was 0.3 us slower with the mode on).
constexpr uint32_t kTermsFirstMinUnits = 8;
static bool terms_first_choice(const tsg_query &q, bool has_dur, const std::vector<ScanSeg> &segs,
                               const std::vector<NarrowSeg> &nsegv, const std::vector<std::array<uint32_t, 8>> &nbms,
                               const std::vector<std::array<uint8_t, kArgTerms>> &nbmi, uint32_t U, uint32_t W) {
  if (!terms_first_shape(q.nterms, has_dur, q.has_range != 0)) return false;
  const int mode = g_terms_first.load(std::memory_order_relaxed);
  if (mode != 2) return mode == 1;
  if (uint64_t(U) < uint64_t(kTermsFirstMinUnits) * W) return false;
  thread_local std::vector<TermsFirstBlock> tb;
  tb.assign(segs.size(), TermsFirstBlock{});
  for (size_t i = 0; i < segs.size(); i++) {
    TermsFirstBlock &b = tb[i];
    b.entries = nsegv[i].nall;
    b.scanned = segs[i].n - segs[i].e0;
    b.nterms = std::min<uint32_t>(q.nterms, 4);
    for (uint32_t t = 0; t < b.nterms; t++) {
      const std::vector<uint32_t> *c = nsegv[i].cnt[t];
      b.counts[t] = c ? c->data() : nullptr;
      b.ncounts[t] = c ? uint32_t(c->size()) : 0u;
      b.bitmap[t] = nbms[nbmi[i][t]].data();
    }
  }
  return terms_first_pick(2, terms_first_p(tb.data(), tb.size()));
}

// One search_pool_kernel launch for a narrow search (every block scanned whole; a limit
// cuts each block's records to its first `cap` on the host). Returns false, with
// nothing written to `out`, when a workgroup found more matches than its record buffer
// holds: the caller then runs the segment / look-back path.
bool pool_search(DeviceCtx &dc, const std::vector<std::pair<uint32_t, Block *>> &blocks, const tsg_query &q,
                 uint32_t limit, uint32_t flags, const std::vector<ScanSeg> &segs, const std::vector<NarrowSeg> &nsegv,
                 const std::vector<std::array<uint32_t, 8>> &nbms,
                 const std::vector<std::array<uint8_t, kArgTerms>> &nbmi,
                 const std::vector<const DevBlockDesc *> &seg_desc, bool has_dur, Tracer &tr, SearchOut &out,
                 std::unique_lock<std::mutex> &lk) {
  hipStream_t s = dc.stream;
  const uint32_t nsegs = uint32_t(segs.size()), W = uint32_t(dc.num_cu);
  PoolArgs PA;
  std::memset(&PA, 0, sizeof PA);
  // limit L: each block's part needs its first L records only (ids are unique within a
  // block: the consumer takes at most L from it), so units keep their first L (parts start
  // on unit boundaries)
  PA.unit_cap = limit;
  for (const auto &sg : segs)
    if (sg.e0 % kPoolTile) PA.unit_cap = 0;
  uint32_t U = 0;
  for (uint32_t i = 0; i < nsegs; i++) {
    PoolBlk &b = PA.blk[i];
    const NarrowSeg &ns = nsegv[i];
    b.scan = ns.scan;
    for (uint32_t t = 0; t < q.nterms; t++) {
      b.col[t] = ns.ncol + uint64_t(ns.slot[t]) * ns.npad;
      b.bmi4 |= uint32_t(nbmi[i][t]) << (8 * t);
      b.nsets4 |= uint32_t(ns.nsets[t]) << (8 * t);
      PA.bm_ns[nbmi[i][t]] = ns.nsets[t];  // (a slot is one (dictionary, term) pair: its blocks agree)
    }
    b.npad = ns.npad;
    b.nent = uint32_t(segs[i].n);
    b.ubase = U;
    b.block_idx = segs[i].block_idx;
    PA.desc[i] = seg_desc[i];
    PA.ubase[i] = U;
    PA.ebase[i] = uint32_t(segs[i].e0);  // (a multiple of kPoolTile)
    PA.sbase[i] = ns.sbase;
    const uint64_t u = (segs[i].n - segs[i].e0 + kPoolTile - 1) / kPoolTile;
    if (uint64_t(U) + u >= (1ull << 31)) return false;
    U += uint32_t(u);
  }
  PA.ubase[nsegs] = U;
  bool tf = terms_first_choice(q, has_dur, segs, nsegv, nbms, nbmi, U, W);
  // A live resident launch of this shape's other instance: leaving it costs a quit and a launch,
  // far more than the mode saves a query, and queries of both kinds may alternate (a batch of
  // different conjunctions). Off is taken at once (a block without counts, an unselective
  // conjunction: the default instance is never wrong by much); terms first only once
  // kTermsFirstSwitch queries in a row have asked for it. Forced modes are obeyed as they are.
  if (g_terms_first.load(std::memory_order_relaxed) == 2 && terms_first_shape(q.nterms, has_dur, q.has_range != 0)) {
    constexpr uint32_t kTermsFirstSwitch = 8;
    const bool live_off = dc.res_alive && dc.res_kernel == kernel_symbol(Kernel::resident, q.nterms, has_dur, q.has_range, dc.pool_nt, false);
    if (!tf) dc.tf_streak = 0;
    else if (live_off && ++dc.tf_streak < kTermsFirstSwitch) tf = false;
  }
  for (size_t j = 0; j < nbms.size(); j++)
    for (int x = 0; x < 8; x++) PA.bms[j][x] = nbms[j][size_t(x)];
  // static runs: (100 - dyn)% of the units split evenly; the rest in dynamic chunks
  uint32_t S = uint32_t(uint64_t(U) * (100 - dc.pool_dyn_pct) / 100 / W);
  // small searches (a limit query's first wave, one block): every unit static. Their
  // refill triggers would all fall in the first two claim rounds, and chunks are
  // requested strictly in order: a chain of device-counter round trips
  if (S < dc.pool_small) S = uint32_t((uint64_t(U) + W - 1) / W);
  // units per dynamic claim: TSG_POOL_CHUNK (16), at most half a workgroup's static run
  uint32_t cs = dc.pool_chunk_shift;
  while (cs > 0 && (1u << cs) > std::max(1u, S / 2)) cs--;
  const uint32_t dyn_units = U > S * W ? U - S * W : 0u;
  while (((dyn_units + (1u << cs) - 1) >> cs) + 64 > kPoolChunks) cs++;
  PA.nsegs = nsegs;
  PA.units = U;
  PA.static_per_wg = S;
  PA.dyn0 = S * W;
  PA.chunk_shift = cs;
  PA.lookahead = std::min(dc.pool_lookahead, S);
  PA.has_min = q.has_min;
  PA.has_max = q.has_max;
  // duration bounds in the ds column's units (2 x whole ms + a remainder bit: devctx.hip):
  // dur >= m ms <=> ds >= 2m, dur <= M ms <=> ds <= 2M (callers: m, M <= kDs16MaxMs)
  PA.min32 = q.has_min ? uint32_t(2 * (q.min_ns / 1000000ull)) : 0u;
  PA.max32 = q.has_max ? uint32_t(2 * (q.max_ns / 1000000ull)) : 0u;
  PA.start_s = q.start_s;
  PA.end_s = q.end_s;
  // the LDS record buffer (kPoolLds); the host segments are smaller (seg_fit)
  const uint32_t rec_cap = std::min(dc.pool_rec, uint32_t(kPoolLds / sizeof(MatchRec)));
  if (uint64_t(W) * rec_cap > (1u << 20)) return false;  // (record slots are 20-bit in the host's sort keys)
  PA.rec_cap = rec_cap;
  const size_t hdr = 256, cntb = align_up(size_t(W) * 4, 256);
  if (dc.pool_head.ensure(256)) {  // then self-resetting
    HIP_OK(hipMemsetAsync(dc.pool_head.p, 0, dc.pool_head.cap, s));
    HIP_OK(hipStreamSynchronize(s));  // (launches may go to the AQL queue, which does not follow this stream)
  }
  if (!dc.aql_tried) {
    dc.aql_tried = true;
    dc.aql = aql_open(dc.ordinal);
  }
  unsigned *heads = static_cast<unsigned *>(dc.pool_head.p);
  static const bool want_stamps = std::getenv("TSG_STAMPS") != nullptr;
  if (want_stamps) {
    dc.stamps.ensure(size_t(W) * kStampSlots * 8);
    HIP_OK(hipMemsetAsync(dc.stamps.p, 0, size_t(W) * kStampSlots * 8, s));
    PA.stamps = static_cast<unsigned long long *>(dc.stamps.p);
  }
  const bool use_static = uint64_t(U) < uint64_t(dc.pool_static_units) * W;
  const Kernel kind = use_static ? Kernel::stat : Kernel::pool;
  const PoolFn fn = pool_fn(kind, q.nterms, has_dur, q.has_range, dc.pool_nt, tf);
  if (!dc.pool_attr.count(reinterpret_cast<const void *>(fn))) {
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                               int(kPoolLds)));
    dc.pool_attr.insert(reinterpret_cast<const void *>(fn));
  }
  const uint32_t threads = 64 * dc.pool_waves;
  PA.nthreads = threads;
  PA.ngroups = W;
  PA.sq = U / (W * (threads / 64));
  PA.sr = U % (W * (threads / 64));
  PA.nbms = uint32_t(nbms.size());
  PA.wq = U / W;
  PA.wr = U % W;
  const bool time_all = flags & TSG_SEARCH_TIME_ALL, time_scan = flags & (TSG_SEARCH_TIME_SCAN | TSG_SEARCH_TIME_ALL);
  // the resident kernel serves the query when it can (the only context on the device, no
  // per-call HIP events or stamps asked for); otherwise the queue and the CUs are freed first
  // (and no other process has a context on the GPU: cotenant_others)
  if (dc.res_on && dc.aql && !want_stamps && !time_scan && (U + W - 1) / W <= kResMaxUnits &&
      contexts_on(dc.ordinal) == 1) {
    if (cotenant_others(dc) == 0) {
      const int r = resident_search(dc, lk, PA, segs, blocks, q, limit, flags, has_dur, tf, kResThreads, W, rec_cap, tr, out);
      if (r >= 0) return r == 1;
    } else {
      dc.res_cotenant_queries++;
      out.path |= TSG_PATH_COTENANT;
    }
  }
  resident_quit(dc);
  dc.res_plain_queries++;
  hipEvent_t e0 = dc.es0, e1 = dc.es1;
  const bool defer = !time_scan && (flags & TSG_SEARCH_TIME_DEFER) && dc.defer_slot(e0, e1);
  uint32_t *counts = nullptr;
  const uint8_t *recs = nullptr;
  bool via_aql = false;  // the launch being waited for went to the AQL queue
  auto launch = [&](bool first) {
    PA.seg_cap = dc.pool_seg;
    dc.hres.ensure(hdr + cntb + size_t(W) * PA.seg_cap * sizeof(MatchRec));
    uint8_t *base = static_cast<uint8_t *>(dc.hres.p);
    counts = reinterpret_cast<uint32_t *>(base + hdr);
    recs = base + hdr + cntb;
    PA.counts = counts;
    PA.recs = base + hdr + cntb;
    PA.err = reinterpret_cast<uint32_t *>(base);
    *reinterpret_cast<volatile uint32_t *>(base) = 0;
    PA.head = heads + 32 * dc.pool_parity;
    PA.head_next = heads + 32 * (dc.pool_parity ^ 1u);
    std::fill_n(counts, W, kCountPending);  // (each workgroup stores its count last)
    if (first && time_all) HIP_OK(hipEventRecord(dc.ev0, s));
    // timing: the first launch on e0/e1 (scan time or a deferred pair), a rerun on er0/er1
    const bool timed = first ? (time_scan || defer) : time_scan;
    hipEvent_t t0 = first ? e0 : dc.er0, t1 = first ? e1 : dc.er1;
    AqlKernel ak;
    via_aql = false;
    // AQL for untimed launches and for deferred-timed first launches (timed by the queue's own
    // dispatch timestamps, as the untimed ones run); explicit per-call timing stays on HIP events
    const bool aql_timed = first && defer && !time_scan;
    if ((!timed || aql_timed) && !want_stamps && dc.aql)
      ak = aql_kernel(dc.aql, kernel_symbol(kind, q.nterms, has_dur, q.has_range, dc.pool_nt, tf).c_str(),
                      uint32_t(sizeof(PoolArgs)));
    if (ak.kobj) {
      // our own AQL packet (aql.hpp): only the argument words this launch's kernel reads
      const int ps = aql_dispatch(dc.aql, ak, W, threads, uint32_t(kPoolLds), &PA, used_parts(nsegs, PA.nbms), aql_timed);
      if (aql_timed) dc.tring_aql[dc.tring_used - 1] = ps >= 0 ? ps : -2;  // (the slot defer_slot took; -2: untimed)
      via_aql = true;
    } else if (timed && dc.ext_events) {  // stamped from the dispatch packet itself
      void *kargs[] = {&PA};
      HIP_OK(hipExtLaunchKernel(reinterpret_cast<const void *>(fn), dim3(W), dim3(threads), kargs, kPoolLds, s, t0,
                                t1, 0));
    } else {
      if (timed) HIP_OK(hipEventRecord(t0, s));
      fn<<<W, threads, kPoolLds, s>>>(PA);
      HIP_OK(hipGetLastError());
      if (timed) HIP_OK(hipEventRecord(t1, s));
    }
    if (first && time_all) HIP_OK(hipEventRecord(dc.ev1, s));
    if (!use_static) dc.pool_parity ^= 1u;  // (the static kernel claims nothing)
    if (tf) dc.tf_queries++;
  };
  // completion: every workgroup's count (stored after its records completed, read with
  // acquire loads); finished segments are pulled into this core's caches meanwhile; the
  // stream is queried now and then so that a kernel that dies fails the search
  auto wait = [&] {
    thread_local std::vector<uint8_t> seen;
    seen.assign(W, 0);
    const uint32_t seg = PA.seg_cap;
    uint32_t lo = 0;
    for (uint32_t it = 1; lo < W; it++) {
      for (uint32_t w = lo; w < W; w++) {
        if (seen[w]) {
          if (w == lo) lo++;
          continue;
        }
        const uint32_t c = __atomic_load_n(counts + w, __ATOMIC_ACQUIRE);
        if (c == kCountPending) continue;
        seen[w] = 1;
        if (w == lo) lo++;
        const uint8_t *p0 = recs + uint64_t(w) * seg * sizeof(MatchRec);
        for (uint64_t o = 0; o < uint64_t(std::min(c, seg)) * sizeof(MatchRec); o += 64) __builtin_prefetch(p0 + o);
      }
      if (lo == W) break;
      if ((it & 255u) == 0) {
        const hipError_t e = via_aql ? (aql_done(dc.aql) ? hipSuccess : hipErrorNotReady) : hipStreamQuery(s);
        if (e == hipSuccess) {
          bool all = true;
          for (uint32_t w = 0; w < W && all; w++) all = __atomic_load_n(counts + w, __ATOMIC_ACQUIRE) != kCountPending;
          if (all) break;
          fail(TSG_E_DEVICE, "pool search kernel completed without storing every workgroup count");
        }
        if (e != hipErrorNotReady) HIP_OK(e);
      }
      __builtin_ia32_pause();
    }
  };
  auto scan_counts = [&](uint64_t &total, uint32_t &maxc) {
    if (__atomic_load_n(PA.err, __ATOMIC_ACQUIRE))
      fail(TSG_E_DEVICE, "pool search: a workgroup's chunk poll ran past its bound (claim protocol broken)");
    total = 0;
    maxc = 0;
    for (uint32_t w = 0; w < W; w++) {
      total += counts[w];
      maxc = std::max(maxc, counts[w]);
    }
  };
  tr.mark("plan");
  launch(true);
  tr.mark("search");
  wait();
  tr.mark("sync");
  if (want_stamps) print_stamps(dc, W, true);
  uint64_t total = 0;
  uint32_t maxc = 0;
  scan_counts(total, maxc);
  // A workgroup's count depends on which dynamic chunks it won, so a rerun can overflow
  // where the first launch did not: launch until every count fits its segment (segments
  // double each time, at most up to the LDS buffer), or leave for the other paths.
  uint32_t reruns = 0;
  float rerun_ms = 0;
  for (SegFit fit; (fit = seg_fit(dc, q, maxc, PA.seg_cap, rec_cap)) != SegFit::fits;) {
    if (fit == SegFit::dense) return false;
    // a rerun produces the records: its time counts too
    launch(false);
    wait();
    if (time_scan) {
      float ms = 0;
      HIP_OK(hipEventSynchronize(dc.er1));
      HIP_OK(hipEventElapsedTime(&ms, dc.er0, dc.er1));
      rerun_ms += ms;
    }
    reruns++;
    scan_counts(total, maxc);
  }
  const uint32_t seg = PA.seg_cap;
  float ms = 0, sms = 0;
  if (time_all) {
    HIP_OK(hipEventSynchronize(dc.ev1));
    HIP_OK(hipEventElapsedTime(&ms, dc.ev0, dc.ev1));
  }
  if (time_scan) {
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(&sms, e0, e1));
  }
  out.kernel_ns = uint64_t(double(ms + (time_all ? rerun_ms : 0.f)) * 1e6);
  out.scan_ns = uint64_t(double(sms + rerun_ms) * 1e6);
  out.reruns = reruns;
  tr.mark("events");
  // records: the blocks' order in the launch, the entry index within a block (the
  // reference scan order) = the record's position in the launch's unit space. Ordered
  // by one bucket pass over that position (about one record per bucket) and an
  // insertion fix-up; a crowded bucket is sorted on its own.
  const std::vector<uint32_t> &pos = block_slots(segs);
  thread_local std::vector<uint32_t> bucket;
  thread_local std::vector<uint64_t> keys, sorted;
  keys.resize(total);
  sorted.resize(total);
  // keys straight from the pinned segments: position << 20 | record slot (w * seg + i);
  // the gather below reads the same lines again, from cache
  const auto *prec = reinterpret_cast<const SearchOut::Rec *>(recs);
  const uint64_t span = uint64_t(U) * kPoolTile;  // positions < span <= 2^31 * 512
  uint32_t lb = 6;
  while ((1ull << lb) < total && lb < 20) lb++;
  uint32_t sb = 0;
  while (((span - 1) >> sb) >= (1ull << lb)) sb++;  // bucket of the largest position < 2^lb
  bucket.assign((size_t(1) << lb) + 1, 0);
  uint64_t nrec = 0;
  for (uint32_t w = 0; w < W; w++)
    for (uint32_t i = 0; i < counts[w]; i++) {
      const uint64_t slot = uint64_t(w) * seg + i;  // (< 256 x 2048 < 2^20)
      const SearchOut::Rec &r = prec[slot];
      const uint32_t ps = slot_of(pos, r);
      const uint64_t at = uint64_t(PA.blk[ps].ubase) * kPoolTile + (r.entry - PA.ebase[ps]);
      keys[nrec++] = (at << 20) | slot;
      bucket[size_t(at >> sb) + 1]++;  // (bucket counts in the same pass)
    }
  tr.mark("post.keys");
  for (size_t b = 1; b < bucket.size(); b++) bucket[b] += bucket[b - 1];
  for (uint64_t i = 0; i < total; i++) sorted[bucket[size_t((keys[i] >> 20) >> sb)]++] = keys[i];
  // (bucket[b] is now the end of bucket b)
  for (size_t b = 0, lo = 0; b + 1 < bucket.size(); lo = bucket[b], b++) {
    const size_t hi = bucket[b];
    if (hi - lo <= 1) continue;
    if (hi - lo > 32) {
      std::sort(sorted.begin() + lo, sorted.begin() + hi);
      continue;
    }
    for (size_t i = lo + 1; i < hi; i++) {
      const uint64_t k = sorted[i];
      size_t j = i;
      while (j > lo && sorted[j - 1] > k) {
        sorted[j] = sorted[j - 1];
        j--;
      }
      sorted[j] = k;
    }
  }
  // (the sorted records of a block are contiguous)
  tr.mark("post.sort");
  finish_records(out, pos, segs, blocks, limit, total, W, has_dur, q.has_range != 0, tf, [&](auto &&f) {
    for (uint64_t i = 0; i < total; i++) f(prec[sorted[i] & 0xfffffu]);
  });
  tr.mark("post");
  return true;
}

}  // namespace tsg
