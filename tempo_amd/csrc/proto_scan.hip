// proto_scan.hip — proto-object backend search on the device.
//
// proto_scan_kernel evaluates, for every object of the searched page range, what
// ObjectDecoder.Matches + trace.MatchesProto decide for it (pkg/model/v2/object_decoder.go:57-89,
// pkg/model/v1/object_decoder.go, pkg/model/trace/matches.go:33-116), over the columns the
// loader built (proto.cpp): one lane per object, one 64-object ballot per wave, two bits
// per object (match, error) written as 64-bit words. The host then replays
// BackendBlock.Search's loop (tempodb/encoding/v2/backend_block.go:185-202, :211-231) over
// those bits: metrics per object, MaxBytes skips, the first error, the limit break, and
// the paged iterator's chunked page reads (iterator_paged.go:62-131).
//
// proto_scan_batch_kernel does the same for many (block, request) jobs in one launch
// (tsg_proto_search_batch): the jobs lie in a table in device memory, each takes
// ceil(objects / 256) workgroups, and a workgroup finds its job by a binary search over the
// jobs' first workgroups. Both kernels call one per-object decision (proto_decide). Per
// device the batch costs one lock hold, one H2D copy (job table + every job's term bitmaps,
// from pinned memory), one launch, one D2H copy (into pinned memory) and one synchronise. A
// launch covers at most 4096 jobs (kPBatchJobs); a larger batch runs as consecutive launches.
//
// Bound: HBM, ~(24 + Σ term column width) B per object + term bitmaps (L2-resident).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>

#include "devctx.hpp"
#include "proto.hpp"

namespace tsg {

std::vector<uint32_t> proto_term_bitmap(const ProtoBlock &b, const std::string &key, std::string_view v, bool &present);
void proto_load_host(ProtoBlock &b, const std::string &dir);

constexpr int kPThreads = 256;
constexpr int kPTerms = 16;

struct PTerm {
  const uint8_t *col;     // value-set id per object (width bytes, all-ones = key absent); null = key not in block
  const uint32_t *bm;     // value-set bitmap of this term
  uint32_t width, pad;
};

// What the per-object decision reads: a block's columns, the objects [t0, t1) of the page
// range, the request scalars and the terms.
struct PScan {
  const uint32_t *fr_start, *fr_end, *st_sec, *en_sec, *dur_ms, *obj_len;
  const uint8_t *flags;
  uint32_t t0, t1, v2, nterms;
  uint32_t start, end, min_ms, max_ms, max_bytes, pad;
  PTerm terms[kPTerms];
};

struct PArgs {
  PScan s;
  unsigned long long *out;  // [2 * words]: match bits, then error bits (bit i = object t0 + i)
  uint32_t words, pad2;
};

// One job of a batched launch (proto_scan_batch_kernel), in device memory: the scan, the job's
// first workgroup of the launch, and where its [2 * words] output words start in the launch's
// output buffer.
struct PJob {
  PScan s;
  uint32_t wg0, words;
  unsigned long long out_word;
};

// Object i of scan A (i < A.t1): m = it matches, e = reading it is an error.
__device__ __forceinline__ void proto_decide(const PScan &A, uint32_t i, bool &m, bool &e) {
  const uint32_t len = A.obj_len[i];
  if (A.max_bytes && len > A.max_bytes) return;  // search(): SkippedTraces, no Matches
  const uint8_t fl = A.flags[i];
  bool pass = true;
  if (A.v2) {
    if (fl & PF_HDRBAD) {  // FastRange: stripStartEnd error
      e = true;
      pass = false;
    } else {
      const uint32_t s = A.fr_start[i], en = A.fr_end[i];
      if (!(A.start <= en && A.end >= s)) pass = false;
      const uint32_t d = en - s;  // (uint32 wrap, as the reference)
      if (A.max_ms && d > A.max_ms / 1000 + 1) pass = false;
      if (A.min_ms && d < A.min_ms / 1000) pass = false;
    }
  }
  if (pass && (fl & PF_BAD)) {  // PrepareForRead: proto.Unmarshal error
    e = true;
    pass = false;
  }
  if (!pass) return;
  for (uint32_t q = 0; q < A.nterms && pass; q++) {
    const PTerm &T = A.terms[q];
    if (!T.col) {
      pass = false;
      break;
    }
    uint32_t sid;
    if (T.width == 1) {
      sid = T.col[i];
      sid = sid == 0xffu ? 0xffffffffu : sid;
    } else if (T.width == 2) {
      sid = reinterpret_cast<const uint16_t *>(T.col)[i];
      sid = sid == 0xffffu ? 0xffffffffu : sid;
    } else {
      sid = reinterpret_cast<const uint32_t *>(T.col)[i];
    }
    pass = sid != 0xffffffffu && ((T.bm[sid >> 5] >> (sid & 31)) & 1u);
  }
  if (pass) {
    const uint32_t dms = A.dur_ms[i];
    if (A.max_ms && A.max_ms < dms) pass = false;
    if (A.min_ms && A.min_ms > dms) pass = false;
    if (!(A.start <= A.en_sec[i] && A.end >= A.st_sec[i])) pass = false;
  }
  m = pass;
}

__global__ void __launch_bounds__(kPThreads) proto_scan_kernel(PArgs A) {
  const uint32_t i = A.s.t0 + blockIdx.x * kPThreads + threadIdx.x;
  bool m = false, e = false;
  if (i < A.s.t1) proto_decide(A.s, i, m, e);
  const unsigned long long bm = __ballot(m), be = __ballot(e);
  const uint32_t w = (blockIdx.x * kPThreads + threadIdx.x) >> 6;
  if ((threadIdx.x & 63) == 0 && w < A.words) {
    A.out[w] = bm;
    A.out[A.words + w] = be;
  }
}

// Many (block, request) jobs in one launch. first[0..njobs] is the jobs' first-workgroup prefix
// (first[j] == jobs[j].wg0, first[njobs] = the grid; a job without objects takes no workgroup,
// so equal neighbours). A workgroup finds the job j with first[j] <= blockIdx.x < first[j + 1]
// by a binary search that is uniform across it, then does what proto_scan_kernel does for its
// 256 objects of that job. No atomics, no polling, nothing another workgroup writes is read.
__global__ void __launch_bounds__(kPThreads) proto_scan_batch_kernel(const PJob *__restrict__ jobs,
                                                                      const uint32_t *__restrict__ first, uint32_t njobs,
                                                                      unsigned long long *__restrict__ out) {
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0, hi = njobs;  // first[lo] <= b < first[hi]
  for (int it = 0; it < 32 && hi - lo > 1; it++) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= b) lo = mid;
    else hi = mid;
  }
  const PJob &J = jobs[lo];
  if (b < J.wg0) return;  // (a grid beyond the table: nothing to do)
  const uint32_t r = (b - J.wg0) * kPThreads + threadIdx.x;  // object of the job's range
  const uint32_t i = J.s.t0 + r;
  bool m = false, e = false;
  if (r < J.s.t1 - J.s.t0) proto_decide(J.s, i, m, e);
  const unsigned long long bm = __ballot(m), be = __ballot(e);
  const uint32_t w = r >> 6;
  if ((threadIdx.x & 63) == 0 && w < J.words) {
    out[J.out_word + w] = bm;
    out[J.out_word + J.words + w] = be;
  }
}

static void *palloc(ProtoBlock &b, size_t bytes) {
  void *p = nullptr;
  HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
  b.allocs.push_back(p);
  b.device_bytes += bytes;
  return p;
}

void proto_block_open(Ctx &c, ProtoBlock &b, const std::string &dir, int device_hint) {
  if (c.devs.empty()) fail(TSG_E_DEVICE, "no device");
  proto_load_host(b, dir);
  DeviceCtx &dc = *c.devs[size_t(std::max(device_hint, 0)) % c.devs.size()];
  b.dc = &dc;
  std::lock_guard<std::mutex> lk(dc.mu);
  HIP_OK(hipSetDevice(dc.ordinal));
  const size_t n = b.n;
  auto *u = static_cast<uint32_t *>(palloc(b, n * 6 * 4));
  const std::vector<uint32_t> *cols[6] = {&b.fr_start, &b.fr_end, &b.st_sec, &b.en_sec, &b.dur_ms, &b.obj_len};
  for (int k = 0; k < 6; k++)
    if (n) HIP_OK(hipMemcpy(u + k * n, cols[k]->data(), n * 4, hipMemcpyHostToDevice));
  b.d_u32 = u;
  auto *fl = static_cast<uint8_t *>(palloc(b, n));
  if (n) HIP_OK(hipMemcpy(fl, b.flags.data(), n, hipMemcpyHostToDevice));
  b.d_flags = fl;
  for (ProtoKey &K : b.keys) {
    auto *p = static_cast<uint8_t *>(palloc(b, K.col.size()));
    if (!K.col.empty()) HIP_OK(hipMemcpy(p, K.col.data(), K.col.size(), hipMemcpyHostToDevice));
    K.d_col = p;
    std::vector<uint8_t>().swap(K.col);
  }
}

void proto_block_free(ProtoBlock &b) {
  if (!b.dc) return;
  std::lock_guard<std::mutex> lk(b.dc->mu);
  (void)hipSetDevice(b.dc->ordinal);
  (void)hipStreamSynchronize(b.dc->stream);
  for (void *p : b.allocs) (void)hipFree(p);
  b.allocs.clear();
  b.dc = nullptr;
}

// The host-side preparation of one search: the objects [t0, t1) of the request's page range,
// the de-duplicated terms and their value-set bitmaps (bm_at[q] words into bmw; key_of[q] < 0:
// the key is in no object of the block).
struct PPlan {
  uint32_t start_page = 0, t0 = 0, t1 = 0, words = 0;
  uint64_t maxp = 0;
  uint32_t nterms = 0;
  std::vector<uint32_t> bmw;
  size_t bm_at[kPTerms] = {};
  int key_of[kPTerms] = {};
};

static void proto_plan(const ProtoBlock &b, const tsg_proto_request &req, PPlan &P) {
  if (!b.dc) fail(TSG_E_INVALID, "proto block not resident");
  if (req.ntags > kPTerms) fail(TSG_E_UNSUPPORTED, "more than 16 tags in one proto search");
  const uint32_t npages = uint32_t(b.page_len.size());
  // TotalPages > 0: partialIterator(StartPage, TotalPages); else Iterator() from page 0
  P.start_page = req.total_pages ? req.start_page : 0;
  P.maxp = req.total_pages ? uint64_t(P.start_page) + req.total_pages : ~0ULL;
  // objects of the searched page range (the kernel covers them; the host walk stops early)
  const uint32_t p0 = std::min(P.start_page, npages);
  const uint32_t p1 = uint32_t(std::min<uint64_t>(npages, P.maxp));
  P.t0 = b.page_first[p0];
  P.t1 = p1 > p0 ? b.page_first[p1] : P.t0;
  P.words = (P.t1 - P.t0 + 63) / 64;
  // query terms: map semantics (one value per key: the last one given wins)
  std::vector<std::pair<std::string, std::string>> tags;
  for (uint32_t q = 0; q < req.ntags; q++) {
    std::string k(req.keys[q], req.key_lens[q]), v(req.values[q], req.value_lens[q]);
    bool dup = false;
    for (auto &kv : tags)
      if (kv.first == k) {
        kv.second = v;
        dup = true;
      }
    if (!dup) tags.emplace_back(k, v);
  }
  P.nterms = uint32_t(tags.size());
  for (size_t q = 0; q < tags.size(); q++) {
    P.key_of[q] = -1;
    bool present;
    std::vector<uint32_t> bm = proto_term_bitmap(b, tags[q].first, tags[q].second, present);
    if (!present) continue;
    P.key_of[q] = int(b.key_index.at(tags[q].first));
    P.bm_at[q] = P.bmw.size();
    P.bmw.insert(P.bmw.end(), bm.begin(), bm.end());
  }
}

// The scan of a planned search; d_bm: where P.bmw lies (or will lie) in device memory.
static void proto_fill(PScan &A, const ProtoBlock &b, const tsg_proto_request &req, const PPlan &P,
                       const uint32_t *d_bm) {
  const size_t n = b.n;
  A.fr_start = b.d_u32;
  A.fr_end = b.d_u32 + n;
  A.st_sec = b.d_u32 + 2 * n;
  A.en_sec = b.d_u32 + 3 * n;
  A.dur_ms = b.d_u32 + 4 * n;
  A.obj_len = b.d_u32 + 5 * n;
  A.flags = b.d_flags;
  A.t0 = P.t0;
  A.t1 = P.t1;
  A.v2 = b.v2;
  A.nterms = P.nterms;
  A.start = req.start;
  A.end = req.end;
  A.min_ms = req.min_duration_ms;
  A.max_ms = req.max_duration_ms;
  A.max_bytes = req.max_bytes;
  for (uint32_t q = 0; q < P.nterms; q++) {
    if (P.key_of[q] < 0) continue;  // (col null: the key is in no object of the block)
    const ProtoKey &K = b.keys[size_t(P.key_of[q])];
    A.terms[q].col = K.d_col;
    A.terms[q].width = K.width;
    A.terms[q].bm = d_bm + P.bm_at[q];
  }
}

// BackendBlock.Search's loop over the paged iterator, from the scan's bit words
// (bits[0 .. words): match, bits[words .. 2 * words): error; bit r = object t0 + r)
static void proto_replay(const ProtoBlock &b, const tsg_proto_request &req, const PPlan &P,
                         const unsigned long long *bits, ProtoOut &out) {
  const uint32_t t0 = P.t0, words = P.words;
  const uint64_t maxp = P.maxp;
  const uint32_t chunk = req.chunk_size_bytes ? req.chunk_size_bytes : 1000000u;  // DefaultSearchOptions
  auto bit = [&](uint32_t i, int which) {
    const uint32_t r = i - t0;
    return (bits[size_t(which) * words + (r >> 6)] >> (r & 63)) & 1ULL;
  };
  auto fail_at = [&](int code, const std::string &m) {
    out.status = code;
    out.error = m;
    out.traces.clear();
  };
  const uint32_t limit = req.limit;
  uint64_t cur = P.start_page;
  for (;;) {
    if (cur >= maxp) return;                    // io.EOF
    auto at = [&](uint64_t r) -> int {          // indexReader.At: 1 record, 0 nil, -1 error
      if (r >= b.total_records) return 0;
      if (r >= b.index_err_at) return -1;
      return 1;
    };
    int a = at(cur);
    if (a < 0) return fail_at(TSG_E_CORRUPT, "error reading index record " + std::to_string(cur));
    if (a == 0) return;
    // gather a chunk: at least one record, then while it fits and is inside the range
    std::vector<uint32_t> chunk_pages;
    uint64_t length = 0;
    while (a > 0) {
      if ((length + b.page_len[cur] > chunk || cur >= maxp) && !chunk_pages.empty()) break;
      chunk_pages.push_back(uint32_t(cur));
      length += b.page_len[cur];
      cur++;
      a = at(cur);
      if (a < 0) return fail_at(TSG_E_CORRUPT, "error getting next record " + std::to_string(cur));
    }
    for (uint32_t p : chunk_pages)
      if (b.page_status[p] == PP_DECODE) return fail_at(TSG_E_CORRUPT, "error reading objects for records (page " + std::to_string(p) + ")");
    for (uint32_t p : chunk_pages) {
      for (uint32_t i = b.page_first[p]; i < b.page_first[p + 1]; i++) {
        out.inspected_traces++;
        out.inspected_bytes += b.obj_len[i];
        if (req.max_bytes && b.obj_len[i] > req.max_bytes) {
          out.skipped_traces++;
        } else if (bit(i, 1)) {
          return fail_at(TSG_E_CORRUPT, "object " + std::to_string(i) + ": trace decode failed");
        } else if (bit(i, 0)) {
          out.traces.push_back(i);
        }
        if (out.traces.size() >= limit) return;  // (limit 0: after the first object)
      }
      if (b.page_status[p] == PP_FRAMING)
        return fail_at(TSG_E_CORRUPT, "error unmarshalling active page " + std::to_string(p));
    }
  }
}

void proto_search(ProtoBlock &b, const tsg_proto_request &req, ProtoOut &out) {
  out = ProtoOut();
  PPlan P;
  proto_plan(b, req, P);
  const std::vector<uint32_t> &bmw = P.bmw;
  const uint32_t t0 = P.t0, t1 = P.t1, words = P.words;
  DeviceCtx &dc = *b.dc;
  std::vector<unsigned long long> bits;
  {
    std::lock_guard<std::mutex> lk(dc.mu);
    resident_quit(dc);  // (the resident search launch holds every CU's LDS)
    HIP_OK(hipSetDevice(dc.ordinal));
    hipStream_t s = dc.stream;
    if (t1 > t0) {
      dc.pbm.ensure(std::max<size_t>(bmw.size(), 1) * 4);
      dc.pout.ensure(size_t(words) * 16);
      if (!bmw.empty()) HIP_OK(hipMemcpyAsync(dc.pbm.p, bmw.data(), bmw.size() * 4, hipMemcpyHostToDevice, s));
      PArgs A{};
      proto_fill(A.s, b, req, P, static_cast<const uint32_t *>(dc.pbm.p));
      A.out = static_cast<unsigned long long *>(dc.pout.p);
      A.words = words;
      HIP_OK(hipEventRecord(dc.ev0, s));
      proto_scan_kernel<<<(t1 - t0 + kPThreads - 1) / kPThreads, kPThreads, 0, s>>>(A);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(dc.ev1, s));
      bits.resize(size_t(words) * 2);
      HIP_OK(hipMemcpyAsync(bits.data(), dc.pout.p, bits.size() * 8, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, dc.ev0, dc.ev1));
      out.kernel_ns = uint64_t(double(ms) * 1e6);
    }
  }
  proto_replay(b, req, P, bits.data(), out);
}

// ---- batched search -----------------------------------------------------------------------
// A launch serves at most kPBatchJobs jobs (and at most kPBatchGroups workgroups, so that the
// grid's thread count stays below 2^32); a larger batch runs as consecutive launches.
// "proto_batch_jobs" (tsg_debug_set) lowers the job cap for tests, 0 restores it.
constexpr uint32_t kPBatchJobs = 4096;
constexpr uint64_t kPBatchGroups = 1u << 23;
static std::atomic<uint32_t> g_batch_jobs{kPBatchJobs};
void proto_batch_cap(uint32_t k) { g_batch_jobs.store(k ? std::min(k, kPBatchJobs) : kPBatchJobs); }

static size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

// One launch for jobs [j0, j1) of a device's items: staging [PJob x nj | first x (nj + 1) | every
// job's term bitmaps] copied to dc.pjob in one piece, the kernel, the [2 * words] bit words of
// every job copied back in one piece, one synchronise. Caller holds dc.mu. Returns the pinned
// block of the bit words, bits[j] pointing at job j's (the replay runs after the lock is gone).
struct PPinned {
  void *p;
  size_t n;
  explicit PPinned(size_t bytes) : p(pinned_get(bytes)), n(bytes) {}
  PPinned(const PPinned &) = delete;
  ~PPinned() { pinned_put(p, n); }
};
static std::unique_ptr<PPinned> proto_batch_launch(DeviceCtx &dc, const ProtoItem *items, const size_t *idx,
                                                   const PPlan *plans, size_t j0, size_t j1, ProtoOut *outs,
                                                   const unsigned long long **bits) {
  const size_t nj = j1 - j0;
  const size_t first_at = up256(nj * sizeof(PJob)), bm_at = first_at + up256((nj + 1) * 4);
  size_t bm_words = 0, out_words = 0;
  for (size_t j = j0; j < j1; j++) {
    bm_words += plans[j].bmw.size();
    out_words += size_t(plans[j].words) * 2;
  }
  const size_t in_bytes = bm_at + bm_words * 4, out_bytes = out_words * 8;
  hipStream_t s = dc.stream;
  dc.pjob.ensure(in_bytes);
  dc.pout.ensure(std::max<size_t>(out_bytes, 16));
  PPinned hin(in_bytes);
  auto hout = std::make_unique<PPinned>(std::max<size_t>(out_bytes, 16));
  auto *base = static_cast<uint8_t *>(hin.p);
  std::memset(base, 0, bm_at);
  auto *jobs = reinterpret_cast<PJob *>(base);
  auto *first = reinterpret_cast<uint32_t *>(base + first_at);
  auto *bm = reinterpret_cast<uint32_t *>(base + bm_at);
  const auto *d_bm = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(dc.pjob.p) + bm_at);
  uint32_t wg = 0;
  size_t bw = 0, ow = 0;
  for (size_t j = j0; j < j1; j++) {
    const PPlan &P = plans[j];
    PJob &J = jobs[j - j0];
    proto_fill(J.s, *items[idx[j]].b, *items[idx[j]].req, P, d_bm + bw);
    if (!P.bmw.empty()) std::memcpy(bm + bw, P.bmw.data(), P.bmw.size() * 4);
    bw += P.bmw.size();
    J.wg0 = first[j - j0] = wg;
    J.words = P.words;
    J.out_word = ow;
    ow += size_t(P.words) * 2;
    wg += (P.t1 - P.t0 + kPThreads - 1) / kPThreads;
  }
  first[nj] = wg;
  uint64_t kernel_ns = 0;
  if (wg) {
    HIP_OK(hipMemcpyAsync(dc.pjob.p, hin.p, in_bytes, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(dc.ev0, s));
    proto_scan_batch_kernel<<<wg, kPThreads, 0, s>>>(static_cast<const PJob *>(dc.pjob.p),
                                                     reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(dc.pjob.p) + first_at),
                                                     uint32_t(nj), static_cast<unsigned long long *>(dc.pout.p));
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(dc.ev1, s));
    HIP_OK(hipMemcpyAsync(hout->p, dc.pout.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, dc.ev0, dc.ev1));
    kernel_ns = uint64_t(double(ms) * 1e6);
  }
  for (size_t j = j0; j < j1; j++) {
    outs[idx[j]].kernel_ns = plans[j].t1 > plans[j].t0 ? kernel_ns : 0;
    bits[j] = static_cast<const unsigned long long *>(hout->p) + jobs[j - j0].out_word;
  }
  return hout;
}

void proto_search_batch(Ctx &c, const ProtoItem *items, size_t n, ProtoOut *outs) {
  for (size_t i = 0; i < n; i++) outs[i] = ProtoOut();
  // the items' devices, the context's first and in its order
  std::vector<DeviceCtx *> devs(c.devs.begin(), c.devs.end());
  for (size_t i = 0; i < n; i++)
    if (items[i].b->dc && std::find(devs.begin(), devs.end(), items[i].b->dc) == devs.end()) devs.push_back(items[i].b->dc);
  auto failed = [&](size_t i, int code, const std::string &m) {
    outs[i] = ProtoOut();
    outs[i].status = code;
    outs[i].error = m;
  };
  for (size_t i = 0; i < n; i++)
    if (!items[i].b->dc) failed(i, TSG_E_INVALID, "proto block not resident");
  for (DeviceCtx *dc : devs) {
    std::vector<size_t> idx;   // the device's items that planned
    std::vector<PPlan> plans;
    for (size_t i = 0; i < n; i++) {
      if (items[i].b->dc != dc) continue;
      PPlan P;
      try {
        proto_plan(*items[i].b, *items[i].req, P);
      } catch (const Error &e) {
        failed(i, e.code, e.what());
        continue;
      }
      idx.push_back(i);
      plans.push_back(std::move(P));
    }
    if (idx.empty()) continue;
    size_t j = 0;  // jobs served so far
    std::vector<std::unique_ptr<PPinned>> held;
    std::vector<const unsigned long long *> bits(idx.size(), nullptr);
    try {
      std::lock_guard<std::mutex> lk(dc->mu);
      resident_quit(*dc);  // (the resident search launch holds every CU's LDS)
      HIP_OK(hipSetDevice(dc->ordinal));
      const uint32_t cap = g_batch_jobs.load();
      while (j < idx.size()) {
        size_t j1 = j;
        uint64_t wg = 0;
        while (j1 < idx.size() && j1 - j < cap) {
          const uint64_t w = (uint64_t(plans[j1].t1 - plans[j1].t0) + kPThreads - 1) / kPThreads;
          if (j1 > j && wg + w > kPBatchGroups) break;
          wg += w;
          j1++;
        }
        held.push_back(proto_batch_launch(*dc, items, idx.data(), plans.data(), j, j1, outs, bits.data()));
        j = j1;
      }
    } catch (const Error &e) {  // a device error: the launch's items and the device's later ones
      for (size_t k = j; k < idx.size(); k++) failed(idx[k], e.code, e.what());
    } catch (const std::bad_alloc &) {
      for (size_t k = j; k < idx.size(); k++) failed(idx[k], TSG_E_OOM, "out of memory");
    }
    for (size_t k = 0; k < j; k++) proto_replay(*items[idx[k]].b, *items[idx[k]].req, plans[k], bits[k], outs[idx[k]]);
  }
}

}  // namespace tsg
