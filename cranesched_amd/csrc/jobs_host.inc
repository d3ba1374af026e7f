// The host pass of cns_upload_jobs: BasicPriority's truncation (JobScheduler.h:185-200), the per-job pre-checks of the ordered
// loop (JobScheduler.cpp:6744-6761: partition / reservation routing, pre-set reasons), the split of the queue by partition
// (:6516-6530) and the offsets of the placement records — everything the device needs besides the caller's own arrays.
//
// Round 5: at 1 M jobs this pass (two walks over the queue on ONE host thread, in front of the first H2D copy) was most of what
// SURVEY 8(d)'s bracket adds to the kernels.  It now runs as two passes over contiguous CHUNKS of the queue on a few host threads:
//   pass 1  validate, route, count: per chunk the placement records, the jobs per engine partition, the window-shaped jobs, the
//           algorithmic bytes; per job the pre-set reason and the engine partition
//   pass 2  (after a prefix sum over the chunks) per job the offset of its placement records, and the queue grouped by partition in
//           queue order — chunk c writes behind what the chunks before it counted, so the result is the serial one for any chunking
// and cns_upload_jobs issues the copies of the caller's arrays between the two, so that pass 2 runs in their shadow.
// No HIP in here: tests/cpp/jobs_host_test.cpp compiles this file with g++ and compares it with the one-thread walk it replaced
// (tests/test_jobs_host.py).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace cns_jobs_host {

constexpr uint32_t kNoPart = 0xFFFFFFFFu;

struct Route {                       // what the snapshot (cns_set_nodes / cns_set_reservations) says about routing
  uint32_t P = 0;                    // engine partitions (groups of partitions + one per reservation)
  uint32_t Pu = 0;                   // partitions of the caller
  uint32_t P_real = 0;               // engine partitions that are not reservations
  uint32_t V = 0;                    // reservations
  const uint8_t* upart_refused = nullptr;   // [Pu]
  const uint32_t* upart_eng = nullptr;      // [Pu] -> engine partition
  const uint32_t* upart_size = nullptr;     // [Pu] schedulable nodes
  const uint8_t* upart_tag = nullptr;       // [Pu] member tag (shared groups) or null
  const uint32_t* part_off = nullptr;       // [P + 1] slots per engine partition
  uint64_t s_node = 32;              // SURVEY 8(d): bytes of a node record in the traffic model
  uint32_t gres_classes = 0;         // defined GRES classes
  uint64_t batch = 0;                // jobs that reach the ordered loop at most (ScheduledBatchSize)
};

struct Out {
  uint8_t* reason = nullptr;         // [J]   pre-set reason (CNS_REASON_NONE: the job reaches an ordered loop)
  uint32_t* job_part = nullptr;      // [J]   engine partition, kNoPart: not given to an ordered loop
  uint64_t* place_off = nullptr;     // [J+1] first placement record of the job
  uint32_t* grouped = nullptr;       // [Jg]  queue indices grouped by engine partition, queue order inside a partition
  uint8_t* jtag = nullptr;           // [J]   member tag of the job's partition inside its group (null: no shared group)
  std::vector<uint64_t> pj_off;      // [P+1] first grouped position per engine partition
  uint64_t places = 0, algo = 0, n_shaped = 0, Jg = 0;
};

struct Chunk {
  uint64_t beg = 0, end = 0;
  uint64_t places = 0, algo = 0, n_shaped = 0;
  uint64_t bad_job = ~0ull;          // first job of the chunk that fails validation
  bool bad_gres = false;             // a routed job names an undefined GRES class
  std::vector<uint64_t> cnt;         // [P] routed jobs per engine partition; after the prefix sum: the chunk's first grouped position
};

// `fixed`: what the caller set on the handle (cns_set_host_threads); 0: the environment's CNS_HOST_THREADS, else up to 16
inline uint32_t threads_for(uint64_t J, uint32_t fixed = 0) {
  if (J < 32768) return 1;
  uint32_t t = fixed;
  if (t == 0)
    if (const char* e = getenv("CNS_HOST_THREADS")) t = (uint32_t)strtoul(e, nullptr, 10);
  if (t == 0) {
    t = std::thread::hardware_concurrency();
    if (t == 0) t = 1;
    if (t > 16) t = 16;
  }
  if (t > 64) t = 64;
  const uint64_t by_size = J / 16384;   // (a chunk below ~16 k jobs does not pay for its thread)
  if ((uint64_t)t > by_size) t = (uint32_t)by_size;
  return t ? t : 1;
}

// Chunk 0 on the calling thread, the others on threads of their own.  The engine never throws through its C ABI: a thread that cannot
// be started (std::system_error: the controller's thread limit) leaves its chunk — and the ones behind it — to the calling thread.
template <class F>
inline void for_chunks(std::vector<Chunk>& ch, F&& f) {
  if (ch.size() == 1) { f(ch[0], 0u); return; }
  std::vector<std::thread> th;
  th.reserve(ch.size() - 1);
  uint32_t started = 1;   // chunks [1, started) have a thread
  try {
    for (; started < ch.size(); ++started) th.emplace_back([&ch, &f, c = started] { f(ch[c], c); });
  } catch (...) {
  }
  f(ch[0], 0u);
  for (uint32_t c = started; c < ch.size(); ++c) f(ch[c], c);
  for (auto& t : th) t.join();
}

inline void pass1_chunk(const cns_job_soa* jb, const Route& R, const Out& o, Chunk& c) {
  c.cnt.assign(R.P, 0);
  static_assert(CNS_MAX_GRES_NAMES == 4 && CNS_MAX_GRES_CLASSES == 8, "the GRES counts of a job are read as one 32-bit and one 64-bit word");
  const uint64_t undefined = R.gres_classes >= 8 ? 0ull : ~0ull << (8 * R.gres_classes);   // count bytes of classes the layout does not define
  for (uint64_t j = c.beg; j < c.end; ++j) {
    const uint32_t k = jb->node_num[j];
    if (k == 0 || jb->ntasks[j] < k || jb->ntasks_per_node_min[j] == 0 || jb->ntasks_per_node_max[j] < jb->ntasks_per_node_min[j] ||
        jb->time_limit_sec[j] <= 0 || jb->task_cpu_raw[j] < 0 || (jb->node_cpu_raw && jb->node_cpu_raw[j] < 0)) {
      c.bad_job = j;
      return;
    }
    c.places += k;
    if (o.jtag) o.jtag[j] = 0;
    const uint32_t rsv = jb->reservation ? jb->reservation[j] : CNS_RESV_NONE;
    if (o.jtag && rsv == CNS_RESV_NONE && jb->partition[j] < R.Pu) o.jtag[j] = R.upart_tag[jb->partition[j]];
    o.job_part[j] = kNoPart;
    if (j >= R.batch) { o.reason[j] = CNS_REASON_PRIORITY; continue; }
    if (jb->skip && jb->skip[j]) { o.reason[j] = CNS_REASON_SKIPPED; continue; }
    // a job submitted to a reservation is scheduled by that reservation's scheduler, its partition is not looked at
    // (JobScheduler.cpp:6525-6527,6746-6761); whether the reservation is ACTIVE is decided on the device (needs `now`)
    uint32_t p;
    if (rsv != CNS_RESV_NONE) {
      if (rsv >= R.V) { o.reason[j] = CNS_REASON_RESERVATION_NOT_FOUND; continue; }
      p = R.P_real + rsv;
    } else {
      const uint32_t up = jb->partition[j];
      if (up >= R.Pu) { o.reason[j] = CNS_REASON_PARTITION_NOT_FOUND; continue; }
      if (R.upart_refused[up]) { o.reason[j] = CNS_REASON_ENGINE_REFUSED; continue; }   // (its group is outside the engine's limits: cns_get_partition_status)
      p = R.upart_eng[up];   // the engine partition that runs the job's partition (its group, if it shares nodes)
    }
    o.reason[j] = CNS_REASON_NONE;
    o.job_part[j] = p;
    c.cnt[p]++;
    bool shaped = k == 1 && jb->ntasks[j] == 1 && jb->ntasks_per_node_min[j] == 1 && !(jb->exclusive && jb->exclusive[j]) &&
                  !(jb->incl_offsets && jb->incl_offsets[j + 1] != jb->incl_offsets[j]) && !(jb->excl_offsets && jb->excl_offsets[j + 1] != jb->excl_offsets[j]);
    if (jb->gres_total) {              // (four name counts and eight class counts per job, read as one word each)
      uint32_t gt;
      memcpy(&gt, jb->gres_total + j * CNS_MAX_GRES_NAMES, sizeof gt);
      shaped = shaped && gt == 0;
    }
    if (jb->gres_spec) {
      uint64_t gs;
      memcpy(&gs, jb->gres_spec + j * CNS_MAX_GRES_CLASSES, sizeof gs);
      shaped = shaped && gs == 0;
      if (gs & undefined) c.bad_gres = true;
    }
    c.n_shaped += shaped ? 1u : 0u;
    const uint64_t np = rsv != CNS_RESV_NONE ? (uint64_t)(R.part_off[p + 1] - R.part_off[p]) : (uint64_t)R.upart_size[jb->partition[j]];
    c.algo += np * R.s_node + 64 + 16 + 24ull * k;  // SURVEY.md §8(d)
  }
}

inline void pass2_chunk(const cns_job_soa* jb, const Out& o, Chunk& c) {
  uint64_t run = c.places;           // (after the prefix sum: the chunk's first placement record)
  for (uint64_t j = c.beg; j < c.end; ++j) {
    o.place_off[j] = run;
    run += jb->node_num[j];
    const uint32_t p = o.job_part[j];
    if (p != kNoPart) o.grouped[c.cnt[p]++] = (uint32_t)j;
  }
}

// Pass 1.  Returns 0, or a CNS_ERR_* with *err set (the serial walk's messages and their precedence: the first invalid job, then an
// undefined GRES class).  `chunks` carries the state pass 2 needs.
inline int pass1(const cns_job_soa* jb, const Route& R, Out& o, std::vector<Chunk>& chunks, uint32_t threads, std::string* err) {
  const uint64_t J = jb->num_jobs;
  if (threads == 0) threads = 1;
  chunks.assign(threads, Chunk{});
  for (uint32_t c = 0; c < threads; ++c) { chunks[c].beg = J * c / threads; chunks[c].end = J * (c + 1) / threads; }
  for_chunks(chunks, [&](Chunk& c, uint32_t) { pass1_chunk(jb, R, o, c); });
  for (const Chunk& c : chunks)
    if (c.bad_job != ~0ull) {
      *err = "job " + std::to_string(c.bad_job) + ": invalid node_num/ntasks/time_limit/cpu";
      return CNS_ERR_INVALID_ARG;
    }
  for (const Chunk& c : chunks)
    if (c.bad_gres) { *err = "job requests an undefined GRES class"; return CNS_ERR_INVALID_ARG; }
  // totals, and every chunk's first placement record / first grouped position per partition
  o.places = o.algo = o.n_shaped = 0;
  std::vector<uint64_t> per_part(R.P, 0);
  for (Chunk& c : chunks) {
    const uint64_t pl = c.places;
    c.places = o.places;
    o.places += pl;
    o.algo += c.algo;
    o.n_shaped += c.n_shaped;
    for (uint32_t p = 0; p < R.P; ++p) per_part[p] += c.cnt[p];
  }
  o.pj_off.assign((size_t)R.P + 1, 0);
  for (uint32_t p = 0; p < R.P; ++p) o.pj_off[p + 1] = o.pj_off[p] + per_part[p];
  o.Jg = o.pj_off[R.P];
  std::vector<uint64_t> cur(o.pj_off.begin(), o.pj_off.end() - 1);
  for (Chunk& c : chunks)
    for (uint32_t p = 0; p < R.P; ++p) { const uint64_t n = c.cnt[p]; c.cnt[p] = cur[p]; cur[p] += n; }
  return 0;
}

// Pass 2: o.place_off [J + 1] and o.grouped [o.Jg] must be allocated by now.
inline void pass2(const cns_job_soa* jb, Out& o, std::vector<Chunk>& chunks) {
  for_chunks(chunks, [&](Chunk& c, uint32_t) { pass2_chunk(jb, o, c); });
  o.place_off[jb->num_jobs] = o.places;
}

// The packed result buffer of a job table (one contiguous HBM buffer: what cns_results_layout reports and an all-gather ships): the
// byte offset of every section, each a multiple of 16 and at least one element long.  The ORDER carries the reset in front of a pass:
// start and the five 8-byte record arrays lie in one run (one memset over [start, node) zeroes them), node (0xFF) and ntasks follow,
// and the planes of core ids 128..255 come last, c2 then c3 (one memset over [c2, total)).  They exist only for a snapshot with such
// nodes: c2 == c3 == total otherwise, nothing more to ship.
struct ResOff { size_t start, cpu, mem, clo, chi, gres, node, ntasks, reason, c2, c3, total; };
inline size_t align16(size_t x) { return (x + 15) & ~size_t(15); }
inline ResOff result_layout(uint64_t J, uint64_t places, bool wide_cores) {
  size_t end = 0;
  auto sec = [&](size_t elem, uint64_t n) { const size_t at = end; end = align16(end + elem * (size_t)(n ? n : 1)); return at; };
  ResOff r{};
  r.start = sec(8, J); r.cpu = sec(8, places); r.mem = sec(8, places); r.clo = sec(8, places);
  r.chi = sec(8, places); r.gres = sec(8, places); r.node = sec(4, places); r.ntasks = sec(4, places);
  r.reason = sec(1, J);
  r.c2 = r.c3 = end;
  if (wide_cores) { r.c2 = sec(8, places); r.c3 = sec(8, places); }
  r.total = end;
  return r;
}

}  // namespace cns_jobs_host
