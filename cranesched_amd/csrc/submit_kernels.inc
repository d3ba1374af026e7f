// Submit-limit admission of a batch of submissions on the GPU (include/crane_gpu_submit/submit_limits.h):
// AccountMetaContainer::TryMallocMetaSubmitResource + MallocMetaSubmitResource (src/CraneCtld/Accounting/AccountMetaContainer.cpp:75-153,
// :374-506, :694-889, :1067-1124) for J jobs in arrival order.  Included by engine.hip (one translation unit, namespace cns).
//
// What changes during a batch is ONE table of 32-bit values: the five submit_jobs_count tables back to back
// [user x qos | user_acct x partition | account x qos | account x partition | qos] (NR records) and behind them one value per entity
// [user | account | qos] (NE values) that is non-zero when the entity's record exists.  Everything else a check reads (limits, jobs_count,
// resource, wall) is an input, so k_sub_prep evaluates it once per job and what is left per job is a list of at most 8 SLOTS in the
// reference's order (the user, up to 6 chain accounts from the job's account to the root, the QoS), each with 3 ITEMS:
//   item 3e   the entity's exists value            (read: > 0; an admission adds 1)
//   item 3e+1 record A, the entity's QoS record    (read: value + count > threshold; an admission adds count)
//   item 3e+2 record B, its partition record       (the same; none for the QoS slot)
// and per slot two precomputed codes: stat (a static check that fails whatever the tables hold: the job is rejected, and the code is
// this one unless an earlier slot fails first) and cond (a static check that fails IF the entity exists: the DenyOnLimit checks).
// One job's decision, given the values v its items see (sub_first_failure): for each slot in order: stat -> that code; if v[entity] > 0:
// A over its threshold -> codeA; cond -> that code; B over its threshold -> codeB.  No code: admitted, every item's value grows.
//
// Kernels
//   k_sub_prep   job-parallel, one lane per job: req_total and req_total * count with overflow detection, every check that does not depend
//                on the batch, the rewritten time limit, the items.
//   k_sub_admit  the ordered admission, ONE wave64: lane = item; per job 24 loads of the table (the only loads that depend on earlier
//                admissions), two ballots, a uniform walk over the 8 slots, 24 stores.  The fallback and the second implementation.
//   the parallel admission (the bracket of limits_kernels.hip on a scalar): items sorted by table index, stable (k_sort_*); per round
//                k_sub_tails (per chunk of sorted items the sums of its last segment over A = surely admitted and over not-X = not
//                surely rejected), k_sub_carry (scan over the chunk tails, one workgroup), k_sub_eval (re-walk with the carry: every
//                item of an undecided job gets the lower and the upper value it may see), k_sub_decide (job-parallel: passes under
//                the upper values -> admitted, fails under the lower ones -> rejected).  Every check is monotone: a larger count, or an
//                existing entity, only fails more.  The first undecided job has a zero-width interval, so every round decides at least
//                one job.  k_sub_final turns the exact values into codes and adds the admitted jobs' items to the table.
// No workgroup waits for another: a scan across workgroups is separate launches.  Every loop is bounded by an argument.
#pragma once

namespace cns {

constexpr u32 kSubChunk = 256;        // jobs per workgroup of k_sub_prep (one lane per job)
constexpr u32 kSubSlots = 8;          // user, CNS_LIM_MAX_CHAIN accounts, qos
constexpr u32 kSubItems = 24;         // 3 per slot
constexpr u32 kSubPerThread = 8;      // sorted items a lane walks
constexpr u32 kSubItemChunk = 256 * kSubPerThread;   // sorted items per workgroup of a round
constexpr u32 kSubMaxRounds = 48;
constexpr u32 kSubNoCheck = 0xFFFFFFFFu;   // threshold no sum can pass (submit_limits.h: no sum of the call goes beyond UINT32_MAX)
static_assert(CNS_LIM_MAX_CHAIN + 2 == kSubSlots, "one slot per chain account, the user and the QoS");

struct SubRes {   // a ResourceView: cpu, mem, per GRES name its total, per class its count; ovf: a component left 64 bits
  i64 cpu; u64 mem; u64 nt[4]; u64 cc[8]; bool ovf;
};

struct SubParams {
  u32 J, Q, Pn, NK;                   // NK = NR + NE: the table's length, and the key of an unused item
  u32 base_uq, base_up, base_aq, base_ap, base_g, ent_user, ent_acct, ent_qos;
  // jobs (cns_job_soa) and keys (cns_submit_keys) as uploaded
  const u32* part; const i64* tl; const i64* ncpu; const u64* nmem; const i64* tcpu; const u64* tmem; const u32* k; const u32* nt;
  const u32* gt; const u64* gs;       // [J] 4 / 8 count bytes per job; may be null
  const u32* user; const u32* ua; const u32* account; const u32* qos; const u32* count; const uint8_t* skip;
  // tables
  const cns_submit_qos* q; const cns_submit_part_limit* pl; const u32* acct_parent; const u32* upl; const u32* apl;   // upl / apl may be null
  const cns_usage* uq_use; const cns_usage* aq_use; const cns_usage* g_use;   // may be null
  cns_gres_layout lay;
  u32* st;                            // [NK] the table
  // per job
  uint8_t* pre; uint8_t* state; u64* stat; u64* cond; u32* item_key; u32* item_thr; u64* sort_key;   // sort_key may be null
  uint8_t* code; i64* tlo;
  u64* ctr;                           // 0 candidates, 1 admitted, 2 sorted items with a key, 3 undecided, 4 largest record value
};

__device__ __forceinline__ bool sub_mul_u64(u64 a, u64 b, u64* r) { return __builtin_mul_overflow(a, b, r); }

// present(n): the GresMap has an entry for name n (a total, or a class of that name)
__device__ __forceinline__ bool sub_name_present(const SubRes& r, const cns_gres_layout& lay, u32 n) {
  bool p = r.nt[n] > 0;
  for (u32 g = 0; g < lay.num_classes && g < 8; ++g) p = p || (lay.class_name[g] == n && r.cc[g] > 0);
  return p;
}

// CheckTres_ (:345-360) with CheckGres_ (:1030-1050) in the canonical order: ascending name, its total, its classes ascending
__device__ bool sub_check_tres(const SubRes& r, const cns_tres& lim, const cns_gres_layout& lay) {
  if (r.ovf) return false;
  if (r.cpu > lim.cpu_raw) return false;
  if (r.mem > lim.mem) return false;
  for (u32 n = 0; n < 4; ++n) {
    if (!sub_name_present(r, lay, n)) continue;
    if (!(lim.name_mask >> n & 1)) return true;            // :1034
    if (r.nt[n] > lim.name_total[n]) return false;         // :1039
    for (u32 g = 0; g < lay.num_classes && g < 8; ++g) {
      if (lay.class_name[g] != n || r.cc[g] == 0) continue;
      if (!(lim.class_mask >> g & 1)) return true;         // :1044
      if (r.cc[g] > lim.class_count[g]) return false;      // :1045
    }
  }
  return true;
}

// req + usage (ResourceView +=); a sum beyond 64 bits sets ovf: beyond every limit
__device__ SubRes sub_add_usage(const SubRes& r, const cns_usage* u) {
  SubRes s = r;
  if (!u) return s;
  s.ovf = s.ovf || __builtin_add_overflow(r.cpu, u->cpu_raw, &s.cpu);
  s.ovf = s.ovf || __builtin_add_overflow(r.mem, u->mem, &s.mem);
  for (u32 n = 0; n < 4; ++n) s.ovf = s.ovf || __builtin_add_overflow(r.nt[n], u->name_total[n], &s.nt[n]);
  for (u32 g = 0; g < 8; ++g) s.ovf = s.ovf || __builtin_add_overflow(r.cc[g], u->class_count[g], &s.cc[g]);
  return s;
}

__device__ __forceinline__ u32 sub_code_a(u32 e) {
  return e == 0 ? CNS_SUBMIT_MAX_JOB_COUNT_PER_USER : e == kSubSlots - 1 ? CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED : CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;
}
__device__ __forceinline__ u32 sub_code_b(u32 e) {
  return e == 0 ? CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER : CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT;
}

// the static part of an entity with a partition limit record (:715-749 / :784-819)
__device__ u32 sub_static_part(const cns_submit_part_limit* lim, const cns_submit_qos& q, bool is_user, const SubRes& req, i64 tl, u32 count,
                               const cns_gres_layout& lay) {
  if (!lim) return 0;
  if (!sub_check_tres(req, lim->max_tres_per_job, lay)) return CNS_SUBMIT_PARTITION_TRES_PER_JOB_BEYOND;
  if (q.max_time_limit_per_job_sec == CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC && tl > lim->max_wall_duration_per_job_sec) return CNS_SUBMIT_PARTITION_TIME_BEYOND;
  if ((is_user ? q.max_submit_jobs_per_user : q.max_submit_jobs_per_account) == 0xFFFFFFFFu && count > lim->max_submit_jobs)
    return is_user ? CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER : CNS_SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT;
  return 0;
}

// the DenyOnLimit checks of CheckQosSubmitLimitsForEntity_ (:389-409): static, and they apply only if the entity exists
__device__ u32 sub_cond_entity(const cns_usage* use, const cns_submit_qos& q, bool is_user, const SubRes& req, const cns_gres_layout& lay) {
  if (!q.deny_on_limit) return 0;
  const u32 jobs = use ? use->jobs_count : 0;
  if ((u64)jobs + 1 > (is_user ? q.max_jobs_per_user : q.max_jobs_per_account))                       // :392
    return is_user ? CNS_SUBMIT_MAX_JOB_COUNT_PER_USER : CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;
  const SubRes s = sub_add_usage(req, use);                                                           // :397-398
  if (is_user) {
    if (s.ovf || s.cpu > q.max_cpus_per_user_raw) return CNS_SUBMIT_CPUS_PER_TASK_BEYOND;             // :401
    if (!sub_check_tres(s, q.max_tres_per_user, lay)) return CNS_SUBMIT_MAX_TRES_PER_USER_BEYOND;     // :403
  } else if (!sub_check_tres(s, q.max_tres_per_account, lay)) {
    return CNS_SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND;                                                    // :406
  }
  return 0;
}

__global__ __launch_bounds__(256) void k_sub_prep(const SubParams P) {
  const u32 j = blockIdx.x * kSubChunk + threadIdx.x;
  bool cand = false;
  if (j < P.J) {
    u32* key = P.item_key + (size_t)j * kSubItems;
    u32* thr = P.item_thr + (size_t)j * kSubItems;
    for (u32 x = 0; x < kSubItems; ++x) { key[x] = P.NK; thr[x] = kSubNoCheck; }
    i64 tl = P.tl[j];
    u32 pre = 0;
    u64 stat = 0, cond = 0;
    bool rejected = false;   // a static failure inside the slots: never admitted, the code may still come from an earlier slot
    const u32 count = P.count[j];
    SubRes req{};
    if (P.skip && P.skip[j]) pre = CNS_SUBMIT_NOT_CANDIDATE;
    else if (count == 0) pre = CNS_SUBMIT_BAD_COUNT;
    else {
      // ---- req_total = node * node_num + task * ntasks (JobScheduler.cpp:7156-7157), then x count (:97) ----
      const u32 k = P.k[j], nt = P.nt[j];
      i64 a, b;
      u64 c, d;
      bool ovf = __builtin_mul_overflow(P.ncpu ? P.ncpu[j] : (i64)0, (i64)k, &a);
      ovf = __builtin_mul_overflow(P.tcpu[j], (i64)nt, &b) || ovf;
      ovf = __builtin_add_overflow(a, b, &req.cpu) || ovf;
      ovf = sub_mul_u64(P.nmem[j], k, &c) || ovf;
      ovf = sub_mul_u64(P.tmem[j], nt, &d) || ovf;
      ovf = __builtin_add_overflow(c, d, &req.mem) || ovf;
      const u32 gt = P.gt ? P.gt[j] : 0u;
      const u64 gs = P.gs ? P.gs[j] : 0ull;
      for (u32 n = 0; n < 4; ++n) req.nt[n] = (u64)(gt >> (8 * n) & 255u) * k;
      for (u32 g = 0; g < 8; ++g) req.cc[g] = g < P.lay.num_classes ? (u64)(gs >> (8 * g) & 255ull) * k : 0ull;
      SubRes use = req;
      ovf = __builtin_mul_overflow(req.cpu, (i64)count, &use.cpu) || ovf;
      ovf = sub_mul_u64(req.mem, count, &use.mem) || ovf;
      for (u32 n = 0; n < 4; ++n) use.nt[n] = req.nt[n] * count;    // < 2^8 * 2^32 * 2^32: no overflow
      for (u32 g = 0; g < 8; ++g) use.cc[g] = req.cc[g] * count;
      const cns_submit_qos& q = P.q[P.qos[j]];
      if (ovf) pre = CNS_SUBMIT_BAD_REQUEST;
      else if (count > q.max_submit_jobs_per_user) pre = CNS_SUBMIT_MAX_JOB_COUNT_PER_USER;            // :99
      else if (count > q.max_submit_jobs_per_account) pre = CNS_SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT;      // :102
      else if (count > q.max_submit_jobs) pre = CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED;                     // :105
      else if (use.cpu > q.max_cpus_per_user_raw) pre = CNS_SUBMIT_CPUS_PER_TASK_BEYOND;               // :108
      else if (!sub_check_tres(use, q.max_tres_per_user, P.lay) || !sub_check_tres(use, q.max_tres_per_account, P.lay) ||
               !sub_check_tres(use, q.max_tres, P.lay)) pre = CNS_SUBMIT_TRES_PER_JOB_BEYOND;          // :111-114
      else if (tl >= CNS_SUBMIT_JOB_MAX_TIME_LIMIT_SEC) tl = q.max_time_limit_per_job_sec;             // :118-119
      else if (tl > q.max_time_limit_per_job_sec) pre = CNS_SUBMIT_TIME_LIMIT_BEYOND;                  // :120-122
    }
    if (!pre) {
      cand = true;
      const u32 qi = P.qos[j], u = P.user[j], ua = P.ua[j], part = P.part[j];
      const cns_submit_qos& q = P.q[qi];
      // ---- slot 0: the user (:701-767) ----
      if (ua == kNone) {
        stat |= (u64)CNS_SUBMIT_USER_ACCOUNT_MISMATCH;   // :703-708
        rejected = true;
      } else {
        const u32 li = P.upl ? P.upl[(size_t)ua * P.Pn + part] : kNone;
        const cns_submit_part_limit* lim = li == kNone ? nullptr : P.pl + li;
        const u32 s = sub_static_part(lim, q, true, req, tl, count, P.lay);
        if (s) { stat |= (u64)s; rejected = true; }
        else {
          key[0] = P.ent_user + u;
          key[1] = P.base_uq + u * P.Q + qi; thr[1] = q.max_submit_jobs_per_user;                      // :384
          key[2] = P.base_up + ua * P.Pn + part;
          if (lim && q.max_submit_jobs_per_user == 0xFFFFFFFFu) thr[2] = lim->max_submit_jobs;         // :420-445
          cond |= (u64)sub_cond_entity(P.uq_use ? P.uq_use + (size_t)u * P.Q + qi : nullptr, q, true, req, P.lay);
        }
      }
      // ---- slots 1..6: the account chain, from the job's account to the root (:770-838) ----
      u32 a = P.account[j];
      for (u32 e = 1; e <= CNS_LIM_MAX_CHAIN && a != kNone && !rejected; ++e) {
        const u32 li = P.apl ? P.apl[(size_t)a * P.Pn + part] : kNone;
        const cns_submit_part_limit* lim = li == kNone ? nullptr : P.pl + li;
        const u32 s = sub_static_part(lim, q, false, req, tl, count, P.lay);
        if (s) { stat |= (u64)s << (8 * e); rejected = true; break; }
        key[3 * e] = P.ent_acct + a;
        key[3 * e + 1] = P.base_aq + a * P.Q + qi; thr[3 * e + 1] = q.max_submit_jobs_per_account;
        key[3 * e + 2] = P.base_ap + a * P.Pn + part;
        if (lim && q.max_submit_jobs_per_account == 0xFFFFFFFFu) thr[3 * e + 2] = lim->max_submit_jobs;
        cond |= (u64)sub_cond_entity(P.aq_use ? P.aq_use + (size_t)a * P.Q + qi : nullptr, q, false, req, P.lay) << (8 * e);
        a = P.acct_parent[a];
      }
      // ---- slot 7: the QoS globally (:841-886) ----
      if (!rejected) {
        const u32 e = kSubSlots - 1;
        key[3 * e] = P.ent_qos + qi;
        key[3 * e + 1] = P.base_g + qi; thr[3 * e + 1] = q.max_submit_jobs;                            // :844
        u32 c = 0;
        if (q.deny_on_limit) {
          const cns_usage* val = P.g_use ? P.g_use + qi : nullptr;
          const i64 wall = val ? val->wall_sec : 0;
          i64 wsum;
          const bool wovf = __builtin_add_overflow(wall, tl, &wsum);
          if ((u64)(val ? val->jobs_count : 0u) + 1 > q.max_jobs) c = CNS_SUBMIT_QOS_JOB_COUNT_EXCEEDED;                        // :854
          else if (q.max_wall_sec > 0 && (wovf ? tl > 0 : wsum > q.max_wall_sec)) c = CNS_SUBMIT_TIME_LIMIT_BEYOND;             // :863-864
          else if (!sub_check_tres(sub_add_usage(req, val), q.max_tres, P.lay)) c = CNS_SUBMIT_TRES_PER_JOB_BEYOND;             // :875-877
        }
        cond |= (u64)c << (8 * e);
      }
    }
    P.pre[j] = (uint8_t)pre;
    P.state[j] = pre || rejected ? 2 : 0;
    P.stat[j] = stat;
    P.cond[j] = cond;
    P.tlo[j] = tl;
    if (pre) P.code[j] = (uint8_t)pre;
    if (P.sort_key)
      for (u32 x = 0; x < kSubItems; ++x) P.sort_key[(size_t)j * kSubItems + x] = key[x];
  }
  const u64 b = __ballot(cand);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)P.ctr, (unsigned long long)__popcll(b));
}

// One job's decision from what its items see.  ex / fa / fb: bit e set = slot e's entity exists / its record A / B is over the threshold.
__device__ __forceinline__ u32 sub_first_failure(u64 stat, u64 cond, u32 ex, u32 fa, u32 fb) {
  for (u32 e = 0; e < kSubSlots; ++e) {
    const u32 s = (u32)(stat >> (8 * e)) & 255u, c = (u32)(cond >> (8 * e)) & 255u;
    if (s) return s;
    if (ex >> e & 1) {
      if (fa >> e & 1) return sub_code_a(e);
      if (c) return c;
      if (fb >> e & 1) return sub_code_b(e);
    }
  }
  return 0;
}

// ---- the ordered admission: one wave, lane = item -----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sub_admit(const SubParams P) {
  const u32 lane = threadIdx.x, r = lane % 3, e = lane / 3;
  const bool it = lane < kSubItems;
  u64 adm = 0;
  u32 key_n = P.NK, thr_n = kSubNoCheck;
  if (P.J && it) { key_n = P.item_key[lane]; thr_n = P.item_thr[lane]; }
  for (u32 j = 0; j < P.J; ++j) {
    const u32 key = key_n, thr = thr_n;
    if (j + 1 < P.J && it) { key_n = P.item_key[(size_t)(j + 1) * kSubItems + lane]; thr_n = P.item_thr[(size_t)(j + 1) * kSubItems + lane]; }
    if (P.pre[j]) continue;   // uniform: decided by k_sub_prep, code written there
    const bool used = it && key < P.NK;
    const u32 v = used ? P.st[key] : 0u;
    const u32 count = P.count[j];
    const bool over = used && r != 0 && thr != kSubNoCheck && (u64)v + count > thr;
    const u64 bex = __ballot(used && r == 0 && v > 0), bov = __ballot(over);
    u32 ex = 0, fa = 0, fb = 0;
    for (u32 s = 0; s < kSubSlots; ++s) {
      ex |= (u32)(bex >> (3 * s) & 1) << s; fa |= (u32)(bov >> (3 * s + 1) & 1) << s; fb |= (u32)(bov >> (3 * s + 2) & 1) << s;
    }
    const u32 code = sub_first_failure(P.stat[j], P.cond[j], ex, fa, fb);
    if (!code) {   // MallocMetaSubmitResource: every record grows by count, every entity exists from now on
      if (used) P.st[key] = v + (r == 0 ? 1u : count);
      ++adm;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the next job's loads (other lanes) see these stores
    }
    if (lane == 0) P.code[j] = (uint8_t)code;
    (void)e;
  }
  if (lane == 0) P.ctr[1] = adm;
}

// ---- the parallel admission ---------------------------------------------------------------------------------------------------
struct SubPar {
  u32 n, nchunks, J, NK;    // n: sorted items that carry a key
  const u32* s_key; const u32* s_item; const u32* s_add;   // [n] table index, job * 24 + position, what an admission adds
  const uint8_t* state;     // [J] 0 undecided, 1 admitted, 2 rejected
  const u32* st;            // the table before the batch
  uint2* tails; uint8_t* heads; uint2* carry;   // [nchunks]
  uint2* val;               // [J * 24] lower / upper value an item sees
};

// sorted (key, item) pairs -> streams; ctr[2] = how many items carry a key
__global__ __launch_bounds__(256) void k_sub_gather(const u64* __restrict__ keys, const u32* __restrict__ vals, u32 n, u32 NK, const u32* __restrict__ count,
                                                    u32* s_key, u32* s_item, u32* s_add, u64* ctr) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u64 key = keys[i];
  if (key >= NK) return;
  const u32 item = vals[i];
  s_key[i] = (u32)key; s_item[i] = item;
  s_add[i] = item % 3 == 0 ? 1u : count[item / kSubItems];
  if (i + 1 == n || keys[i + 1] >= NK) ctr[2] = (u64)i + 1;
}

// A workgroup's chunk of the sorted items: every lane walks kSubPerThread consecutive items; the lanes' sums are combined by a segmented
// scan in LDS (a segment = the items of one table index).  -> this lane's exclusive prefix inside the chunk (xl, xu; xh: a segment head
// lies before this lane inside the chunk) and, in s_* [255], the chunk's total.
struct SubWalk { u32 key[kSubPerThread], item[kSubPerThread], al[kSubPerThread], au[kSubPerThread]; bool act[kSubPerThread], head[kSubPerThread]; };

__device__ __forceinline__ void sub_walk_load(const SubPar& P, u32 beg, SubWalk& W) {
  const u32 i0 = beg + threadIdx.x * kSubPerThread;
  u32 prev = i0 > 0 && i0 - 1 < P.n ? P.s_key[i0 - 1] : kNone;
#pragma unroll
  for (u32 b = 0; b < kSubPerThread; ++b) {
    const u32 i = i0 + b;
    W.act[b] = i < P.n;
    const u32 x = W.act[b] ? i : 0u;   // clamped: masked afterwards (item 0 exists whenever n > 0)
    W.key[b] = P.s_key[x]; W.item[b] = P.s_item[x];
    const u32 add = P.s_add[x];
    const u32 st = P.state[W.item[b] / kSubItems];
    W.al[b] = W.act[b] && st == 1 ? add : 0u;
    W.au[b] = W.act[b] && st != 2 ? add : 0u;
    W.head[b] = W.act[b] && W.key[b] != prev;
    if (W.act[b]) prev = W.key[b];
  }
}

__device__ __forceinline__ void sub_block_scan(const SubWalk& W, u32* s_l, u32* s_u, u32* s_h, u32& xl, u32& xu, u32& xh) {
  u32 l = 0, u = 0, hd = 0;
#pragma unroll
  for (u32 b = 0; b < kSubPerThread; ++b) {
    if (W.head[b]) { l = 0; u = 0; hd = 1; }
    l += W.al[b]; u += W.au[b];
  }
  const u32 t = threadIdx.x;
  s_l[t] = l; s_u[t] = u; s_h[t] = hd;
  __syncthreads();
  for (u32 d = 1; d < 256; d <<= 1) {   // Hillis-Steele, inclusive, segmented: (a then b) = b.head ? b : (a + b, a.head)
    u32 pl = 0, pu = 0, ph = 0;
    if (t >= d) { pl = s_l[t - d]; pu = s_u[t - d]; ph = s_h[t - d]; }
    __syncthreads();
    if (t >= d && !s_h[t]) { s_l[t] += pl; s_u[t] += pu; s_h[t] = ph; }
    __syncthreads();
  }
  xl = t ? s_l[t - 1] : 0u; xu = t ? s_u[t - 1] : 0u; xh = t ? s_h[t - 1] : 0u;
}

__global__ __launch_bounds__(256) void k_sub_tails(const SubPar P) {
  __shared__ u32 s_l[256], s_u[256], s_h[256];
  SubWalk W;
  sub_walk_load(P, blockIdx.x * kSubItemChunk, W);
  u32 xl, xu, xh;
  sub_block_scan(W, s_l, s_u, s_h, xl, xu, xh);
  if (threadIdx.x == 255) { P.tails[blockIdx.x] = make_uint2(s_l[255], s_u[255]); P.heads[blockIdx.x] = (uint8_t)s_h[255]; }
}

// carry[c] = the sums of the items since the last segment head before chunk c.  One workgroup: every lane over `per` consecutive chunks,
// a segmented scan over the lanes, a second sweep that writes.
__global__ __launch_bounds__(1024) void k_sub_carry(const SubPar P) {
  __shared__ u32 s_l[1024], s_u[1024], s_h[1024];
  const u32 t = threadIdx.x, per = (P.nchunks + 1023) / 1024;
  const u32 lo = t * per < P.nchunks ? t * per : P.nchunks, hi = lo + per < P.nchunks ? lo + per : P.nchunks;
  u32 l = 0, u = 0, hd = 0;
  for (u32 c = lo; c < hi; ++c) {
    const uint2 v = P.tails[c];
    if (P.heads[c]) { l = v.x; u = v.y; hd = 1; } else { l += v.x; u += v.y; }
  }
  s_l[t] = l; s_u[t] = u; s_h[t] = hd;
  __syncthreads();
  for (u32 d = 1; d < 1024; d <<= 1) {
    u32 pl = 0, pu = 0, ph = 0;
    if (t >= d) { pl = s_l[t - d]; pu = s_u[t - d]; ph = s_h[t - d]; }
    __syncthreads();
    if (t >= d && !s_h[t]) { s_l[t] += pl; s_u[t] += pu; s_h[t] = ph; }
    __syncthreads();
  }
  l = t ? s_l[t - 1] : 0u; u = t ? s_u[t - 1] : 0u;
  for (u32 c = lo; c < hi; ++c) {
    P.carry[c] = make_uint2(l, u);
    const uint2 v = P.tails[c];
    if (P.heads[c]) { l = v.x; u = v.y; } else { l += v.x; u += v.y; }
  }
}

// FINAL = false: the items of the undecided jobs get the interval of values they may see.  FINAL = true: every job is decided, the
// interval has no width: every item gets the exact value it sees.
template <bool FINAL>
__global__ __launch_bounds__(256) void k_sub_eval(const SubPar P) {
  __shared__ u32 s_l[256], s_u[256], s_h[256];
  SubWalk W;
  sub_walk_load(P, blockIdx.x * kSubItemChunk, W);
  u32 xl, xu, xh;
  sub_block_scan(W, s_l, s_u, s_h, xl, xu, xh);
  const uint2 cin = P.carry[blockIdx.x];
  u32 l = xh ? xl : xl + cin.x, u = xh ? xu : xu + cin.y;
#pragma unroll
  for (u32 b = 0; b < kSubPerThread; ++b) {
    if (W.head[b]) { l = 0; u = 0; }
    if (W.act[b] && (FINAL || P.state[W.item[b] / kSubItems] == 0)) {
      const u32 base = P.st[W.key[b]];
      P.val[W.item[b]] = make_uint2(base + l, base + u);
    }
    l += W.al[b]; u += W.au[b];
  }
}

__device__ __forceinline__ void sub_job_masks(const SubParams& P, const uint2* val, u32 j, bool upper, u32& ex, u32& fa, u32& fb) {
  const u32 count = P.count[j];
  ex = fa = fb = 0;
  for (u32 e = 0; e < kSubSlots; ++e) {
    const size_t x = (size_t)j * kSubItems + 3 * e;
    if (P.item_key[x] >= P.NK) continue;   // the slot is not used
    const uint2 ve = val[x], va = val[x + 1];
    if ((upper ? ve.y : ve.x) > 0) ex |= 1u << e;
    const u32 ta = P.item_thr[x + 1], tb = P.item_thr[x + 2];
    if (ta != kSubNoCheck && (u64)(upper ? va.y : va.x) + count > ta) fa |= 1u << e;
    if (P.item_key[x + 2] < P.NK && tb != kSubNoCheck) {
      const uint2 vb = val[x + 2];
      if ((u64)(upper ? vb.y : vb.x) + count > tb) fb |= 1u << e;
    }
  }
}

__global__ __launch_bounds__(256) void k_sub_decide(const SubParams P, const uint2* val) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  bool und = false;
  if (j < P.J && P.state[j] == 0) {
    u32 ex, fa, fb;
    const u64 stat = P.stat[j], cond = P.cond[j];
    sub_job_masks(P, val, j, false, ex, fa, fb);
    if (sub_first_failure(stat, cond, ex, fa, fb)) P.state[j] = 2;          // fails whatever the undecided jobs turn out to be
    else {
      sub_job_masks(P, val, j, true, ex, fa, fb);
      if (!sub_first_failure(stat, cond, ex, fa, fb)) P.state[j] = 1;       // passes whatever they turn out to be
      else und = true;
    }
  }
  const u64 b = __ballot(und);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)(P.ctr + 3), (unsigned long long)__popcll(b));
}

// exact values -> codes; the admitted jobs' items grow the table (DoMallocResource_)
__global__ __launch_bounds__(256) void k_sub_final(const SubParams P, const uint2* val) {
  const u32 j = blockIdx.x * 256 + threadIdx.x;
  bool adm = false;
  if (j < P.J && !P.pre[j]) {
    u32 ex, fa, fb;
    sub_job_masks(P, val, j, false, ex, fa, fb);
    const u32 code = sub_first_failure(P.stat[j], P.cond[j], ex, fa, fb);
    P.code[j] = (uint8_t)code;
    adm = code == 0;
    if (adm) {
      const u32 count = P.count[j];
      for (u32 x = 0; x < kSubItems; ++x) {
        const u32 key = P.item_key[(size_t)j * kSubItems + x];
        if (key < P.NK) atomicAdd(P.st + key, x % 3 == 0 ? 1u : count);
      }
    }
  }
  const u64 b = __ballot(adm);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)(P.ctr + 1), (unsigned long long)__popcll(b));
}

// the largest submit count of the table (the input rule of the next call that carries on)
__global__ __launch_bounds__(256) void k_sub_max(const u32* st, u32 NR, u64* ctr) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  u32 v = i < NR ? st[i] : 0u;
  for (u32 off = 32; off; off >>= 1) { const u32 o = (u32)__shfl_xor((int)v, (int)off); v = o > v ? o : v; }
  if ((threadIdx.x & 63) == 0 && v) atomicMax((unsigned long long*)(ctr + 4), (unsigned long long)v);
}

}  // namespace cns
