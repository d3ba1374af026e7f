// MultiFactorPriority on the GPU: bounds (min/max reductions) -> per-account service values -> one fp64
// priority per pending job -> stable LSD radix sort by descending priority (the sort's kernels: sort_kernels.inc).
//
// Reference: src/CraneCtld/JobScheduler.cpp:7606-7819 (see include/crane_gpu/priority.h).  Unlike the node
// selection chain this path is embarrassingly parallel and HBM-bound: every kernel streams SoA arrays with
// coalesced loads; reductions go wave (DPP) -> one atomic per wave.  fp64 is evaluated in the reference's
// operation order with -ffp-contract=off, so priorities match the CPU bit for bit.
//
// Included by engine.hip after select_kernels.hip and sort_kernels.inc (one translation unit, namespace cns).
#pragma once

namespace cns {

struct PrioBounds {  // FactorBound, JobScheduler.h:214-224 (+ the per-account map as two arrays)
  u64 age_max, age_min;
  u64 mem_max, mem_min;
  u64 cpus_max_bits, cpus_min_bits;  // non-negative doubles order like their bit patterns
  double sv_max, sv_min;
  u32 qos_max, qos_min;
  u32 part_max, part_min;
  u32 nn_max, nn_min;
};

struct PrioParams {
  i64 now;
  u64 max_age;
  u32 w_age, w_fair, w_size, w_part, w_qos, favor_small;
  u32 J, R, A, pad;
  // pending
  const i64* submit; const u32* qos; const u32* part; const u32* node_num; const i64* cpu_raw; const u64* mem;
  const u32* account; const double* cached;
  // running
  const i64* r_start; const u32* r_qos; const u32* r_part; const u32* r_node_num; const i64* r_cpu_raw;
  const u64* r_mem; const u32* r_account;
  const u32* acc_off;     // [A+1] CSR: running jobs of each account, in vector order
  const u32* acc_jobs;    // [R]
  const uint8_t* acc_present;  // [A] the account appears among the pending or running jobs
  PrioBounds* bounds;
  double* acc_val;        // [A]
  double* terms;          // [R] service_val * run_time of the running jobs, in account-CSR order
  double* prio;           // [J]
  u64* keys;              // [J] sort keys (ascending = descending priority)
};

__device__ __forceinline__ double prio_cpu_double(i64 raw) { return (double)raw / 256.0; }  // PublicHeader.cpp:509-511

// k_prio_bounds: one pass over the pending and the running jobs (CalculateFactorBound_ :7663-7713).
__global__ __launch_bounds__(256) void k_prio_bounds(const PrioParams P) {
  u64 age_max = 0, age_min = ~0ull, mem_max = 0, mem_min = ~0ull, c_max = 0, c_min = ~0ull;
  u32 qos_max = 0, qos_min = ~0u, part_max = 0, part_min = ~0u, nn_max = 0, nn_min = ~0u;
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < P.J; i += stride) {
    u64 age = (u64)(P.now - P.submit[i]);
    age = age < P.max_age ? age : P.max_age;
    age_max = age > age_max ? age : age_max; age_min = age < age_min ? age : age_min;
    const u64 m = P.mem[i];
    mem_max = m > mem_max ? m : mem_max; mem_min = m < mem_min ? m : mem_min;
    const u64 cb = (u64)__double_as_longlong(prio_cpu_double(P.cpu_raw[i]));
    c_max = cb > c_max ? cb : c_max; c_min = cb < c_min ? cb : c_min;
    const u32 q = P.qos[i], pp = P.part[i], nn = P.node_num[i];
    qos_max = q > qos_max ? q : qos_max; qos_min = q < qos_min ? q : qos_min;
    part_max = pp > part_max ? pp : part_max; part_min = pp < part_min ? pp : part_min;
    nn_max = nn > nn_max ? nn : nn_max; nn_min = nn < nn_min ? nn : nn_min;
  }
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < P.R; i += stride) {
    const u64 m = P.r_mem[i];
    mem_max = m > mem_max ? m : mem_max; mem_min = m < mem_min ? m : mem_min;
    const u64 cb = (u64)__double_as_longlong(prio_cpu_double(P.r_cpu_raw[i]));
    c_max = cb > c_max ? cb : c_max; c_min = cb < c_min ? cb : c_min;
    const u32 q = P.r_qos[i], pp = P.r_part[i], nn = P.r_node_num[i];
    qos_max = q > qos_max ? q : qos_max; qos_min = q < qos_min ? q : qos_min;
    part_max = pp > part_max ? pp : part_max; part_min = pp < part_min ? pp : part_min;
    nn_max = nn > nn_max ? nn : nn_max; nn_min = nn < nn_min ? nn : nn_min;
  }
  // wave reduction on the DPP crossbar -> block fold through LDS -> one set of atomics per block
  age_max = wave_max_u64(age_max); age_min = wave_min_u64(age_min);
  mem_max = wave_max_u64(mem_max); mem_min = wave_min_u64(mem_min);
  c_max = wave_max_u64(c_max); c_min = wave_min_u64(c_min);
  qos_max = wave_umax32(qos_max); qos_min = wave_umin32(qos_min);
  part_max = wave_umax32(part_max); part_min = wave_umin32(part_min);
  nn_max = wave_umax32(nn_max); nn_min = wave_umin32(nn_min);
  __shared__ u64 s64[4][6];
  __shared__ u32 s32[4][6];
  const u32 wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    s64[wv][0] = age_max; s64[wv][1] = age_min; s64[wv][2] = mem_max; s64[wv][3] = mem_min; s64[wv][4] = c_max; s64[wv][5] = c_min;
    s32[wv][0] = qos_max; s32[wv][1] = qos_min; s32[wv][2] = part_max; s32[wv][3] = part_min; s32[wv][4] = nn_max; s32[wv][5] = nn_min;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const u32 f = threadIdx.x;
    const bool is_max = (f & 1u) == 0;
    u64 a = s64[0][f];
    u32 b = s32[0][f];
    for (u32 w = 1; w < 4; ++w) {
      a = is_max ? (s64[w][f] > a ? s64[w][f] : a) : (s64[w][f] < a ? s64[w][f] : a);
      b = is_max ? (s32[w][f] > b ? s32[w][f] : b) : (s32[w][f] < b ? s32[w][f] : b);
    }
    PrioBounds* B = P.bounds;
    unsigned long long* p64 = f == 0 ? (unsigned long long*)&B->age_max : f == 1 ? (unsigned long long*)&B->age_min
                            : f == 2 ? (unsigned long long*)&B->mem_max : f == 3 ? (unsigned long long*)&B->mem_min
                            : f == 4 ? (unsigned long long*)&B->cpus_max_bits : (unsigned long long*)&B->cpus_min_bits;
    u32* p32 = f == 0 ? &B->qos_max : f == 1 ? &B->qos_min : f == 2 ? &B->part_max : f == 3 ? &B->part_min
             : f == 4 ? &B->nn_max : &B->nn_min;
    if (is_max) { atomicMax(p64, (unsigned long long)a); atomicMax(p32, b); }
    else { atomicMin(p64, (unsigned long long)a); atomicMin(p32, b); }
  }
}

// Service values (:7715-7746).  The term of a running job (service_val * run_time) does not depend on the
// order, the fp64 SUM of an account does: k_prio_terms computes the terms in parallel, laid out in account-CSR
// order (x-th running job of the account, vector order kept); k_prio_service then adds each account's
// contiguous run front to back, one thread per account (independent loads, only the adds are serial).
__global__ __launch_bounds__(256) void k_prio_terms(const PrioParams P) {
  const u32 x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= P.R) return;
  const PrioBounds B = *P.bounds;
  const double cpus_max = __longlong_as_double((long long)B.cpus_max_bits);
  const double cpus_min = __longlong_as_double((long long)B.cpus_min_bits);
  const u32 i = P.acc_jobs[x];
  double service_val = 0;
  if (cpus_max > cpus_min) service_val += 1.0 * (prio_cpu_double(P.r_cpu_raw[i]) - cpus_min) / (cpus_max - cpus_min);
  else service_val += 1.0;
  if (B.nn_max > B.nn_min) service_val += 1.0 * (P.r_node_num[i] - B.nn_min) / (B.nn_max - B.nn_min);
  else service_val += 1.0;
  if (B.mem_max > B.mem_min) service_val += 1.0 * (double)(P.r_mem[i] - B.mem_min) / (double)(B.mem_max - B.mem_min);
  else service_val += 1.0;
  const u64 run_time = (u64)(P.now - P.r_start[i]);
  P.terms[x] = service_val * (double)run_time;
}
__global__ __launch_bounds__(256) void k_prio_service(const PrioParams P) {
  const u32 a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= P.A) return;
  double acc = 0.0;
  const u32 b = P.acc_off[a], e = P.acc_off[a + 1];
  u32 x = b;
  for (; x + 8 <= e; x += 8) {  // eight loads in flight, adds strictly in order
    const double t0 = P.terms[x], t1 = P.terms[x + 1], t2 = P.terms[x + 2], t3 = P.terms[x + 3];
    const double t4 = P.terms[x + 4], t5 = P.terms[x + 5], t6 = P.terms[x + 6], t7 = P.terms[x + 7];
    acc += t0; acc += t1; acc += t2; acc += t3; acc += t4; acc += t5; acc += t6; acc += t7;
  }
  for (; x < e; ++x) acc += P.terms[x];
  P.acc_val[a] = acc;
}
__global__ __launch_bounds__(256) void k_prio_service_bounds(const PrioParams P) {
  __shared__ double s_max[256], s_min[256];
  double mx = 0.0, mn = 4294967295.0;  // :7657-7658 (service_val_min starts at uint32 max)
  for (u32 a = threadIdx.x; a < P.A; a += blockDim.x)
    if (P.acc_present[a]) {
      const double v = P.acc_val[a];
      mx = v > mx ? v : mx;   // std::max(ser_val, max)
      mn = v < mn ? v : mn;   // std::min(ser_val, min)
    }
  s_max[threadIdx.x] = mx; s_min[threadIdx.x] = mn;
  __syncthreads();
  for (u32 w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      s_max[threadIdx.x] = s_max[threadIdx.x + w] > s_max[threadIdx.x] ? s_max[threadIdx.x + w] : s_max[threadIdx.x];
      s_min[threadIdx.x] = s_min[threadIdx.x + w] < s_min[threadIdx.x] ? s_min[threadIdx.x + w] : s_min[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { P.bounds->sv_max = s_max[0]; P.bounds->sv_min = s_min[0]; }
}

// k_prio_calc: CalculatePriority_ (:7754-7817) per pending job + the sort key.
__global__ __launch_bounds__(256) void k_prio_calc(const PrioParams P) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.J) return;
  const PrioBounds B = *P.bounds;
  const double cpus_max = __longlong_as_double((long long)B.cpus_max_bits);
  const double cpus_min = __longlong_as_double((long long)B.cpus_min_bits);
  double priority = P.cached ? P.cached[i] : 0.0;
  if (priority == 0.0) {  // :7616
    u64 job_age = (u64)(P.now - P.submit[i]);
    job_age = job_age < P.max_age ? job_age : P.max_age;
    const u32 q = P.qos[i], pp = P.part[i], nn = P.node_num[i];
    const u64 m = P.mem[i];
    const double c = prio_cpu_double(P.cpu_raw[i]);
    double qos_factor = 0, age_factor = 0, partition_factor = 0, job_size_factor = 0, fair_share_factor = 0;
    if (B.age_max > B.age_min) age_factor = 1.0 * (double)(job_age - B.age_min) / (double)(B.age_max - B.age_min);
    if (B.qos_max > B.qos_min) qos_factor = 1.0 * (q - B.qos_min) / (B.qos_max - B.qos_min);
    if (B.part_max > B.part_min) partition_factor = 1.0 * (pp - B.part_min) / (B.part_max - B.part_min);
    if (cpus_max > cpus_min) job_size_factor += 1.0 * (c - cpus_min) / (cpus_max - cpus_min);
    if (B.nn_max > B.nn_min) job_size_factor += 1.0 * (nn - B.nn_min) / (B.nn_max - B.nn_min);
    if (B.mem_max > B.mem_min) job_size_factor += 1.0 * (double)(m - B.mem_min) / (double)(B.mem_max - B.mem_min);
    if (P.favor_small) job_size_factor = 1.0 - job_size_factor / 3;
    else job_size_factor /= 3.0;
    if (B.sv_max > B.sv_min) fair_share_factor = 1.0 - (P.acc_val[P.account[i]] - B.sv_min) / (B.sv_max - B.sv_min);
    priority = P.w_age * age_factor + P.w_part * partition_factor + P.w_size * job_size_factor +
               P.w_fair * fair_share_factor + P.w_qos * qos_factor;
  }
  P.prio[i] = priority;
  // order-preserving u64 image of the double, inverted: ascending keys = descending priority
  const u64 b = (u64)__double_as_longlong(priority);
  const u64 asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  P.keys[i] = ~asc;
}

}  // namespace cns
