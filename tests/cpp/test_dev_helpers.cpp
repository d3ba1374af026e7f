// CPU unit test of the engine's host-compilable device helpers (cranesched_amd/csrc/res_dev.h,
// pq_emul.h) against the oracle's MaskAlgebra and the real std::priority_queue.  feasible / feasible_counts run over the GRES
// layouts of tests/gres_wide.py (a 64-slot class, 8 classes under 4 names, uneven widths ending at bit 63) and random ones,
// with requests around 15 / 16 / the class width / 64 / 127 / 128 / 255.
// csr_owner / sorted_contains (csr_dev.h) run against std::upper_bound / std::binary_search, with 32-bit and 64-bit offsets.
// Build: g++ -O1 -std=c++20 tests/cpp/test_dev_helpers.cpp -o tests/cpp/test_dev_helpers
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <initializer_list>
#include <random>
#include <utility>
#include <vector>

#include "../../cranesched_amd/csrc/csr_dev.h"
#include "../../cranesched_amd/csrc/pq_emul.h"
#include "../../oracle/res_algebra.hpp"

using namespace cns;

static GresDev make_dev(const ora::GresLayout& L) {
  GresDev d{};
  d.num_classes = L.num_classes;
  for (u32 c = 0; c < L.num_classes; ++c) {
    d.class_mask[c] = L.class_mask(c);
    d.class_name_packed |= (u32)L.class_name[c] << (4 * c);
    d.name_mask[L.class_name[c]] |= L.class_mask(c);
    d.name_bytes[L.class_name[c]] |= 0xFFull << (8 * c);
  }
  return d;
}

struct node_info {  // JobScheduler.cpp:6157-6164
  int ntasks_on_node;
  int id;
  bool operator<(const node_info& o) const { return ntasks_on_node > o.ntasks_on_node; }
};

static ora::GresLayout layout_of(std::initializer_list<int> name, std::initializer_list<int> shift, std::initializer_list<int> width) {
  ora::GresLayout L;
  L.num_classes = (u32)name.size();
  u32 g = 0;
  for (int v : name) L.class_name[g++] = (uint8_t)v;
  g = 0;
  for (int v : shift) L.class_shift[g++] = (uint8_t)v;
  g = 0;
  for (int v : width) L.class_width[g++] = (uint8_t)v;
  return L;
}

// 1..8 classes under 1..4 names, widths 1..64, no overlaps, class order shuffled against bit order
static ora::GresLayout random_layout(std::mt19937_64& rng) {
  ora::GresLayout L;
  const u32 C = 1 + (u32)(rng() % 8);
  int w[8], used = 0;
  for (u32 c = 0; c < C; ++c) { w[c] = 1; ++used; }
  for (u32 c = 0; c < C && used < 64; ++c) { const int add = (int)(rng() % (u64)(64 - used + 1)) * (int)(rng() % 2); w[c] += add; used += add; }
  int gap = 64 - used, pos = 0, perm[8];
  for (u32 c = 0; c < C; ++c) perm[c] = (int)c;
  for (u32 c = C; c > 1; --c) std::swap(perm[c - 1], perm[rng() % c]);
  const u32 names = 1 + (u32)(rng() % 4);
  for (u32 c = 0; c < C; ++c) {
    const int skip = gap ? (int)(rng() % (u64)(gap + 1)) : 0;
    gap -= skip; pos += skip;
    const int g = perm[c];
    L.class_shift[g] = (uint8_t)pos; L.class_width[g] = (uint8_t)w[c]; L.class_name[g] = (uint8_t)(rng() % names);
    pos += w[c];
  }
  L.num_classes = C;
  return L;
}

static u64 lowest_n_ref(u64 x, int n) {
  u64 out = 0;
  for (int b = 0; b < 64 && n > 0; ++b)
    if ((x >> b) & 1ull) { out |= 1ull << b; --n; }
  return out;
}

// a slot count near the edges of the 4-bit / 7-bit / 8-bit forms of the hot path, or small
static u32 edge_count(std::mt19937_64& rng, u32 w) {
  static const u32 e[] = {1, 2, 3, 7, 8, 14, 15, 16, 17, 63, 64, 65, 127, 128, 255};
  switch (rng() % 4) {
    case 0: return e[rng() % (sizeof(e) / sizeof(e[0]))];
    case 1: { const u32 v = w - 1 + (u32)(rng() % 3); return v == 0 ? 1 : v > 255 ? 255 : v; }   // the width, one less, one more
    default: return 1 + (u32)(rng() % (w < 20 ? w : 20));
  }
}

// every flat index of an offsets table (list lengths given) against std::upper_bound over the first n offsets
template <class Off>
static bool owner_ok(const std::vector<u32>& len) {
  std::vector<Off> off(len.size() + 1, 0);
  for (size_t l = 0; l < len.size(); ++l) off[l + 1] = off[l] + len[l];
  const u32 n = (u32)len.size();
  for (Off i = 0; i < off[n]; ++i) {
    const u32 want = (u32)(std::upper_bound(off.begin(), off.begin() + n, i) - off.begin()) - 1;
    if (csr_owner(off.data(), n, i) != want || off[want] > i || off[want + 1] <= i) return false;
  }
  return true;
}

// every x from below the least to above the largest element of the ascending a[b, e), inside a longer array
template <class Off>
static bool contains_ok(const std::vector<u32>& a, Off b, Off e) {
  const u32 lo = b < e ? a[b] - 1 : 0, hi = b < e ? a[e - 1] + 1 : 4;
  for (u32 x = lo; x <= hi; ++x)
    if (sorted_contains(a.data(), b, e, x) != std::binary_search(a.begin() + b, a.begin() + e, x)) return false;
  return true;
}

static int test_csr() {
  std::mt19937_64 rng(20250612);
  std::vector<std::vector<u32>> tables = {
      {5}, {1}, {4, 0, 0, 0}, {0, 0, 0, 4}, {0, 0, 3, 2}, {2, 0, 0, 0, 3}, {2, 3, 0, 0}, {0, 0, 1, 0, 0, 2, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 1, 1}};
  for (int it = 0; it < 500; ++it) {
    std::vector<u32> len(1 + rng() % 9);
    for (u32& l : len) l = rng() % 3 ? (u32)(rng() % 21) : 0;
    tables.push_back(len);
  }
  for (size_t t = 0; t < tables.size(); ++t)
    if (!owner_ok<u32>(tables[t]) || !owner_ok<u64>(tables[t])) { printf("FAIL csr_owner table=%zu\n", t); return 1; }
  for (u32 len : {0u, 1u, 2u, 3u, 4u, 7u, 8u}) {
    std::vector<u32> a = {1, 3};   // two entries in front of the range and two behind it that the search must not see
    for (u32 i = 0; i < len; ++i) a.push_back(10 + 3 * i + (u32)(rng() % 3));
    a.push_back(10); a.push_back(11);
    if (!contains_ok<u32>(a, 2u, 2u + len) || !contains_ok<u64>(a, (u64)2, (u64)2 + len)) { printf("FAIL sorted_contains len=%u\n", len); return 1; }
  }
  return 0;
}

int main() {
  if (test_csr()) return 1;
  std::mt19937_64 rng(12345);
  std::vector<std::pair<ora::GresLayout, int>> layouts = {
      {layout_of({0, 0, 1}, {0, 4, 8}, {4, 4, 8}), 400000},                                         // tests/helpers.py: 16 slots
      {layout_of({0}, {0}, {64}), 100000},                                                          // one class of 64 (bit 63)
      {layout_of({3, 0, 2, 1, 0, 3, 1, 2}, {56, 8, 40, 0, 24, 48, 16, 32}, {8, 8, 8, 8, 8, 8, 8, 8}), 100000},  // 8 x 8, 4 names
      {layout_of({0, 1, 0, 0, 2}, {0, 2, 20, 26, 43}, {1, 17, 5, 16, 21}), 100000}};               // uneven, gaps, ends at 63
  for (int i = 0; i < 40; ++i) layouts.push_back({random_layout(rng), 10000});
  long nfeas = 0, nfail = 0;
  for (size_t li = 0; li < layouts.size(); ++li) {
    const ora::GresLayout& L = layouts[li].first;
    const bool small = li == 0;   // the original 16-slot stream
    GresDev D = make_dev(L);
    ora::MaskAlgebra A(&L);
    u64 full = 0;
    for (u32 c = 0; c < L.num_classes; ++c) full |= L.class_mask(c);
    for (int it = 0; it < layouts[li].second; ++it) {
      Res a;
      a.cpu = (i64)(rng() % 40) * 128;
      a.mem = rng() % 64;
      a.clo = (rng() % 4 == 0) ? 0 : (rng() & rng() & 0xFFFF);
      a.chi = (rng() % 8 == 0) ? (rng() & 0xF) : 0;
      a.c2 = (rng() % 8 == 0) ? (rng() & 0x3F) : 0;      // core ids 128..255 (ABI 3)
      a.c3 = (rng() % 16 == 0) ? (rng() & 0x7) : 0;
      Req q;
      q.cpu = (i64)(rng() % 12) * 128;
      q.mem = rng() % 48;
      q.gtot = 0; q.gspec = 0;
      if (small) {
        a.gres = rng() & rng() & 0xFFFF;
        if (rng() % 2) {
          q.gtot = (u32)(rng() % 5) | ((u32)(rng() % 6) << 8);
          if (rng() % 2) q.gspec = (rng() % 3) | ((rng() % 3) << 8) | ((rng() % 4) << 16);
        }
      } else {
        const u32 st = (u32)(rng() % 4);
        a.gres = st == 0 ? full : st == 1 ? (full & (rng() | rng())) : st == 2 ? (full & rng()) : (full & rng() & rng());
        const int nreq = (int)(rng() % 3);
        u32 tot[4] = {0, 0, 0, 0}, spec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = 0; r < nreq; ++r) {
          const u32 c = (u32)(rng() % L.num_classes), nm = L.class_name[c];
          const u32 nw = (u32)__builtin_popcountll(L.name_mask(nm));
          switch (rng() % 4) {
            case 0: tot[nm] = edge_count(rng, nw); break;                                          // untyped
            case 1: spec[c] = edge_count(rng, L.class_width[c]); if (tot[nm] < spec[c]) tot[nm] = spec[c]; break;  // typed
            case 2: spec[c] = edge_count(rng, L.class_width[c]); tot[nm] = spec[c] + 1 + (u32)(rng() % 20); break;  // typed + untyped
            default: spec[c] = edge_count(rng, L.class_width[c]); break;                           // typed, no total
          }
        }
        for (int n = 0; n < 4; ++n) q.gtot |= (tot[n] > 255 ? 255u : tot[n]) << (8 * n);
        for (int g = 0; g < 8; ++g) q.gspec |= (u64)(spec[g] > 255 ? 255u : spec[g]) << (8 * g);
      }
      ora::ReqView v;
      v.cpu = q.cpu; v.mem = q.mem;
      for (int i = 0; i < 4; ++i) v.gtot[i] = (q.gtot >> (8 * i)) & 0xFF;
      for (int i = 0; i < 8; ++i) v.gspec[i] = (q.gspec >> (8 * i)) & 0xFF;
      ora::MaskRes am; am.cpu = a.cpu; am.mem = a.mem; am.clo = a.clo; am.chi = a.chi; am.gres = a.gres; am.c2 = a.c2; am.c3 = a.c3;
      ora::MaskRes om;
      Res od;
      bool r1 = A.feasible(v, am, &om);
      bool r2 = feasible(q, a, od, D);
      u64 cnt = 0;   // per-class slot counts, one byte per class (what class_counts hands feasible_counts)
      for (u32 g = 0; g < L.num_classes; ++g) {
        u32 k = 0;
        for (int b = 0; b < 64; ++b) k += (u32)(((a.gres & L.class_mask(g)) >> b) & 1ull);
        cnt |= (u64)k << (8 * g);
      }
      bool r3 = feasible_counts(q, a.cpu, a.mem, cores_count(a), cnt, D);
      if (r1 != r2 || r1 != r3) {
        printf("FAIL feasible truth layout=%zu it=%d %d %d %d gtot=%08x gspec=%016llx gres=%016llx\n", li, it, r1, r2, r3, q.gtot,
               (unsigned long long)q.gspec, (unsigned long long)a.gres);
        return 1;
      }
      if (r1 && !(om.cpu == od.cpu && om.mem == od.mem && om.clo == od.clo && om.chi == od.chi && om.c2 == od.c2 && om.c3 == od.c3 && om.gres == od.gres)) {
        printf("FAIL feasible alloc layout=%zu it=%d\n", li, it);
        return 1;
      }
      (r1 ? nfeas : nfail)++;
    }
  }
  // lowest_n over all 64 bits (a class that ends at bit 63, n up to 64 and beyond)
  for (int it = 0; it < 200000; ++it) {
    const u64 x = it % 5 == 0 ? ~0ull : (rng() | (it % 3 == 0 ? rng() : 0)) | (it % 2 ? 1ull << 63 : 0);
    const int n = (int)(rng() % 70);
    if (lowest_n(x, n) != lowest_n_ref(x, n)) { printf("FAIL lowest_n x=%016llx n=%d\n", (unsigned long long)x, n); return 1; }
  }
  // priority_queue emulation: random push / pop-when-over-k sequences with many ties
  for (int it = 0; it < 20000; ++it) {
    int k = 1 + (int)(rng() % 9);
    std::priority_queue<node_info> pq;
    std::vector<HeapEnt> H(k + 2);
    int hs = 0;
    int n = 1 + (int)(rng() % 40);
    for (int i = 0; i < n; ++i) {
      int cap = 1 + (int)(rng() % 3);
      pq.push(node_info{cap, i});
      H[hs] = HeapEnt{}; H[hs].ntasks = cap; H[hs].node = (u32)i; ++hs; pq_push(H.data(), hs);
      if ((int)pq.size() > k) {
        if (pq.top().id != (int)H[0].node) { printf("FAIL pq top it=%d\n", it); return 1; }
        pq.pop();
        pq_pop(H.data(), hs); --hs;
      }
    }
    while (!pq.empty()) {
      if (pq.top().id != (int)H[0].node || pq.top().ntasks_on_node != H[0].ntasks) { printf("FAIL pq drain it=%d\n", it); return 1; }
      pq.pop();
      pq_pop(H.data(), hs); --hs;
    }
  }
  printf("ok feasible=%ld infeasible=%ld\n", nfeas, nfail);
  return 0;
}
