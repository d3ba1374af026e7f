// CPU test of the CSR checks of the callers' lists (cranesched_amd/csrc/csr_host.inc): the offsets verdicts and the per-list
// sort-and-check pass, on hand cases and against std::sort / std::adjacent_find / std::max_element over seeded random CSRs.
// Build: g++ -O1 -std=c++17 -Wall -Werror tests/cpp/csr_host_test.cpp -o csr_host_test
#include <cstdio>
#include <random>
#include <vector>

#include "../../cranesched_amd/csrc/csr_host.inc"

using namespace cns_csr;
typedef uint32_t u32;
typedef uint64_t u64;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

template <class Off>
static void offsets_cases() {
  auto is = [](std::vector<Off> off, Offsets what, u64 index) {
    const OffsetsVerdict v = check_offsets(off.data(), off.size() - 1);
    const u64 n = off.size() - 1, d = first_decrease(off.data(), n);
    return v.what == what && (what != Offsets::Decreases || (v.index == index && d == index)) && (what != Offsets::Ok || d == n);
  };
  CHECK(is({0}, Offsets::Ok, 0));                      // n = 0
  CHECK(is({3}, Offsets::FirstNot0, 0));
  CHECK(is({0, 2, 5, 9}, Offsets::Ok, 0));
  CHECK(is({0, 0, 0, 4, 4, 4}, Offsets::Ok, 0));       // empty lists
  CHECK(is({1, 2, 5, 9}, Offsets::FirstNot0, 0));
  CHECK(is({1, 0, 5, 9}, Offsets::FirstNot0, 0));      // the first offset is reported before a decrease ...
  { const std::vector<Off> off = {1, 0, 5, 9}; CHECK(first_decrease(off.data(), 3) == 0); }   // ... which first_decrease still finds
  CHECK(is({0, 4, 3, 9, 9}, Offsets::Decreases, 1));   // middle
  CHECK(is({0, 4, 6, 9, 8}, Offsets::Decreases, 3));   // last index
  CHECK(is({0, 4, 3, 2, 1}, Offsets::Decreases, 1));   // the first of several
  { const std::vector<Off> off = {5, 3, 4}; CHECK(first_decrease(off.data(), 2) == 0); }      // first index (a table that does not start at 0)
  { const std::vector<Off> off = {0, 7, 3}; CHECK(check_offsets(off.data(), 2).what == Offsets::Decreases && check_offsets(off.data(), 2).index == 1 && check_offsets(off.data(), 1).what == Offsets::Ok); }
}

struct Csr {
  std::vector<u64> off;
  std::vector<u32> val;
};
static Csr make(const std::vector<std::vector<u32>>& lists) {
  Csr c;
  c.off.push_back(0);
  for (const auto& l : lists) { c.val.insert(c.val.end(), l.begin(), l.end()); c.off.push_back(c.val.size()); }
  return c;
}

// the verdict by the standard library: per list in order, the least value that is >= bound or repeated, a bound breach first at a tie
static ListsVerdict reference(const Csr& c, u64 beg, u64 end, u64 bound) {
  for (u64 l = beg; l < end; ++l) {
    std::vector<u32> s(c.val.begin() + c.off[l], c.val.begin() + c.off[l + 1]);
    if (s.empty()) continue;
    std::sort(s.begin(), s.end());
    const auto rep = std::adjacent_find(s.begin(), s.end());
    const bool over = *std::max_element(s.begin(), s.end()) >= bound;
    const u32 first_over = over ? *std::lower_bound(s.begin(), s.end(), bound, [](u32 a, u64 b) { return a < b; }) : 0;
    if (over && (rep == s.end() || first_over <= *rep)) return {Lists::OutOfBound, l, first_over};
    if (rep != s.end()) return {Lists::Repeated, l, *rep};
  }
  return {Lists::Ok, 0, 0};
}

// runs the pass over [beg, end) and holds it to the reference: the verdict, the source untouched, the output sorted for every list
// before the offending one and untouched outside [beg, end)
static ListsVerdict run(const Csr& c, u64 beg, u64 end, u64 bound, int line) {
  const u32 kMark = 0xDEADBEEFu;
  const std::vector<u32> src = c.val;
  std::vector<u32> dst(c.val.size(), kMark);
  const ListsVerdict v = bound == kNoBound ? sort_lists(c.off.data(), c.val.data(), dst.data(), beg, end) : sort_lists(c.off.data(), c.val.data(), dst.data(), beg, end, bound);
  const ListsVerdict r = reference(c, beg, end, bound);
  bool ok = v.what == r.what && (v.what == Lists::Ok || (v.list == r.list && v.value == r.value)) && src == c.val;
  const u64 lists = c.off.size() - 1, sorted_to = v.what == Lists::Ok ? end : v.list;
  for (u64 l = 0; l < lists && ok; ++l) {
    std::vector<u32> want(c.val.begin() + c.off[l], c.val.begin() + c.off[l + 1]);
    if (l >= beg && l < sorted_to) std::sort(want.begin(), want.end());
    else if (l < beg || l >= end) want.assign(want.size(), kMark);
    else continue;   // the offending list and those behind it inside the range: unspecified
    ok = std::equal(want.begin(), want.end(), dst.begin() + c.off[l]);
  }
  if (!ok) { printf("FAIL line %d: verdict %d list %llu value %u, reference %d list %llu value %u\n", line, (int)v.what, (unsigned long long)v.list, v.value,
                    (int)r.what, (unsigned long long)r.list, r.value); ++g_fail; }
  return v;
}
#define RUN(c, beg, end, bound) run(c, beg, end, bound, __LINE__)

static void lists_cases() {
  std::vector<u32> big(300);
  for (u32 i = 0; i < 300; ++i) big[i] = (i * 7919u) % 1000u;   // 300 distinct values below 1000, unsorted
  {
    const Csr c = make({{}, {7}, {9, 2}, big, {}});
    CHECK(RUN(c, 0, 5, kNoBound).what == Lists::Ok);
    CHECK(RUN(c, 0, 5, 1000).what == Lists::Ok);
    const ListsVerdict eq = RUN(c, 0, 5, 9);                    // a value equal to the bound
    CHECK(eq.what == Lists::OutOfBound && eq.list == 2 && eq.value == 9);
    const ListsVerdict ab = RUN(c, 0, 5, 8);                    // ... and one above it
    CHECK(ab.what == Lists::OutOfBound && ab.list == 2 && ab.value == 9);
    CHECK(RUN(c, 0, 2, 8).what == Lists::Ok);                   // the range ends before the offending list
    CHECK(RUN(c, 3, 5, 8).what == Lists::OutOfBound);
    CHECK(RUN(c, 1, 3, kNoBound).what == Lists::Ok);            // a range over some lists leaves the others' output alone
    CHECK(RUN(c, 2, 2, kNoBound).what == Lists::Ok);            // an empty range
  }
  for (u32 at : {0u, 150u, 299u}) {                             // a repeat of the least, a middle and the largest value of the long list
    std::vector<u32> s = big;
    std::sort(s.begin(), s.end());
    std::vector<u32> l = big;
    l[(size_t)(std::find(big.begin(), big.end(), s[at]) - big.begin() + 1) % 300] = s[at];   // its neighbour in the list names it again
    const Csr c = make({{1}, l, {5, 5}});
    const ListsVerdict v = RUN(c, 0, 3, kNoBound);
    CHECK(v.what == Lists::Repeated && v.list == 1 && v.value == s[at]);
    CHECK(RUN(c, 0, 1, kNoBound).what == Lists::Ok);
    const ListsVerdict w = RUN(c, 2, 3, kNoBound);              // a list of two equal entries
    CHECK(w.what == Lists::Repeated && w.list == 2 && w.value == 5);
  }
  {
    const Csr c = make({{4, 1, 4}, {3, 3, 9}, {9, 9}});
    const ListsVerdict v = RUN(c, 0, 3, 9);                     // the first list's repeat comes first
    CHECK(v.what == Lists::Repeated && v.list == 0 && v.value == 4);
    const ListsVerdict w = RUN(c, 1, 3, 9);                     // a repeat below the bound before a value at it
    CHECK(w.what == Lists::Repeated && w.list == 1 && w.value == 3);
    const ListsVerdict x = RUN(c, 2, 3, 9);                     // a repeated value that is itself out of bound: the bound speaks
    CHECK(x.what == Lists::OutOfBound && x.list == 2 && x.value == 9);
  }
  std::mt19937_64 rng(7);
  for (int it = 0; it < 200; ++it) {
    std::vector<std::vector<u32>> lists(rng() % 9);
    for (auto& l : lists) { l.resize(rng() % 13); for (u32& v : l) v = (u32)(rng() % 16); }
    const Csr c = make(lists);
    const u64 n = lists.size(), beg = rng() % (n + 1), end = beg + rng() % (n - beg + 1);
    RUN(c, 0, n, kNoBound);
    RUN(c, 0, n, 8 + rng() % 10);
    RUN(c, beg, end, rng() % 2 ? kNoBound : 12);
    CHECK(check_offsets(c.off.data(), n).what == Offsets::Ok);
  }
  {
    const std::vector<u32> off = {0, 2, 2, 5}, val = {8, 3, 6, 1, 6};   // 32-bit offsets (the partition lists of the validity check)
    std::vector<u32> dst(5, 0);
    const ListsVerdict v = sort_lists(off.data(), val.data(), dst.data(), 0, 3);
    CHECK(v.what == Lists::Repeated && v.list == 2 && v.value == 6 && dst[0] == 3 && dst[1] == 8);
  }
}

int main() {
  offsets_cases<u32>();
  offsets_cases<u64>();
  lists_cases();
  if (g_fail) return 1;
  printf("ok\n");
  return 0;
}
