// What the adapter's test drivers (test_*_adapter.cpp) share: the failure count behind CHECK, the byte unit, the generator of the
// random cases and of the --bench inputs, the median of the timed repeats.  The node() and job() builders differ per driver and stay there.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("CHECK failed line %d: %s\n", __LINE__, #c); ++g_fail; } } while (0)

static const uint64_t G = 1ull << 30;

struct Rng {
  uint64_t x;
  uint64_t operator()() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
};

inline double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
