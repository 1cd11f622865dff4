// side_sort_asan.cpp — the side lists' key prefix and short-run boundary
// (bwa-flow_amd/csrc/side_sort.h: the lane pieces the fused scatter runs, DESIGN.md
// §27) against a plain loop, under the host sanitizers.
// Stand-alone: no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I bwa-flow_amd/csrc
//       tests/cpp/side_sort_asan.cpp -o side_sort_asan && ./side_sort_asan
//
// Histograms: random ones (sparse, dense, large counts), all zero, and one key
// alone at every key; short_q = 0, 1, 63 and 255 (the largest key's query
// length: side_key maps everything from 255 bases on to key 0).  Every array is
// sized exactly, so a read or write past the 256 keys is a sanitizer error.
#include <cstdio>
#include <random>
#include <vector>

#include "side_sort.h"

using namespace bwagpu;

static int g_fail = 0;

static void check(const std::vector<int32_t>& hist, const char* what) {
  std::vector<int32_t> first(kSideKeys, -1), want(kSideKeys);
  int32_t run = 0;
  for (int k = 0; k < kSideKeys; ++k) {
    want[k] = run;
    run += hist[k];
  }
  side_prefix(hist.data(), first.data());
  bool ok = first == want;
  const int short_qs[] = {0, 1, 63, 255};
  for (int q : short_qs) {
    // the sides longer than q bases lie in front of the short run: a plain count over the query lengths
    int32_t longer = 0;
    for (int len = q + 1; len <= 255; ++len) longer += hist[255 - len];
    ok = ok && side_short_first(first.data(), q) == longer;
  }
  if (!ok && g_fail++ == 0) std::printf("FAIL %s\n", what);
}

int main() {
  for (int q = 0; q <= 300; ++q) {
    const int k = side_key(q);
    if (k != (q >= 255 ? 0 : 255 - q) && g_fail++ == 0) std::printf("FAIL side_key(%d) = %d\n", q, k);
  }
  std::mt19937 rng(20261021);
  std::vector<int32_t> h(kSideKeys, 0);
  h.shrink_to_fit();
  check(h, "all zero");
  for (int k = 0; k < kSideKeys; ++k) {
    std::vector<int32_t> one(kSideKeys, 0);
    one.shrink_to_fit();
    one[k] = 1 + (int32_t)(rng() % 100000u);
    check(one, "one key");
  }
  for (int it = 0; it < 4000; ++it) {
    const int kind = it % 4;
    for (auto& x : h)
      x = kind == 0 ? (rng() % 16u ? 0 : (int32_t)(rng() % 9u)) : kind == 1 ? (int32_t)(rng() % 300u)
          : kind == 2 ? (int32_t)(rng() % 4000000u) : (int32_t)(rng() % 2u);
    check(h, "random");
  }
  if (g_fail) return 1;
  std::printf("side_sort_asan OK\n");
  return 0;
}
