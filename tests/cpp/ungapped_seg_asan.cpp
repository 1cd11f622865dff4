// ungapped_seg_asan.cpp — the segment form of the ungapped certificate's scan
// (UngSeg / ungseg_combine, bwa-flow_amd/csrc/ungapped.h) against the serial
// UngappedScan on random score sequences, under the host sanitizers.
// Stand-alone: no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       -I bwa-flow_amd/csrc tests/cpp/ungapped_seg_asan.cpp -o ungapped_seg_asan && ./ungapped_seg_asan
//
// The sequences are those of tests/test_ungapped_seg.py's random comparison: 1
// .. 160 scores, cut at every multiple of 16, at random places and after every
// base, folded left- and right-nested.  Every array is sized exactly, so a
// read past the scores or the cuts is a sanitizer error.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "ungapped_seg_shim.cpp"

static int g_fail = 0;

static void check(const std::vector<int32_t>& s, int max_mat, const std::vector<int32_t>& cuts, const char* what) {
  int32_t want[4], got[5];
  ungseg_serial(s.data(), (int32_t)s.size(), max_mat, want);
  for (int order = 0; order < 2; ++order) {
    ungseg_fold(s.data(), (int32_t)s.size(), max_mat, cuts.data(), (int32_t)cuts.size(), order, got);
    const bool ok = got[0] == (int32_t)s.size() && got[1] == want[0] && got[2] == want[1] && got[3] == want[2] && got[4] == want[3];
    if (!ok && g_fail++ == 0)
      std::printf("FAIL %s, %zu scores, %zu cuts, order %d: got c %d P %d M %d am %d, the serial scan has %d %d %d %d\n", what,
                  s.size(), cuts.size(), order, got[1], got[2], got[3], got[4], want[0], want[1], want[2], want[3]);
  }
}

int main() {
  std::mt19937 rng(20261021);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };  // inclusive
  for (int it = 0; it < 6000; ++it) {
    const int n = rnd(1, 160), kind = it % 3;
    const int max_mat = kind == 1 ? 4 : 1;
    std::vector<int32_t> s(n);
    for (auto& x : s) x = kind == 0 ? (rnd(0, 9) ? 1 : (rnd(0, 1) ? -4 : -1)) : (kind == 1 ? rnd(-6, 4) : rnd(-1, 1));
    std::vector<int32_t> c16, call, crnd;
    for (int k = 16; k < n; k += 16) c16.push_back(k);
    for (int k = 1; k < n; ++k) call.push_back(k);
    for (int k = 1; k < n; ++k)
      if (rnd(0, 15) == 0) crnd.push_back(k);
    c16.shrink_to_fit(), call.shrink_to_fit(), crnd.shrink_to_fit(), s.shrink_to_fit();
    check(s, max_mat, c16, "every 16");
    check(s, max_mat, call, "every base");
    check(s, max_mat, crnd, "random cuts");
    check(s, max_mat, {}, "one segment");
  }
  if (g_fail) return 1;
  std::printf("ungapped_seg_asan OK\n");
  return 0;
}
