// xa_select_asan.cpp — xa_pri_idx and xa_over_cap (bwa-flow_amd/csrc/pure.h), the
// per-region arithmetic of bwagpu_xa_select_device, under the host sanitizers.
// Stand-alone: no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/xa_select_asan.cpp -o xa_select_asan && ./xa_select_asan
//
// Checked:
//  * the comparison is the reference's (bwa/bwamem_extra.c:90-95): a float option
//    in a double parameter, for every pair of scores in [0, 1023] under 0.8f, 0.5f
//    and 1.0f against that expression written out with a volatile double, and
//    decided in integers where the float is exact;
//  * 80 under 100 is dropped at 0.8f and 81 is kept;
//  * a secondary_all at the ends of int, at -1 and at n never indexes the array
//    (ASan: the array is exactly n records) and joins nothing; scores at the
//    ends of int raise no UBSan report;
//  * the caps (bwamem_extra.c:118) over every count around both limits.
#include <climits>
#include <cstdio>
#include <vector>

#include "pure.h"

using namespace bwagpu;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

int main() {
  const float ratios[] = {0.8f, 0.5f, 1.0f};
  for (float rf : ratios) {
    volatile double rd = rf;  // what get_pri_idx's parameter holds
    std::vector<bwagpu_alnreg_t> a(2);
    a[1].secondary_all = 0;
    a[0].secondary_all = -1;
    for (int p = 0; p < 1024; ++p)
      for (int s = 0; s < 1024; ++s) {
        a[0].score = p, a[1].score = s;
        const bool want = s >= p * rd;
        EXPECT((xa_pri_idx(rf, a.data(), 2, 1) == 0) == want);
        if (rf == 0.5f) EXPECT(want == (2 * s >= p));
        if (rf == 1.0f) EXPECT(want == (s >= p));
        if (rf == 0.8f) EXPECT(want == (5 * s > 4 * p || p == 0));  // 0.8f is above 4/5
        EXPECT(xa_pri_idx(rf, a.data(), 2, 0) == -1);
      }
  }
  {
    std::vector<bwagpu_alnreg_t> a(3);
    a[0].score = 100, a[1].score = 80, a[2].score = 81;
    a[0].secondary_all = -1, a[1].secondary_all = a[2].secondary_all = 0;
    EXPECT(xa_pri_idx(0.8f, a.data(), 3, 1) == -1 && xa_pri_idx(0.8f, a.data(), 3, 2) == 0);
    for (int k : {INT_MIN, -2, -1, 3, 4, INT_MAX}) {
      a[1].secondary_all = k;
      EXPECT(xa_pri_idx(0.8f, a.data(), 3, 1) == -1);
    }
    a[1].secondary_all = 2;
    for (int s : {INT_MIN, -1, 0, INT_MAX})
      for (int p : {INT_MIN, -1, 0, INT_MAX}) {
        a[1].score = s, a[2].score = p;
        EXPECT((xa_pri_idx(0.8f, a.data(), 3, 1) == 2) == ((double)s >= (double)p * (double)0.8f));
      }
  }
  for (int mx = 0; mx <= 6; ++mx)
    for (int mx_alt = 0; mx_alt <= 8; ++mx_alt)
      for (int cnt = 0; cnt <= 10; ++cnt)
        for (int alt = 0; alt < 2; ++alt)
          EXPECT(xa_over_cap(cnt, alt != 0, mx, mx_alt) == (cnt > mx_alt || (!alt && cnt > mx)));
  EXPECT(!xa_over_cap(5, false, 5, 200) && xa_over_cap(6, false, 5, 200) && !xa_over_cap(6, true, 5, 200) &&
         !xa_over_cap(200, true, 5, 200) && xa_over_cap(201, true, 5, 200));
  if (g_fail) return 1;
  std::printf("xa_select_asan OK\n");
  return 0;
}
