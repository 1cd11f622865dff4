// ungapped_asan.cpp — the ungapped certificate (bwa-flow_amd/csrc/ungapped.h)
// against the project's own ksw_extend2 (oracle/ksw_ext.c) on random short
// calls, under the host sanitizers.  Stand-alone: no GPU, no HIP, not loaded
// into any other process.
//
//   gcc -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I oracle -c oracle/ksw_ext.c -o ksw_ext.o
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I oracle
//       -I bwa-flow_amd/csrc tests/cpp/ungapped_asan.cpp ksw_ext.o -o ungapped_asan && ./ungapped_asan
//
// The calls are those of tests/test_ungapped_cert.py's random comparison: 1 ..
// 40 query bases, zero to three planted mismatches and Ns, targets that run
// past the query or stop short of it, under option sets that sit on the
// certificate's conditions.  Every pool is sized exactly, so a read past a
// query or a target is a sanitizer error.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "oracle.h"
#include "ungapped_shim.cpp"

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

struct Case {
  const char* name;
  int a, b, o_del, e_del, o_ins, e_ins, w, zdrop;
  bool matrix, none;  // a general matrix; nothing can be certified
};

static bwagpu_opt_t make_opt(const Case& c) {
  bwagpu_opt_t o;
  std::memset(&o, 0, sizeof o);
  o.a = c.a, o.b = c.b, o.o_del = c.o_del, o.e_del = c.e_del, o.o_ins = c.o_ins, o.e_ins = c.e_ins;
  o.pen_clip5 = o.pen_clip3 = 5, o.w = c.w, o.zdrop = c.zdrop;
  static const int8_t gen[25] = {3, -4, -2, -5, -1, -4, 2, -6, -3, -1, -2, -6, 4, -4, -2, -5, -3, -4, 3, -1, -1, -1, -2, -1, -1};
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j)  // bwa_fill_scmat (bwa.c:109-118)
      o.mat[i * 5 + j] = c.matrix ? gen[i * 5 + j] : (int8_t)(i == 4 || j == 4 ? -1 : (i == j ? c.a : -c.b));
  return o;
}

static void run_case(const Case& c, std::mt19937& rng) {
  const bwagpu_opt_t opt = make_opt(c);
  const int n = 3000;
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };  // inclusive
  std::vector<bwagpu_ext_task_t> tasks(n);
  std::vector<uint8_t> qp, tp;
  for (int k = 0; k < n; ++k) {
    const int ql = rnd(1, 40);
    std::vector<uint8_t> q(ql), t;
    for (auto& x : q) x = (uint8_t)rnd(0, 3);
    t = q;
    for (int m = rnd(0, 3); m > 0; --m) {
      const int p = rnd(0, ql - 1);
      t[p] = (uint8_t)((t[p] + rnd(1, 3)) & 3);
    }
    if (rnd(0, 9) < 4)
      for (int m = rnd(0, 3); m > 0; --m) q[rnd(0, ql - 1)] = 4;
    if (rnd(0, 7) == 0 && ql > 1) t.resize(rnd(1, ql - 1));
    else
      for (int m = rnd(0, 12); m > 0; --m) t.push_back((uint8_t)rnd(0, 3));
    tasks[k] = bwagpu_ext_task_t{(int64_t)qp.size(), (int64_t)tp.size(), ql, (int32_t)t.size(), c.w, rnd(0, 7), c.zdrop, rnd(1, 60)};
    qp.insert(qp.end(), q.begin(), q.end());
    tp.insert(tp.end(), t.begin(), t.end());
  }
  qp.shrink_to_fit();
  tp.shrink_to_fit();
  std::vector<bwagpu_ext_result_t> got(n), want(n);
  std::vector<uint8_t> cert(n);
  const int nc = ungapped_batch(&opt, n, tasks.data(), qp.data(), tp.data(), got.data(), cert.data());
  int bad = 0, short_cert = 0;
  for (int k = 0; k < n; ++k) {
    const bwagpu_ext_task_t& t = tasks[k];
    bwagpu_ext_result_t& r = want[k];
    r.score = oracle_ksw_extend2(t.qlen, qp.data() + t.qoff, t.tlen, tp.data() + t.toff, 5, opt.mat, opt.o_del, opt.e_del,
                                 opt.o_ins, opt.e_ins, t.w, t.end_bonus, t.zdrop, t.h0, &r.qle, &r.tle, &r.gtle,
                                 &r.gscore, &r.max_off, nullptr);
    if (!cert[k]) continue;
    if (std::memcmp(&got[k], &r, sizeof r) != 0 && bad++ == 0)
      std::printf("%s: task %d (qlen %d tlen %d h0 %d): got %d %d %d %d %d %d want %d %d %d %d %d %d\n", c.name, k, t.qlen,
                  t.tlen, t.h0, got[k].score, got[k].qle, got[k].tle, got[k].gtle, got[k].gscore, got[k].max_off, r.score,
                  r.qle, r.tle, r.gtle, r.gscore, r.max_off);
    if (t.tlen < t.qlen) ++short_cert;
  }
  std::printf("%s: %d of %d calls certified\n", c.name, nc, n);
  EXPECT(bad == 0);
  EXPECT(short_cert == 0);
  if (c.none) EXPECT(nc == 0);
  else EXPECT(nc >= 150 && nc <= n - 150);
}

int main() {
  const Case cases[] = {
      {"default", 1, 4, 6, 1, 6, 1, 100, 100, false, false},
      {"oe_min_2", 1, 4, 1, 1, 3, 2, 100, 100, false, false},
      {"oe_min_2_zdrop_3", 1, 4, 4, 2, 1, 1, 100, 3, false, false},
      {"zdrop_3", 1, 4, 2, 1, 2, 1, 100, 3, false, false},
      {"zdrop_below_oe_min", 1, 4, 6, 1, 6, 1, 100, 3, false, true},
      {"w_1", 1, 4, 6, 1, 6, 1, 1, 100, false, false},
      {"asym_gaps", 1, 4, 9, 2, 4, 1, 100, 100, false, false},
      {"matrix", 4, 6, 8, 2, 7, 3, 100, 100, true, false},
      {"a_2", 2, 3, 5, 2, 5, 2, 100, 0, false, false},
  };
  std::mt19937 rng(20261021);
  for (const Case& c : cases) run_case(c, rng);
  if (g_fail) return 1;
  std::printf("ungapped_asan OK\n");
  return 0;
}
