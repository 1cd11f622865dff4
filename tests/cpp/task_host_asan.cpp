// task_host_asan.cpp — the host-side plans of bwagpu_extend_batch,
// bwagpu_align2_batch and bwagpu_sw_stream
// (bwa-flow_amd/csrc/task_host.h) under the host sanitizers.  Stand-alone: no
// GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/task_host_asan.cpp -o task_host_asan && ./task_host_asan
//
// The task, base and output arrays handed to a plan are heap allocations of
// exactly the size the ABI promises, so a read past the end is an
// AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "task_host.h"

using namespace bwagpu;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static const int64_t I64MAX = std::numeric_limits<int64_t>::max();
static const int32_t I32MAX = std::numeric_limits<int32_t>::max();

template <class T>
struct Exact {  // an exact-size heap copy: a vector's capacity may exceed its size
  T* p;
  explicit Exact(const std::vector<T>& v) : p((T*)std::malloc(v.size() ? v.size() * sizeof(T) : 1)) {
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  }
  ~Exact() { std::free(p); }
  Exact(const Exact&) = delete;
};

static DevOpt default_opt() {  // bwa mem's defaults: -A1 -B4 -O6 -E1 -L5 -w100 -d100
  DevOpt o{};
  o.a = 1, o.o_del = o.o_ins = 6, o.e_del = o.e_ins = 1, o.oe_del = o.oe_ins = 7;
  o.pen_clip5 = o.pen_clip3 = 5, o.w = 100, o.zdrop = 100, o.max_mat = 1, o.row_bound = 1;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (i == 4 || j == 4) ? -1 : (i == j ? 1 : -4);
  return o;
}

static bool is(const char* why, const char* text) { return why && !std::strcmp(why, text); }

static bool is_permutation_of_n(const std::vector<int32_t>& all, size_t n) {
  std::vector<char> seen(n, 0);
  if (all.size() != n) return false;
  for (int32_t k : all) {
    if (k < 0 || (size_t)k >= n || seen[(size_t)k]) return false;
    seen[(size_t)k] = 1;
  }
  return true;
}

// ---------------------------------------------------------------- extend
struct Ext {
  DevOpt o = default_opt();
  bool quad = false;
  std::vector<bwagpu_ext_task_t> t;
  std::vector<uint8_t> q, tp;
  ExtendPlan plan;
  const char* why = nullptr;
  int run() {
    Exact<bwagpu_ext_task_t> et(t);
    Exact<uint8_t> eq(q), ett(tp);
    Exact<bwagpu_ext_result_t> res(std::vector<bwagpu_ext_result_t>(t.size()));
    return extend_plan(o, quad, (int32_t)t.size(), et.p, eq.p, (int64_t)q.size(), ett.p, (int64_t)tp.size(), res.p,
                       &plan, &why);
  }
};
static bwagpu_ext_task_t ext(int64_t qoff, int32_t qlen, int64_t toff, int32_t tlen, int32_t h0 = 0, int32_t w = 100) {
  return bwagpu_ext_task_t{qoff, toff, qlen, tlen, w, 5, 100, h0};
}
static Ext ext_base() {
  Ext c;
  c.q.assign(2048, 1);
  c.tp.assign(4096, 2);
  c.t = {ext(0, 100, 0, 150), ext(100, 50, 150, 80), ext(0, 300, 0, 400)};
  return c;
}

static void test_extend() {
  ExtendPlan plan;
  const char* why = nullptr;
  const DevOpt o = default_opt();
  bwagpu_ext_result_t r1;
  bwagpu_ext_task_t t1 = ext(0, 0, 0, 0);
  uint8_t b1 = 0;
  {  // n == 0 reads nothing; the argument checks (align2_batch's, with the pools')
    EXPECT(extend_plan(o, true, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_OK);
    EXPECT(plan.all.empty() && is(why, ""));
    EXPECT(extend_plan(o, true, -1, nullptr, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 1, nullptr, nullptr, 0, nullptr, 0, &r1, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 1, &t1, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 0, nullptr, nullptr, -1, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 0, nullptr, nullptr, 0, nullptr, -1, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 1, &t1, nullptr, 1, &b1, 1, &r1, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(extend_plan(o, true, 1, &t1, &b1, 1, nullptr, 1, &r1, &plan, &why) == BWAGPU_E_INVAL && is(why, ""));
    EXPECT(extend_plan(o, true, 1, &t1, nullptr, 0, nullptr, 0, &r1, &plan, &why) == BWAGPU_OK);  // empty pools
    EXPECT(plan.all.size() == 1 && plan.count[0] == 1);
  }
  {  // every refusal text
    Ext c = ext_base();
    EXPECT(c.run() == BWAGPU_OK);
    for (int f = 0; f < 7; ++f) {
      c = ext_base();
      bwagpu_ext_task_t& t = c.t[1];
      if (f == 0) t.qlen = -1;
      if (f == 1) t.tlen = -1;
      if (f == 2) t.qoff = -1;
      if (f == 3) t.toff = -1;
      if (f == 4) t.qoff = 2048 - 49;
      if (f == 5) t.toff = 4096 - 79;
      if (f == 6) t.w = -1;
      EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    }
    c = ext_base();
    c.t[1] = ext(2048 - 50, 50, 4096 - 80, 80);  // up to the last base of both pools
    EXPECT(c.run() == BWAGPU_OK);
    c.t[1].qlen = 1024;
    c.t[1].qoff = 0;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen too long"));
    c = ext_base();
    c.q[2047] = 5;  // a base no task covers
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "query base > 4"));
    c.tp[4095] = 5;  // the query pool is looked at first
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "query base > 4"));
    c.q[2047] = 4;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "target base > 4"));
    c = ext_base();
    c.tp.assign(20000, 2);
    c.t[0] = ext(0, 100, 0, 20000, 0, 1 << 20);
    c.t[0].end_bonus = 1 << 20;  // neither the band nor the penalties bound the rows: 20000 of them
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "task needs too many LDS rows"));
  }
  {  // the earlier of two bad tasks wins; a bad task wins over a bad pool base
    Ext c = ext_base();
    c.t[1].qlen = 1024, c.t[1].qoff = 0;
    c.t[2].tlen = 5000;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen too long"));
    c.t[0].tlen = 5000;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = ext_base();
    c.q[0] = 9;
    c.t[2].qlen = 1024;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen too long"));
  }
  {  // sums that do not fit their type: the task is outside its pool
    Ext c = ext_base();
    c.t[1].qoff = I64MAX, c.t[1].qlen = 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = ext_base();
    c.t[1].toff = I64MAX, c.t[1].tlen = 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = ext_base();
    c.t[1].qlen = I32MAX;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c.t[1].qoff = 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
  }
  {  // both sides of every max_len() boundary (qlen + 1 columns): 192, 256, 1024
    Ext c = ext_base();
    c.t.clear();
    const int ql[] = {191, 192, 255, 256, 1023, 0}, want[] = {0, 1, 1, 2, 2, 0};
    for (int q : ql) c.t.push_back(ext(0, q, 0, 100, 7));
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(!c.plan.t5 && c.plan.count[0] == 2 && c.plan.count[1] == 2 && c.plan.count[2] == 2);
    for (int v = 0; v < kNumExtVariants; ++v)
      for (int i = 0; i < c.plan.count[v]; ++i) EXPECT(want[c.plan.all[(size_t)(c.plan.off[v] + i)]] == v);
    EXPECT((c.plan.all == std::vector<int32_t>{0, 5, 1, 2, 3, 4}));  // task order inside a list
    // rows = min(tlen, qlen + band + 1) = 100 -> (100 + 2 + 15) & ~15
    EXPECT(c.plan.tb[0] == 112 && c.plan.tb[1] == 112 && c.plan.tb[2] == 112 && c.plan.tb[3] == 0);
    // the packed kernel takes h0 > 0, 1 <= qlen <= 255, targets without an N
    c.quad = true;
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT((c.plan.all == std::vector<int32_t>{5, 3, 4, 0, 1, 2}) && c.plan.count[3] == 3 && c.plan.off[3] == 3);
    c.tp[99] = 4;  // an N in the last target row of every task
    EXPECT(c.run() == BWAGPU_OK && c.plan.t5 && c.plan.count[3] == 0);
    EXPECT((c.plan.all == std::vector<int32_t>{0, 5, 1, 2, 3, 4}));
    c.tp[99] = 2, c.tp[100] = 4;  // an N just past them
    EXPECT(c.run() == BWAGPU_OK && c.plan.t5 && c.plan.count[3] == 3);
    c.t[0].h0 = 0;
    EXPECT(c.run() == BWAGPU_OK && c.plan.count[3] == 2 && c.plan.all[0] == 0);
  }
}

static void test_extend_mixed() {  // the plan of a mixed batch
  Ext c = ext_base();
  c.quad = true;
  c.t.clear();
  std::mt19937 g(5);
  const int ql[] = {0, 1, 100, 150, 191, 192, 255, 256, 300, 1023};
  for (int i = 0; i < 200; ++i) {
    const int q = ql[g() % 10], tl = (int)(g() % 9) * 40;
    c.t.push_back(ext((int64_t)(g() % (2048 - q + 1)), q, (int64_t)(g() % (4096 - tl + 1)), tl, (int)(g() % 3) * 20));
  }
  for (int i = 0; i < 4096; i += 97) c.tp[(size_t)i] = 4;  // some targets hold an N
  EXPECT(c.run() == BWAGPU_OK);
  const ExtendPlan& p = c.plan;
  EXPECT(is_permutation_of_n(p.all, c.t.size()) && p.t5);
  int32_t off = 0;
  for (int v = 0; v < kExtLists; ++v) {
    EXPECT(p.off[v] == off && (p.count[v] == 0) == (p.tb[v] == 0) && p.tb[v] % 16 == 0);
    for (int32_t i = 0; i < p.count[v]; ++i) {
      const int32_t k = p.all[(size_t)(off + i)];
      const bwagpu_ext_task_t& t = c.t[(size_t)k];
      if (i) EXPECT(p.all[(size_t)(off + i - 1)] < k);  // task order inside a list
      if (v < kNumExtVariants) {
        EXPECT(t.qlen + 1 <= kExtVariants[v].max_len() && (v == 0 || t.qlen + 1 > kExtVariants[v - 1].max_len()));
      } else {
        EXPECT(t.h0 > 0 && t.qlen >= 1 && t.qlen <= 255);
        for (int32_t j = 0; j < t.tlen; ++j) EXPECT(c.tp[(size_t)(t.toff + j)] <= 3);
      }
      EXPECT(std::min(t.tlen, t.qlen + 1) + 2 <= p.tb[v]);  // its rows fit: at least the band-free ones
    }
    off += p.count[v];
  }
  EXPECT((size_t)off == c.t.size() && p.count[3] > 0 && p.count[0] > 0 && p.count[2] > 0);
}

// ---------------------------------------------------------------- the range gates
// Both sides of every boundary of the packed kernel's gates on the bare path
// (task_host.h extend_plan: quad_bound_ok(h0 + qlen * max_mat) and
// quad_rows_ok(tlen), pure.h): the last admitted value lands in list
// kNumExtVariants (extend4_kernel), the first refused one in a wave list.  The
// numbers are those of tests/range_cases.py, whose GPU test relies on this
// routing to know which kernel it ran.
static DevOpt scored_opt(int a, int b) {
  DevOpt o = default_opt();
  o.a = a, o.max_mat = a;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) o.mat[i * 5 + j] = (int8_t)(i == j ? a : -b);
  return o;
}
static void set_gaps(DevOpt& o, int o_del, int e_del, int o_ins, int e_ins) {
  o.o_del = o_del, o.e_del = e_del, o.o_ins = o_ins, o.e_ins = e_ins;
  o.oe_del = o_del + e_del, o.oe_ins = o_ins + e_ins;
}
// one task -> the list it lands in (0 .. kNumExtVariants), or -rc
static int list_of(const DevOpt& o, int qlen, int tlen, int h0, const char** why = nullptr) {
  Ext c;
  c.o = o;
  c.quad = true;
  c.q.assign(1024, 1);
  c.tp.assign(16384, 2);
  c.t = {ext(0, qlen, 0, tlen, h0)};
  const int rc = c.run();
  if (why) *why = c.why;
  if (rc != BWAGPU_OK) return -rc;
  for (int v = 0; v < kExtLists; ++v)
    if (c.plan.count[v]) return v;
  return -100;
}
static int wave_list(int qlen) { return qlen + 1 <= 192 ? 0 : (qlen + 1 <= 256 ? 1 : 2); }
#define EXPECT_FLIP(o_in, o_out, qlen, tl_in, tl_out, h0_in, h0_out)        \
  do {                                                                      \
    EXPECT(list_of(o_in, qlen, tl_in, h0_in) == kNumExtVariants);           \
    EXPECT(list_of(o_out, qlen, tl_out, h0_out) == wave_list(qlen));        \
  } while (0)

static void test_extend_ranges() {
  const DevOpt d = default_opt();
  // hb < 4096 (binding for max_mat 1 and 3)
  EXPECT_FLIP(d, d, 255, 255, 255, 4095 - 255, 4096 - 255);
  EXPECT_FLIP(d, d, 1, 1, 1, 4094, 4095);
  const DevOpt a3 = scored_opt(3, 4);
  EXPECT_FLIP(a3, a3, 255, 255, 255, 4095 - 765, 4096 - 765);
  // (hb << sk) + 128 < 32768: sk = 3 for max_mat 4..7 -> hb <= 4079; sk = 4 for 8..15 -> hb <= 2039
  const DevOpt a4 = scored_opt(4, 4), a7 = scored_opt(7, 4), a8 = scored_opt(8, 4), a15 = scored_opt(15, 4);
  EXPECT_FLIP(a4, a4, 255, 255, 255, 4079 - 1020, 4080 - 1020);
  EXPECT_FLIP(a7, a7, 255, 255, 255, 2294, 2295);
  EXPECT_FLIP(a8, a8, 254, 254, 254, 2039 - 2032, 2040 - 2032);
  EXPECT_FLIP(a15, a15, 135, 135, 135, 2039 - 2025, 2040 - 2025);
  DevOpt diag = scored_opt(2, 4);  // one large diagonal cell decides max_mat
  diag.mat[0] = 15, diag.max_mat = 15;
  EXPECT_FLIP(diag, diag, 135, 135, 135, 14, 15);
  DevOpt m127 = scored_opt(4, 127), m128 = scored_opt(4, 127);  // matrix entries in [-127, 127]
  m128.mat[1] = (int8_t)-128;
  EXPECT_FLIP(m127, m128, 255, 255, 255, 3059, 3059);
  DevOpt m16 = scored_opt(15, 4), m0 = scored_opt(1, 4);  // max_mat 1..15
  m16.mat[6] = 16, m16.max_mat = 16;
  EXPECT_FLIP(a15, m16, 100, 100, 100, 1, 1);
  for (int i = 0; i < 25; ++i) m0.mat[i] = (int8_t)std::min<int>(m0.mat[i], 0);
  m0.max_mat = 0;
  EXPECT_FLIP(d, m0, 100, 100, 100, 50, 50);
  // o_del + 128 < 32768, oe_ins + 128 < 32768
  DevOpt g_in = d, g_out = d;
  set_gaps(g_in, 32639, 1, 6, 1), set_gaps(g_out, 32640, 1, 6, 1);
  EXPECT_FLIP(g_in, g_out, 255, 255, 255, 3840, 3840);
  set_gaps(g_in, 6, 1, 32638, 1), set_gaps(g_out, 6, 1, 32639, 1);
  EXPECT_FLIP(g_in, g_out, 255, 255, 255, 3840, 3840);
  set_gaps(g_in, 32638, 1, 32638, 1), set_gaps(g_out, 32639, 1, 32639, 1);  // o_del == o_ins
  EXPECT_FLIP(g_in, g_out, 255, 255, 255, 3840, 3840);
  // hb + 264 e_ins < 32768 at e_ins = 111 (two target rows at the most: the rows gate)
  DevOpt sc = d;
  set_gaps(sc, 6, 1, 1, 111);
  EXPECT_FLIP(sc, sc, 255, 2, 2, 3463 - 255, 3464 - 255);
  EXPECT_FLIP(sc, sc, 1, 2, 3, 3462, 3462);  // 258 * 111 = 28638, 259 * 111 = 28749
  // (tlen + 256) * max(e_del, e_ins) < 28672
  const int te[3][2] = {{1, 111}, {256, 55}, {768, 27}};
  for (auto& x : te) {
    DevOpt r_in = d, r_out = d;
    set_gaps(r_in, 6, x[1], 6, x[1]), set_gaps(r_out, 6, x[1] + 1, 6, x[1] + 1);
    EXPECT_FLIP(r_in, r_out, 255, x[0], x[0], 3000 - 255, 3000 - 255);
    set_gaps(r_out, 6, x[1] + 1, 6, 1);  // either extension penalty alone
    EXPECT(list_of(r_out, 255, x[0], 2745) == 1);
    set_gaps(r_out, 6, 1, 6, x[1] + 1);
    EXPECT(list_of(r_out, 255, x[0], 2745) == 1);
  }
  EXPECT_FLIP(d, d, 255, 16383, 16384, 3840, 3840);  // rows < 16384
  // the 32-bit kernels' own ceiling (wave_bound_ok): hb < 2^21, whichever list
  const char* why = nullptr;
  const int ql[] = {100, 255, 700, 1022};
  for (int q : ql) {
    EXPECT(list_of(d, q, q, (1 << 21) - 1 - q) == wave_list(q));
    EXPECT(list_of(d, q, q, (1 << 21) - q, &why) == -BWAGPU_E_UNSUPPORTED);
    EXPECT(is(why, "h0 + qlen * max score >= 2^21: over the 32-bit kernels' row-max key"));
  }
  EXPECT(list_of(a15, 1022, 100, (1 << 21) - 1 - 15 * 1022) == 2);
  EXPECT(list_of(a15, 1022, 100, (1 << 21) - 15 * 1022) == -BWAGPU_E_UNSUPPORTED);
  EXPECT(list_of(d, 0, 0, (1 << 21) - 1) == 0 && list_of(d, 0, 0, 1 << 21) == -BWAGPU_E_UNSUPPORTED);
  EXPECT(list_of(d, 1000, 10, I32MAX) == -BWAGPU_E_UNSUPPORTED);  // the sum is taken in 64 bits
  {  // in task order with the other refusals; wave-only plans (quad off) refuse it too
    Ext c = ext_base();
    c.t[1].h0 = 1 << 21;
    c.t[2].qlen = 1024;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && std::strstr(c.why, "2^21"));
    c.t[0].qlen = 1024;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen too long"));
  }
}

// ---------------------------------------------------------------- align2
struct A2 {
  DevOpt o = default_opt();
  std::vector<bwagpu_align2_task_t> t;
  std::vector<uint8_t> q, tp;
  Align2Plan plan;
  const char* why = nullptr;
  int run() {
    Exact<bwagpu_align2_task_t> et(t);
    Exact<uint8_t> eq(q), ett(tp);
    Exact<bwagpu_kswr_t> res(std::vector<bwagpu_kswr_t>(t.size()));
    return align2_plan(o, (int32_t)t.size(), et.p, eq.p, (int64_t)q.size(), ett.p, (int64_t)tp.size(), res.p, &plan,
                       &why);
  }
};
static bwagpu_align2_task_t a2(int64_t qoff, int32_t qlen, int64_t toff, int32_t tlen, int32_t xtra) {
  return bwagpu_align2_task_t{qoff, toff, qlen, tlen, xtra, 0};
}
static A2 a2_base() {
  A2 c;
  c.q.assign(2048, 1);
  c.tp.assign(4096, 2);
  c.t = {a2(0, 100, 0, 150, BWAGPU_KSW_XBYTE), a2(100, 50, 150, 80, 0), a2(0, 300, 0, 400, BWAGPU_KSW_XBYTE)};
  return c;
}

static void test_align2() {
  Align2Plan plan;
  const char* why = nullptr;
  DevOpt o = default_opt();
  bwagpu_kswr_t r1;
  bwagpu_align2_task_t t1 = a2(0, 0, 0, 0, 0);
  uint8_t b1 = 0;
  {
    EXPECT(align2_plan(o, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_OK && plan.bins.empty());
    EXPECT(align2_plan(o, -1, nullptr, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 1, nullptr, nullptr, 0, nullptr, 0, &r1, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 1, &t1, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 0, nullptr, nullptr, -1, nullptr, 0, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 0, nullptr, nullptr, 0, nullptr, -1, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 1, &t1, nullptr, 1, &b1, 1, &r1, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(align2_plan(o, 1, &t1, &b1, 1, nullptr, 1, &r1, &plan, &why) == BWAGPU_E_INVAL && is(why, ""));
    DevOpt bad = o;  // an empty batch is accepted before the options are looked at
    bad.o_ins = 0;
    EXPECT(align2_plan(bad, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, &plan, &why) == BWAGPU_OK);
  }
  {  // every refusal text
    A2 c = a2_base();
    EXPECT(c.run() == BWAGPU_OK);
    c.o.o_ins = 0;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && std::strstr(c.why, "ksw_align2 with o_ins == 0") == c.why);
    c = a2_base();
    c.o.max_mat = 0;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && std::strstr(c.why, "ksw_align2 needs a positive match score") == c.why);
    c = a2_base();
    c.o.e_del = 65536;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "gap penalty > 65535"));
    for (int f = 0; f < 6; ++f) {
      c = a2_base();
      bwagpu_align2_task_t& t = c.t[1];
      if (f == 0) t.qlen = -1;
      if (f == 1) t.tlen = -1;
      if (f == 2) t.qoff = -1;
      if (f == 3) t.toff = -1;
      if (f == 4) t.qoff = 2048 - 49;
      if (f == 5) t.toff = 4096 - 79;
      EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    }
    c = a2_base();
    c.t[1] = a2(2048 - 50, 50, 4096 - 80, 80, 0);
    EXPECT(c.run() == BWAGPU_OK);
    c.t[1] = a2(0, BWAGPU_MAX_READ_LEN, 0, 80, 0);
    EXPECT(c.run() == BWAGPU_OK);
    c.t[1].qlen = BWAGPU_MAX_READ_LEN + 1;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen > BWAGPU_MAX_READ_LEN"));
    c = a2_base();
    c.o.max_mat = 100;
    c.t[1].qlen = 327;  // 32700
    EXPECT(c.run() == BWAGPU_OK);
    c.t[1].qlen = 328;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "i16 scores could saturate (qlen * max score > 32767)"));
    c.t[1].xtra = BWAGPU_KSW_XBYTE;  // the 8-bit kernels saturate like the reference's
    EXPECT(c.run() == BWAGPU_OK);
    c = a2_base();
    c.tp[4095] = 5;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "target base > 4"));
    c.q[2047] = 5;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "query base > 4"));
  }
  {  // order of verdicts
    A2 c = a2_base();
    c.t[1].qlen = BWAGPU_MAX_READ_LEN + 1;
    c.t[2].tlen = 5000;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen > BWAGPU_MAX_READ_LEN"));
    c.t[0].tlen = 5000;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = a2_base();
    c.q[0] = 9;
    c.t[2].qlen = BWAGPU_MAX_READ_LEN + 1;
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen > BWAGPU_MAX_READ_LEN"));
  }
  {  // overflow
    A2 c = a2_base();
    c.t[1].qoff = I64MAX, c.t[1].qlen = 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = a2_base();
    c.t[1].tlen = I32MAX, c.t[1].toff = 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    c = a2_base();
    c.t[1].qlen = I32MAX;
    EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
  }
  {  // the plan of a mixed batch
    A2 c = a2_base();
    c.t.clear();
    std::mt19937 g(7);
    const int ql[] = {0, 1, 64, 65, 128, 129, 150, 250, 256, 257, 384, 385, 512, 513, 768, 769, 1023};
    for (int i = 0; i < 200; ++i) {
      const int q = ql[g() % 17], tl = (int)(g() % 8) * 50;
      c.t.push_back(a2((int64_t)(g() % (2048 - q + 1)), q, (int64_t)(g() % (4096 - tl + 1)), tl,
                       g() % 2 ? BWAGPU_KSW_XBYTE : 0));
    }
    EXPECT(c.run() == BWAGPU_OK);
    const Align2Plan& p = c.plan;
    const size_t n = c.t.size();
    EXPECT(is_permutation_of_n(p.all, n) && p.boff.size() == n);
    int64_t scr = 0;
    for (size_t k = 0; k < n; ++k) {
      EXPECT(p.boff[k] == scr);
      scr += c.t[k].tlen + 1;
    }
    EXPECT(p.scratch == scr);
    int32_t off = 0;
    std::vector<int64_t> work(kA2Bins, 0);
    for (int b = 0; b < kA2Bins; ++b) {
      EXPECT(p.list_off[b] == off && p.counts[kA2Bins + b] == 0);
      for (int32_t i = 0; i < p.counts[b]; ++i) {
        const int32_t k = p.all[(size_t)(off + i)];
        EXPECT(a2_bin_of(c.t[(size_t)k].qlen, (c.t[(size_t)k].xtra & BWAGPU_KSW_XBYTE) != 0) == b);
        if (i) {  // longest target first, task order among equals
          const int32_t prev = p.all[(size_t)(off + i - 1)];
          EXPECT(c.t[(size_t)prev].tlen > c.t[(size_t)k].tlen || (c.t[(size_t)prev].tlen == c.t[(size_t)k].tlen && prev < k));
        }
        work[(size_t)b] += (int64_t)c.t[(size_t)k].tlen * kA2CD[b % kA2Buckets];
      }
      off += p.counts[b];
    }
    EXPECT((size_t)off == n);
    size_t nonempty = 0;
    for (int b = 0; b < kA2Bins; ++b) nonempty += p.counts[b] != 0;
    EXPECT(p.bins.size() == nonempty);
    for (size_t i = 0; i < p.bins.size(); ++i) {
      EXPECT(p.counts[p.bins[i]] > 0);
      if (i) EXPECT(work[(size_t)p.bins[i - 1]] >= work[(size_t)p.bins[i]]);
    }
  }
  {  // the reference's SIMD lane widths (pure.h): each quantity's last admitted value plans, the
     // next is refused with its reason.  Byte quantities: a batch with a byte task (a2_base's first).
    const char* const kByte =
        "ksw_align2 XBYTE task with e_del, e_ins, o_del + e_del or o_ins + e_ins > 255: the reference's 8-bit pass "
        "keeps 8 bits of them (_mm_set1_epi8, ksw.c:132-135)";
    const char* const kWord =
        "ksw_align2 with o_del + e_del or o_ins + e_ins > 65535: the reference keeps 16 bits of them "
        "(_mm_set1_epi16, ksw.c:252-255)";
    auto with = [](int o_del, int e_del, int o_ins, int e_ins) {
      A2 c = a2_base();
      c.o.o_del = o_del, c.o.e_del = e_del, c.o.o_ins = o_ins, c.o.e_ins = e_ins;
      c.o.oe_del = o_del + e_del, c.o.oe_ins = o_ins + e_ins;
      return c;
    };
    struct Edge { int o_del, e_del, o_ins, e_ins; };
    const Edge byte_in[] = {{254, 1, 6, 1}, {6, 1, 254, 1}, {0, 255, 6, 1}, {6, 1, 1, 254}, {1, 254, 6, 1}, {254, 1, 254, 1}};
    const Edge byte_out[] = {{255, 1, 6, 1}, {6, 1, 255, 1}, {0, 256, 6, 1}, {6, 1, 1, 255}, {1, 255, 6, 1}, {300, 1, 6, 1}};
    for (const Edge& e : byte_in) {
      A2 c = with(e.o_del, e.e_del, e.o_ins, e.e_ins);
      EXPECT(align2_byte_ok(c.o) && c.run() == BWAGPU_OK);
    }
    for (const Edge& e : byte_out) {
      A2 c = with(e.o_del, e.e_del, e.o_ins, e.e_ins);
      EXPECT(!align2_byte_ok(c.o) && c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, kByte));
      // the same options with no byte task in the batch: word tasks stay admitted
      for (auto& t : c.t) t.xtra &= ~BWAGPU_KSW_XBYTE;
      EXPECT(c.run() == BWAGPU_OK && c.plan.all.size() == c.t.size());
    }
    {  // e_del alone: 255 is the last value a lane holds; it needs o_del = 0 to keep o_del + e_del there
      DevOpt o = default_opt();
      o.o_del = 0, o.e_del = 255, o.oe_del = 255;
      EXPECT(align2_byte_ok(o));
      o.e_del = 256;
      o.oe_del = 255;  // (not reachable from bwagpu_opt_t: the clause on e_del itself)
      EXPECT(!align2_byte_ok(o));
      o = default_opt();
      o.o_ins = 1, o.e_ins = 254, o.oe_ins = 255;
      EXPECT(align2_byte_ok(o));
      o.e_ins = 256, o.oe_ins = 255;
      EXPECT(!align2_byte_ok(o));
    }
    {  // a mixed batch is refused at its first byte task: the verdict of an earlier word task wins
      A2 c = with(300, 1, 6, 1);
      c.t = {a2(0, 100, 0, 150, 0), a2(100, 50, 150, 80, BWAGPU_KSW_XBYTE), a2(0, BWAGPU_MAX_READ_LEN + 1, 0, 80, 0)};
      EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, kByte));
      c.t[0].qlen = BWAGPU_MAX_READ_LEN + 1;
      EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, "qlen > BWAGPU_MAX_READ_LEN"));
      c.t[0] = a2(0, 100, 0, 150, 0);
      c.t[1].toff = 4096;  // a byte task outside its pools is a bad argument first
      EXPECT(c.run() == BWAGPU_E_INVAL && is(c.why, "task outside its pools"));
    }
    // the word sums: 65535 plans (word tasks; a byte task is over the byte limit there), 65536 is refused for all
    const Edge word_in[] = {{65534, 1, 6, 1}, {6, 1, 65534, 1}, {1, 65534, 6, 1}, {6, 1, 1, 65534}};
    const Edge word_out[] = {{65535, 1, 6, 1}, {6, 1, 65535, 1}, {1, 65535, 6, 1}, {6, 1, 1, 65535}};
    for (const Edge& e : word_in) {
      A2 c = with(e.o_del, e.e_del, e.o_ins, e.e_ins);
      EXPECT(align2_opt_unsupported(c.o) == nullptr);
      EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, kByte));
      for (auto& t : c.t) t.xtra &= ~BWAGPU_KSW_XBYTE;
      EXPECT(c.run() == BWAGPU_OK);
    }
    for (const Edge& e : word_out) {
      A2 c = with(e.o_del, e.e_del, e.o_ins, e.e_ins);
      for (auto& t : c.t) t.xtra &= ~BWAGPU_KSW_XBYTE;
      EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && is(c.why, kWord) && is(align2_opt_unsupported(c.o), kWord));
    }
    // the 16-bit ceiling at a = 127: 258 columns (32766) plan, 259 (32893) do not
    A2 c = a2_base();
    c.o.max_mat = 127;
    c.t[1].qlen = 258;
    EXPECT(align2_word_fits(258, 127) && c.run() == BWAGPU_OK);
    c.t[1].qlen = 259;
    EXPECT(!align2_word_fits(259, 127) && c.run() == BWAGPU_E_UNSUPPORTED &&
           is(c.why, "i16 scores could saturate (qlen * max score > 32767)"));
    EXPECT(align2_word_fits(32767, 1) && !align2_word_fits(32768, 1));
  }
}

// ---------------------------------------------------------------- stream
static int run_stream(const std::vector<int32_t>& w, StreamPlan* plan, const char** why) {
  Exact<int32_t> e(w);
  return stream_plan(e.p, (int64_t)w.size(), plan, why);
}

static void test_stream() {
  StreamPlan plan;
  const char* why = nullptr;
  EXPECT(stream_plan(nullptr, 0, &plan, &why) == BWAGPU_OK && plan.starts.empty() && plan.lq_max == 1);
  EXPECT(stream_plan(nullptr, -1, &plan, &why) == BWAGPU_E_INVAL);
  EXPECT(stream_plan(nullptr, 3, &plan, &why) == BWAGPU_E_INVAL && is(why, ""));
  // three records: words [0, 5), [5, 8), [8, 14); word 1 of each is its read length
  const std::vector<int32_t> good = {5, 150, -7, -7, -7, 8, 0, -7, 14, 250, -7, -7, -7, -7};
  EXPECT(run_stream(good, &plan, &why) == BWAGPU_OK);
  EXPECT((plan.starts == std::vector<int64_t>{0, 5, 8}) && plan.lq_max == 250);
  std::vector<int32_t> w = good;
  w[8] = 15;  // past the end
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: a record's end word is out of range"));
  w[8] = 10;  // a record of two words
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: a record's end word is out of range"));
  w[8] = -1;
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: a record's end word is out of range"));
  w = good;
  w.push_back(20);  // a last record of one word: its length word is never read
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: a record's end word is out of range"));
  w = good;
  w[6] = -1;
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: negative read length"));
  w[6] = BWAGPU_MAX_READ_LEN;
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_OK && plan.lq_max == BWAGPU_MAX_READ_LEN);
  w[6] = BWAGPU_MAX_READ_LEN + 1;
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_UNSUPPORTED && is(why, "stream: read longer than BWAGPU_MAX_READ_LEN"));
  w[1] = -1;  // the earlier record wins
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: negative read length"));
  w[0] = 2;
  EXPECT(run_stream(w, &plan, &why) == BWAGPU_E_INVAL && is(why, "stream: a record's end word is out of range"));
}

int main() {
  test_extend();
  test_extend_mixed();
  test_extend_ranges();
  test_align2();
  test_stream();
  if (g_fail) {
    std::printf("task_host_asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("task_host_asan OK\n");
  return 0;
}
