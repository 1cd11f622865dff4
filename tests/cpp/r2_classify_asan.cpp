// r2_classify_asan.cpp — r2_classify (bwa-flow_amd/csrc/pure.h), the per-job
// classifier of bwagpu_reg2aln_device, under the host sanitizers.  Stand-alone:
// no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/r2_classify_asan.cpp -o r2_classify_asan && ./r2_classify_asan
//
// Checked on 100,000 random jobs and on hostile ones (fields at the ends of
// their types), under three scorings:
//  * no sanitizer report (no signed overflow, no out-of-range float cast);
//  * the verdict equals an independent statement of the refusal rules in
//    128-bit arithmetic;
//  * for an accepted job lq <= 1023, rl <= 8192 and zb / bucket / cls equal a
//    transcription of bwagpu_reg2aln_batch's validation loop;
//  * the band of each of the three tries reg2aln_kernel can make, recomputed
//    in wide arithmetic from the reference's formulas, needs a direction
//    matrix of at most zb bytes: the inequality that keeps the kernel inside
//    the LDS (or HBM slice) its bin was sized for.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
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

typedef __int128 wide;
static const int32_t I32MIN = std::numeric_limits<int32_t>::min(), I32MAX = std::numeric_limits<int32_t>::max();
static const int64_t I64MIN = std::numeric_limits<int64_t>::min(), I64MAX = std::numeric_limits<int64_t>::max();

static DevOpt make_opt(int a, int b, int o_del, int e_del, int o_ins, int e_ins, int w) {
  DevOpt o{};
  o.a = a, o.o_del = o_del, o.e_del = e_del, o.o_ins = o_ins, o.e_ins = e_ins;
  o.oe_del = o_del + e_del, o.oe_ins = o_ins + e_ins, o.pen_clip5 = o.pen_clip3 = 5, o.w = w, o.zdrop = 100;
  o.max_mat = a, o.row_bound = 1;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (int8_t)((i == 4 || j == 4) ? -1 : (i == j ? a : -b));
  return o;
}

// the window test of bwagpu_reg2aln_batch (bwa.c:133-135), in wide arithmetic
static bool window_ok(int64_t l_pac, const bwagpu_reg2aln_task_t& t) {
  if (t.rb < 0 || t.re < 0) return false;
  const wide two = (wide)l_pac * 2, beg = t.rb, end = (wide)t.re > two ? two : (wide)t.re;
  return t.qe > t.qb && t.rb < t.re && !(t.rb < l_pac && t.re > l_pac) && (beg >= l_pac || end <= l_pac) &&
         end - beg == (wide)t.re - t.rb;
}

// the refusal rules as the header states them
static bool must_refuse(const DevOpt& o, int64_t l_pac, int64_t qpool_len, const bwagpu_reg2aln_task_t& t,
                        bool* lds_rule) {
  *lds_rule = false;
  if (t.l_seq < 0 || t.qoff < 0 || (wide)t.qoff + t.l_seq > (wide)qpool_len) return true;
  if ((wide)t.truesc < -(wide)(1 << 24) || (wide)t.truesc > (wide)(1 << 24)) return true;
  if (t.w < 0 || t.w > (1 << 24)) return true;
  if (!window_ok(l_pac, t)) return false;
  if (t.qb < 0 || t.qe > t.l_seq) return true;
  if ((wide)t.qe - t.qb > BWAGPU_MAX_READ_LEN) return true;
  if ((wide)t.re - t.rb > kR2MaxRef) return true;
  (void)o;
  *lds_rule = true;  // the LDS rule needs the class: checked with the transcription below
  return false;
}

// bwagpu_reg2aln_batch's loop body from `lq = t.qe - t.qb` on (capi_tasks.hip), for a job inside its limits
struct Batch {
  int lq, rl, cls;
  int64_t zb;
};
static Batch batch_body(const DevOpt& o, const bwagpu_reg2aln_task_t& t) {
  const int wmax = o.w << 2;
  const int lq = t.qe - t.qb, rl = (int)(t.re - t.rb);
  auto infer = [&](int q_, int r_) {
    if (lq == rl && lq * o.a - t.truesc < (q_ + r_ - o.a) * 2) return 0;
    const int w = (int)((double)(std::min(lq, rl) * o.a - t.truesc - q_) / r_ + 2.);
    return std::max(w, std::abs(lq - rl));
  };
  int w2 = std::max(infer(o.o_del, o.e_del), infer(o.o_ins, o.e_ins));
  if (w2 > o.w) w2 = std::min(w2, t.w);
  w2 = std::min(w2, wmax);
  const int w2max = (int)std::min<int64_t>((int64_t)w2 * 4, wmax);
  const int half = (lq + 1) >> 1;
  const int mi = (int)((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
  const int mdl = (int)((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
  const int mg = std::max(std::max(mi, mdl), 1), dl = std::abs(rl - lq);
  const int wb = std::max(std::min((mg + dl + 1) >> 1, w2max), dl + 3);
  Batch b;
  b.lq = lq, b.rl = rl;
  b.zb = (int64_t)std::min(lq, 2 * wb + 1) * rl;
  b.cls = b.zb <= kR2ZSmall ? 0 : (b.zb <= kR2ZLarge ? 1 : 2);
  return b;
}

// mem_reg2aln's band loop (bwamem.c:801-808, 1122-1134; bwa.c:152-165) in wide
// arithmetic, every try taken: the largest direction matrix any try writes
static wide infer_bw_wide(wide l1, wide l2, wide score, wide a, wide q, wide r) {
  if (l1 == l2 && l1 * a - score < (q + r - a) * 2) return 0;
  const long double x = (long double)(double)((l1 < l2 ? l1 : l2) * a - score - q) / (long double)(double)r + 2.L;
  const wide w = (wide)std::trunc((double)x);
  const wide d = l1 > l2 ? l1 - l2 : l2 - l1;
  return w < d ? d : w;
}
static wide widest_matrix(const DevOpt& o, const bwagpu_reg2aln_task_t& t) {
  const wide lq = (wide)t.qe - t.qb, rl = (wide)t.re - t.rb, wmax = (wide)o.w * 4;
  wide w2 = std::max(infer_bw_wide(lq, rl, t.truesc, o.a, o.o_del, o.e_del),
                     infer_bw_wide(lq, rl, t.truesc, o.a, o.o_ins, o.e_ins));
  if (w2 > o.w) w2 = std::min<wide>(w2, t.w);
  wide worst = 0;
  for (int tries = 0; tries < 3; ++tries) {
    w2 = std::min(w2, wmax);
    if (!(lq == rl && w2 == 0)) {
      const wide half = (lq + 1) / 2;
      const wide mi = (wide)std::trunc((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
      const wide md = (wide)std::trunc((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
      const wide mg = std::max<wide>(std::max(mi, md), 1), dl = lq > rl ? lq - rl : rl - lq;
      wide w = std::min((mg + dl + 1) / 2, w2);
      w = std::max(w, dl + 3);
      const wide ncol = lq < 2 * w + 1 ? lq : 2 * w + 1;
      worst = std::max(worst, ncol * rl);
    }
    if (w2 == wmax) break;
    w2 *= 2;
  }
  return worst;
}

static long g_accepted = 0, g_refused = 0, g_dp = 0, g_cls[3] = {};

static void check(const DevOpt& o, int64_t l_pac, int64_t qpool_len, const bwagpu_reg2aln_task_t& t) {
  const R2Class c = r2_classify(o, l_pac, qpool_len, t);
  bool lds_rule = false;
  const bool refuse = must_refuse(o, l_pac, qpool_len, t, &lds_rule);
  if (refuse) {
    EXPECT(c.verdict == R2_REFUSED);
    ++g_refused;
    return;
  }
  if (!lds_rule) {  // unmapped, or a window bwa_gen_cigar2 rejects: the kernel's verdicts, no DP
    EXPECT(c.verdict == R2_ACCEPTED && c.lq == 0 && c.rl == 0 && c.zb == 0 && c.cls == 0 && c.bucket == 0);
    ++g_accepted;
    return;
  }
  const Batch b = batch_body(o, t);
  int qc, rc, oc;
  const bool too_big = (b.cls == 1 ? 1 : 4) * r2_lds_per_wave(b.lq, b.rl, b.cls, &qc, &rc, &oc) > 160 * 1024;
  if (too_big) {
    EXPECT(c.verdict == R2_REFUSED);
    ++g_refused;
    return;
  }
  EXPECT(c.verdict == R2_ACCEPTED);
  EXPECT(c.lq >= 1 && c.lq <= 1023 && c.rl >= 1 && c.rl <= 8192);
  EXPECT(c.lq == b.lq && c.rl == b.rl && c.zb == b.zb && c.cls == b.cls && c.bucket == r2_bucket_of(b.lq));
  EXPECT(c.bucket >= 0 && c.bucket < kR2Buckets && c.lq + 1 <= 64 * kR2CD[c.bucket]);
  EXPECT(widest_matrix(o, t) <= (wide)c.zb);
  EXPECT(c.cls == 2 || c.zb <= (c.cls == 0 ? kR2ZSmall : kR2ZLarge));
  const int cc = r2_cost_class(c.cls, c.zb + c.lq + c.rl);
  EXPECT(cc >= 0 && cc < kR2CostClasses);
  ++g_accepted, ++g_dp, ++g_cls[c.cls];
}

int main() {
  const DevOpt opts[3] = {make_opt(1, 4, 6, 1, 6, 1, 100), make_opt(2, 5, 7, 2, 5, 3, 30),
                          make_opt(127, 127, 65535, 1, 0, 1, 1 << 20)};
  const int64_t l_pac = 5000000, qpool_len = 4000000;
  std::mt19937_64 rng(20);
  auto uni = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  for (const DevOpt& o : opts) {
    for (int it = 0; it < 100000; ++it) {
      bwagpu_reg2aln_task_t t{};
      const int kind = (int)(rng() % 8);
      t.l_seq = (int32_t)uni(1, kind == 0 ? 1100 : (kind < 4 ? 260 : 1023));
      t.qoff = uni(0, qpool_len - t.l_seq);
      t.qb = (int32_t)uni(0, t.l_seq / 4);
      t.qe = (int32_t)uni(t.l_seq - t.l_seq / 4, t.l_seq);
      const int lq = t.qe - t.qb;
      const bool rev = rng() & 1;
      t.rb = uni(0, l_pac - 10000) + (rev ? l_pac : 0);
      const int64_t slack = kind == 1 ? uni(-lq + 1, 9000) : uni(-std::min(lq - 1, 40), 40);
      t.re = t.rb + std::max<int64_t>(1, lq + slack);
      t.truesc = (int32_t)uni(kind == 2 ? -(1 << 24) - 2 : 0, kind == 2 ? (1 << 24) + 2 : (int64_t)lq * o.a);
      t.w = (int32_t)uni(kind == 3 ? -2 : 0, kind == 3 ? (1 << 24) + 2 : 4 * o.w);
      if (kind == 4) t.qoff = uni(-5, qpool_len + 5);
      if (kind == 5) t.rb = uni(l_pac - 300, l_pac + 300), t.re = t.rb + lq;
      if (kind == 6) t.qe = (int32_t)uni(t.qb - 2, t.l_seq + 2);
      check(o, l_pac, qpool_len, t);
    }
    // hostile: every field at the ends of its type, a few at a time, over a good job
    bwagpu_reg2aln_task_t g{};
    g.rb = 1000, g.re = 1150, g.qoff = 0, g.l_seq = 150, g.qb = 0, g.qe = 150, g.truesc = 140, g.w = 100;
    const int64_t v64[] = {I64MIN, I64MIN + 1, -1, 0, 1, l_pac - 1, l_pac, l_pac + 1, 2 * l_pac, I64MAX - 1, I64MAX};
    const int32_t v32[] = {I32MIN, I32MIN + 1, -(1 << 24) - 1, -(1 << 24), -1, 0, 1, 1023, 1024, (1 << 24), (1 << 24) + 1,
                           I32MAX - 1, I32MAX};
    for (int64_t a : v64)
      for (int64_t b : v64) {
        bwagpu_reg2aln_task_t t = g;
        t.rb = a, t.re = b;
        check(o, l_pac, qpool_len, t);
        t = g, t.qoff = a, t.rb = b;
        check(o, l_pac, qpool_len, t);
        t = g, t.re = a, t.qoff = b;
        check(o, l_pac, I64MAX, t);
      }
    for (int32_t a : v32)
      for (int32_t b : v32) {
        bwagpu_reg2aln_task_t t = g;
        t.qb = a, t.qe = b;
        check(o, l_pac, qpool_len, t);
        t.l_seq = I32MAX;
        check(o, l_pac, I64MAX, t);
        t = g, t.truesc = a, t.w = b;
        check(o, l_pac, qpool_len, t);
        t = g, t.l_seq = a, t.qe = b;
        check(o, l_pac, qpool_len, t);
        t = g, t.truesc = a, t.qb = b;
        check(o, l_pac, qpool_len, t);
        // the limits themselves, with the score and band fields at the ends
        t = g, t.l_seq = 1023, t.qe = 1023, t.re = t.rb + 8192, t.truesc = a, t.w = b;
        check(o, l_pac, qpool_len, t);
        t.re = t.rb + 8193;
        check(o, l_pac, qpool_len, t);
        t = g, t.l_seq = 1100, t.qe = 1024, t.truesc = a, t.w = b;
        check(o, l_pac, qpool_len, t);
      }
  }
  EXPECT(g_dp > 100000 && g_refused > 5000 && g_cls[0] > 1000 && g_cls[1] > 1000 && g_cls[2] > 1000);
  if (g_fail) {
    std::printf("r2_classify_asan: %d failure(s); %ld accepted (%ld with a DP: %ld / %ld / %ld per class), %ld refused\n",
                g_fail, g_accepted, g_dp, g_cls[0], g_cls[1], g_cls[2], g_refused);
    return 1;
  }
  std::printf("r2_classify_asan OK: %ld accepted (%ld with a DP: %ld / %ld / %ld per class), %ld refused\n", g_accepted,
              g_dp, g_cls[0], g_cls[1], g_cls[2], g_refused);
  return 0;
}
