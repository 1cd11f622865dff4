// ext_plan_asan.cpp — ext_plan (bwa-flow_amd/csrc/spec_plan.h), the one place
// that names the extension kernel of each length bin, against the decision it
// replaced, under the host sanitizers.  Stand-alone: no GPU, no HIP, not
// loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I include -I bwa-flow_amd/csrc tests/cpp/ext_plan_asan.cpp -o ext_plan_asan && ./ext_plan_asan
//
// The reference below is the launch code as it stood before the plan (commit
// c325099: ext_kernel_for, the branches of launch_ext_round and
// launch_side_pair, side_short_plan), with its two environment knobs at their
// defaults (the phased mask 1, the producer waves off) and every launch
// replaced by a record of what it would have launched (old_*: the names that
// spec_plan.h now has).  Some literal rows of the table follow, so that the
// copy and the plan cannot be wrong together.
#include <cstdio>
#include <cstring>
#include <vector>

#include "spec_plan.h"

using namespace bwagpu;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

// ---------------------------------------------------------------- the reference
namespace ref {
constexpr int kBinLen[2] = {160, 256};
constexpr int kSide = 96, kSG = 8, kSP = 8, kSQMax = 63, kBlk = 256;

static size_t old_side4_wave_lds(int tb_bytes, int g, int pmax) {
  return (size_t)(64 / g) * (2 * (size_t)tb_bytes + 2 * kSide + 2 * (size_t)pmax * g);
}
static int old_side_short_plan(const DevOpt& o, int tb_bytes, int g, int pmax, int short_q, int* tb_short, size_t* wave_lds) {
  const size_t w1 = old_side4_wave_lds(tb_bytes, g, pmax);
  *tb_short = 0;
  *wave_lds = w1;
  short_q = std::min(std::max(short_q, 0), kSQMax);
  if (short_q == 0) return 0;
  const int tbs = tb_bytes_for(o, short_q);
  const size_t w2 = (old_side4_wave_lds(tbs, kSG, kSP) + 15) & ~(size_t)15;
  if ((size_t)(kBlk / 64) * std::max(w1, w2) > 64 * 1024) return 0;
  *tb_short = tbs;
  *wave_lds = std::max(w1, w2);
  return short_q;
}
constexpr int kMask = 1;  // ext_phased_mask() with the variable unset
static int ext_kernel_for(const DevOpt& o, int form, int tb_bytes) {
  const bool quad = form != 1 && quad_scores_ok(o, kBinLen[1]) && quad_rows_ok(o, tb_bytes);
  const bool key8 = quad && quad_key8_ok(o, kBinLen[0]);
  const int k = key8 ? (form == 0 ? 8 : 4) : (quad ? 5 : 2);
  if (!quad || !(kMask & 1)) return k;
  return 10 + k;  // ext_producer() is false
}

struct Launch {  // one bin's kernel; for a side pair also launch_side_pair's arguments
  int family = -1, G = 0, PMAX = 0;
  bool K8 = false;
  size_t wave_lds = 0;
  int short_q = 0, tb_short = 0;
};
struct Round {
  bool quad = false, p0 = false, p1 = false;
  int sort_short_q = 0;
  Launch bin[2];
};
static Launch side_pair(const DevOpt& o, int tb_bytes, int G, int PMAX, bool K8, int short_q) {
  Launch l;
  l.family = SIDE4, l.G = G, l.PMAX = PMAX, l.K8 = K8;
  l.short_q = old_side_short_plan(o, tb_bytes, G, PMAX, G == 16 && K8 ? short_q : 0, &l.tb_short, &l.wave_lds);
  return l;
}
static Launch task(int family, int G, int PMAX, bool K8) {
  Launch l;
  l.family = family, l.G = G, l.PMAX = PMAX, l.K8 = K8;
  return l;
}
static Round launch_ext_round(const DevOpt& o, int form, int tb_bytes, int ss_short_q) {
  Round r;
  const bool quad = form != 1 && quad_scores_ok(o, kBinLen[1]) && quad_rows_ok(o, tb_bytes);
  const bool key8 = quad && quad_key8_ok(o, kBinLen[0]), oct = key8 && form == 0;
  const int pm = quad ? kMask : 0;
  const bool p0 = pm & 1, p1 = (pm >> 1) & 1;
  int short_q = 0;
  if (p0 && oct) {
    int tbs;
    size_t wl;
    short_q = old_side_short_plan(o, tb_bytes, 16, kBinLen[0] / 16, ss_short_q, &tbs, &wl);
  }
  r.quad = quad, r.p0 = p0, r.p1 = p1, r.sort_short_q = short_q;
  if (p0) {
    if (oct) r.bin[0] = side_pair(o, tb_bytes, 16, kBinLen[0] / 16, true, short_q);
    else if (key8) r.bin[0] = side_pair(o, tb_bytes, 32, kBinLen[0] / 32, true, 0);
    else r.bin[0] = side_pair(o, tb_bytes, 32, kBinLen[1] / 32, false, 0);
  } else if (oct) {
    r.bin[0] = task(EXT4, 16, kBinLen[0] / 16, true);
  } else if (key8) {
    r.bin[0] = task(EXT4, 32, kBinLen[0] / 32, true);
  } else if (quad) {
    r.bin[0] = task(EXT4, 32, kBinLen[1] / 32, false);
  } else {
    r.bin[0] = task(EXT2, 32, kBinLen[0] / 32, false);
  }
  if (p1) {
    if (form == 0) r.bin[1] = side_pair(o, tb_bytes, 16, kBinLen[1] / 16, false, 0);
    else r.bin[1] = side_pair(o, tb_bytes, 32, kBinLen[1] / 32, false, 0);
  } else if (quad && form == 0) {
    r.bin[1] = task(EXT4, 16, kBinLen[1] / 16, false);
  } else if (quad) {
    r.bin[1] = task(EXT4, 32, kBinLen[1] / 32, false);
  } else {
    r.bin[1] = task(EXT2, 32, kBinLen[1] / 32, false);
  }
  return r;
}
}  // namespace ref

// ---------------------------------------------------------------- option sets
static DevOpt default_opt() {  // bwa mem's defaults: -A1 -B4 -O6 -E1 -L5 -w100 -d100
  DevOpt o{};
  o.a = 1, o.o_del = o.o_ins = 6, o.e_del = o.e_ins = 1, o.oe_del = o.oe_ins = 7;
  o.pen_clip5 = o.pen_clip3 = 5, o.w = 100, o.zdrop = 100, o.max_mat = 1, o.row_bound = 1;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) o.mat[i * 5 + j] = (i == 4 || j == 4) ? -1 : (i == j ? 1 : -4);
  return o;
}
struct OptSet {
  const char* name;
  DevOpt o;
};
static std::vector<OptSet> option_sets() {
  std::vector<OptSet> v;
  v.push_back({"default", default_opt()});  // quad, key8
  DevOpt m2 = default_opt();                // quad, not key8: 160 * 2 > 255
  m2.a = m2.max_mat = 2;
  for (int i = 0; i < 4; ++i) m2.mat[i * 5 + i] = 2;
  v.push_back({"max_mat 2", m2});
  DevOpt m16 = default_opt();  // not quad: max_mat over 15, an entry outside [-127, 127]
  m16.a = m16.max_mat = 16;
  for (int i = 0; i < 4; ++i) m16.mat[i * 5 + i] = 16;
  m16.mat[1] = (int8_t)128;
  v.push_back({"max_mat 16", m16});
  DevOpt ge = default_opt();  // quad_scores_ok holds, quad_rows_ok fails from 31 row bytes on
  ge.e_del = ge.e_ins = 100, ge.oe_del = ge.oe_ins = 106;
  v.push_back({"gap extension 100", ge});
  DevOpt wide = default_opt();  // rows of several KB: the eight-per-wave pair's own buffers pass 64 KB per
  wide.w = 4000;                // block, so no short run (the end bonus lets the band cap reach 2 w)
  wide.pen_clip5 = wide.pen_clip3 = 5000;
  v.push_back({"band 4000", wide});
  return v;
}

static bool known_tuple(const ExtBin& k) {  // the kernels spec.hip's launch_ext_bin compiles
  static const ExtBin all[] = {{SIDE4, 16, 10, true, 0, true}, {SIDE4, 32, 5, true, 0, true}, {SIDE4, 32, 8, false, 0, true},
                               {EXT4, 16, 16, false, 0, false}, {EXT4, 32, 8, false, 0, false},
                               {EXT2, 32, 5, false, 0, false},  {EXT2, 32, 8, false, 0, false}};
  for (const ExtBin& a : all)
    if (a.family == k.family && a.G == k.G && a.PMAX == k.PMAX && a.K8 == k.K8 && a.phased == k.phased) return true;
  return false;
}

static bool bin_is(const ExtBin& k, int family, int g, int pmax, bool k8, int code, bool phased) {
  return k.family == family && k.G == g && k.PMAX == pmax && k.K8 == k8 && k.code == code && k.phased == phased;
}

int main() {
  static const int kLq[] = {1, 63, 64, 100, 160, 161, 256};
  static const int kShort[] = {-1, 0, 1, 63, 64, 1000};
  const std::vector<OptSet> sets = option_sets();
  int n = 0;
  bool saw_quad[2] = {false, false}, saw_key8[2] = {false, false}, saw_short_off_by_lds = false, saw_short_on = false;
  for (const OptSet& s : sets)
    for (int form = 0; form <= 2; ++form)
      for (int lq : kLq)
        for (int sq : kShort) {
          const int tb = tb_bytes_for(s.o, lq);
          const ExtPlan p = ext_plan(s.o, form, tb, sq);
          const ref::Round r = ref::launch_ext_round(s.o, form, tb, sq);
          const int before = g_fail;
          EXPECT(p.quad == r.quad);
          EXPECT(p.bin[0].code == ref::ext_kernel_for(s.o, form, tb));
          EXPECT(p.bin[1].code == 0);
          EXPECT(p.bin[0].phased == r.p0);
          EXPECT(p.bin[1].phased == r.p1);
          EXPECT(p.short_q == r.sort_short_q);  // what spec_sort2_scan is given
          for (int b = 0; b < 2; ++b) {
            EXPECT(p.bin[b].family == r.bin[b].family);
            EXPECT(p.bin[b].G == r.bin[b].G);
            EXPECT(p.bin[b].PMAX == r.bin[b].PMAX);
            EXPECT(p.bin[b].K8 == r.bin[b].K8);
            EXPECT(known_tuple(p.bin[b]));
            EXPECT((p.bin[b].family == SIDE4) == p.bin[b].phased);
          }
          EXPECT(p.bin[1].family != SIDE4);  // the plan's side-launch fields are the first bin's
          // launch_side_pair's arguments (no side pair: nothing to size)
          EXPECT(p.short_q == r.bin[0].short_q);
          EXPECT(p.tb_short == r.bin[0].tb_short);
          EXPECT(p.wave_lds == r.bin[0].wave_lds);
          EXPECT(p.short_q >= 0 && p.short_q <= kShortQMax);
          if (p.short_q) EXPECT(bin_is(p.bin[0], SIDE4, 16, 10, true, 18, true) && (kBlock / 64) * p.wave_lds <= 64 * 1024);
          if (g_fail != before) std::printf("  at %s, form %d, lq %d (tb %d), short_q %d\n", s.name, form, lq, tb, sq);
          const bool key8 = p.bin[0].K8;
          saw_quad[p.quad] = true;
          if (p.quad) saw_key8[key8] = true;
          if (p.bin[0].code == 18 && sq >= 1 && p.short_q == 0) saw_short_off_by_lds = true;
          if (p.short_q > 0) saw_short_on = true;
          ++n;
        }
  // every predicate was seen both ways
  EXPECT(saw_quad[0] && saw_quad[1] && saw_key8[0] && saw_key8[1] && saw_short_off_by_lds && saw_short_on);
  EXPECT(n == 5 * 3 * 7 * 6);

  // literal rows of the table (spec_plan.h)
  const DevOpt d = sets[0].o, m2 = sets[1].o, m16 = sets[2].o, ge = sets[3].o, wide = sets[4].o;
  const int tb = tb_bytes_for(d, 160);
  EXPECT(tb == 336);  // 160 + min(2 w, 160) + 2, to 16
  ExtPlan p = ext_plan(d, 0, tb, 63);
  EXPECT(p.quad && bin_is(p.bin[0], SIDE4, 16, 10, true, 18, true) && bin_is(p.bin[1], EXT4, 16, 16, false, 0, false));
  EXPECT(p.short_q == 63 && p.tb_short == 128);               // 63 + min(200, 63) + 2
  EXPECT(p.wave_lds == 4u * (2 * 336 + 2 * 96 + 2 * 160));    // the long run's 4 736 > the short run's 4 608
  EXPECT(side4_wave_lds(128, 8, 8) == 8u * (2 * 128 + 2 * 96 + 2 * 64));
  p = ext_plan(d, 0, tb, 0);
  EXPECT(p.short_q == 0 && p.tb_short == 0 && p.wave_lds == 4736 && p.bin[0].code == 18);
  p = ext_plan(d, 0, tb, 1000);
  EXPECT(p.short_q == 63);
  p = ext_plan(d, 2, tb, 63);
  EXPECT(p.quad && bin_is(p.bin[0], SIDE4, 32, 5, true, 14, true) && bin_is(p.bin[1], EXT4, 32, 8, false, 0, false));
  EXPECT(p.short_q == 0 && p.tb_short == 0 && p.wave_lds == 2u * (2 * 336 + 2 * 96 + 2 * 160));
  p = ext_plan(d, 1, tb, 63);
  EXPECT(!p.quad && bin_is(p.bin[0], EXT2, 32, 5, false, 2, false) && bin_is(p.bin[1], EXT2, 32, 8, false, 0, false));
  EXPECT(p.short_q == 0 && p.wave_lds == 0);
  for (int form = 0; form <= 2; form += 2) {
    p = ext_plan(m2, form, tb_bytes_for(m2, 160), 63);
    EXPECT(p.quad && bin_is(p.bin[0], SIDE4, 32, 8, false, 15, true) && p.short_q == 0);
    EXPECT(p.wave_lds == 2u * (2 * (size_t)tb_bytes_for(m2, 160) + 2 * 96 + 2 * 256));
    EXPECT(bin_is(p.bin[1], EXT4, form == 0 ? 16 : 32, form == 0 ? 16 : 8, false, 0, false));
    p = ext_plan(m16, form, tb_bytes_for(m16, 160), 63);
    EXPECT(!p.quad && p.bin[0].code == 2 && p.bin[1].family == EXT2);
    p = ext_plan(ge, form, tb_bytes_for(ge, 160), 63);
    EXPECT(!p.quad && p.bin[0].code == 2 && p.bin[1].family == EXT2);
  }
  EXPECT(quad_scores_ok(ge, 256) && !quad_rows_ok(ge, tb_bytes_for(ge, 160)));
  p = ext_plan(wide, 0, tb_bytes_for(wide, 160), 63);
  EXPECT(tb_bytes_for(wide, 160) > 1792);  // four waves x 4 groups x 2 rows pass 64 KB
  EXPECT(p.quad && p.bin[0].code == 18 && p.short_q == 0 && p.tb_short == 0);

  // the plan at the edges of its gates (quad_scores_ok(o, 256), quad_rows_ok(o, tb_bytes),
  // quad_key8_ok(o, 160); pure.h), the option sets of tests/test_gpu_packed_ranges.py:
  auto scored = [](int a) {
    DevOpt o = default_opt();
    o.a = o.max_mat = a;
    for (int i = 0; i < 4; ++i) o.mat[i * 5 + i] = (int8_t)a;
    return o;
  };
  auto ext_gap = [](DevOpt o, int e) {
    o.e_del = o.e_ins = e, o.oe_del = o.o_del + e, o.oe_ins = o.o_ins + e;
    return o;
  };
  // max_mat 7: hb = 256 * 7 = 1792, (1792 << 3) + 128 = 14464; max_mat 8: (2048 << 4) + 128 = 32896
  p = ext_plan(scored(7), 0, tb_bytes_for(scored(7), 257), 63);
  EXPECT(p.quad && bin_is(p.bin[0], SIDE4, 32, 8, false, 15, true) && bin_is(p.bin[1], EXT4, 16, 16, false, 0, false));
  p = ext_plan(scored(8), 0, tb_bytes_for(scored(8), 257), 63);
  EXPECT(!p.quad && p.bin[0].code == 2 && p.bin[1].family == EXT2);
  EXPECT(quad_scores_ok(scored(7), 256) && !quad_scores_ok(scored(8), 256));
  // reads up to 250: the band cap (250 + 5 - 6) / e + 1 is 5 at e = 54 and 55, so 250 + 5 + 2 -> 272
  // row bytes; (272 + 256) * 54 = 28512 < 28672 <= 29040 = 528 * 55.  Reads up to 257: 272 too.
  for (int lq : {250, 257}) {
    EXPECT(tb_bytes_for(ext_gap(d, 54), lq) == 272 && tb_bytes_for(ext_gap(d, 55), lq) == 272);
    p = ext_plan(ext_gap(d, 54), 0, 272, 63);
    EXPECT(p.quad && p.bin[0].code == 18);
    p = ext_plan(ext_gap(d, 55), 0, 272, 63);
    EXPECT(!p.quad && p.bin[0].code == 2);
  }
  // reads up to 150: the cap (150 + 5 - 6) / e + 1 is 3, 150 + 3 + 2 -> 160; 416 * 68 = 28288, 416 * 69 = 28704
  EXPECT(tb_bytes_for(ext_gap(d, 68), 150) == 160 && tb_bytes_for(ext_gap(d, 69), 150) == 160);
  EXPECT(ext_plan(ext_gap(d, 68), 0, 160, 63).quad && !ext_plan(ext_gap(d, 69), 0, 160, 63).quad);
  EXPECT(quad_scores_ok(ext_gap(d, 69), 256));  // the rows gate alone refuses it
  // max_mat 7 with e = 54: the cap grows with the scores ((257 * 7 + 5 - 6) / 54 + 1 = 34), 257 + 34 + 2 ->
  // 304 row bytes, 560 * 54 = 30240: the rows gate refuses what either option alone passes
  EXPECT(tb_bytes_for(ext_gap(scored(7), 54), 257) == 304 && quad_scores_ok(ext_gap(scored(7), 54), 256));
  EXPECT(!ext_plan(ext_gap(scored(7), 54), 0, 304, 63).quad);
  // the first bin's 8-bit key: 160 * max_mat <= 255
  EXPECT(quad_key8_ok(d, 160) && quad_key8_ok(d, 255) && !quad_key8_ok(d, 256) && !quad_key8_ok(scored(2), 128));

  if (g_fail) {
    std::printf("ext_plan_asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("ext_plan_asan OK (%d plans)\n", n);
  return 0;
}
