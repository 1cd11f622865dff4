// pairsel_host_asan.cpp — the host-side argument validation, span arithmetic
// and tables of bwagpu_mark_primary and bwagpu_pair_select
// (bwa-flow_amd/csrc/stage_host.h) under the host sanitizers.  Stand-alone:
// no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/pairsel_host_asan.cpp -o pairsel_host_asan && ./pairsel_host_asan
//
// Every array handed to the checks is a heap allocation of exactly the size the
// ABI promises, so a read past reg_off[n_reads - 1], n[n_reads - 1],
// n_pri[n_reads - 1], a read's span or a table's end is an AddressSanitizer
// report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "stage_host.h"

using namespace bwagpu;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

static bwagpu_selopt_t dflt(int32_t flags = 0) { return bwagpu_selopt_t{30, 17, 19, 50.f, 3, 0.5f, 0.5f, flags}; }

struct Case {
  std::vector<int64_t> reg_off;
  std::vector<bwagpu_alnreg_t> regs;
  std::vector<int32_t> n, n_pri;
  bwagpu_selopt_t so = dflt();
  bwagpu_pestat_t pes[4] = {{0, 0, 1, 0, 0., 0.}, {200, 600, 0, 0, 400., 50.}, {0, 0, 1, 0, 0., 0.}, {0, 0, 1, 0, 0., 0.}};
  int32_t n_seqs = 3;
  StagePlan plan;
  const char* why = nullptr;
  template <class V>
  static typename V::value_type* dup(const V& v) {  // exact-size copies: a vector's capacity may exceed its size
    using T = typename V::value_type;
    T* p = (T*)std::malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
  }
  int run_mark() {
    int64_t* ro = dup(reg_off);
    bwagpu_alnreg_t* rg = dup(regs);
    int32_t* nn = dup(n);
    std::vector<int32_t> out(n.size() + 1), status(n.size() + 1);
    const int rc = mark_check(&so, (int32_t)n.size(), ro, rg, nn, out.data(), status.data(), &plan, &why);
    std::free(ro), std::free(rg), std::free(nn);
    return rc;
  }
  int run_sel() {
    int64_t* ro = dup(reg_off);
    bwagpu_alnreg_t* rg = dup(regs);
    int32_t *nn = dup(n), *np = dup(n_pri);
    std::vector<bwagpu_pairsel_t> sel(n.size() / 2 + 1);
    std::vector<int32_t> mapq(regs.size() + 1);
    const int rc = pairsel_check(&so, pes, (int32_t)n.size(), ro, rg, nn, np, sel.data(), mapq.data(), n_seqs, &plan, &why);
    std::free(ro), std::free(rg), std::free(nn), std::free(np);
    return rc;
  }
};

static bwagpu_alnreg_t reg(int32_t rid) {
  bwagpu_alnreg_t r;
  std::memset(&r, 0, sizeof r);
  r.rb = 1000, r.re = 1100, r.qe = 100, r.score = 100, r.rid = rid;
  return r;
}

// two pairs; spans out of order and with a gap: read 0 at regs[5..7), read 1
// empty, read 2 at regs[1..4), read 3 at regs[4..5)
static Case base() {
  Case c;
  c.regs.assign(7, reg(1));
  c.reg_off = {5, 0, 1, 4};
  c.n = {2, 0, 3, 1};
  c.n_pri = {2, 0, 1, 1};
  return c;
}

int main() {
  {
    Case c = base();
    EXPECT(c.run_mark() == BWAGPU_OK);
    EXPECT(c.plan.lo == 1 && c.plan.hi == 7 && c.plan.n_regs == 6);
    EXPECT(c.run_sel() == BWAGPU_OK);
    EXPECT(c.plan.lo == 1 && c.plan.hi == 7 && c.plan.n_regs == 6);
  }
  {  // an empty batch reads nothing at all
    bwagpu_selopt_t so = dflt();
    Case c = base();
    StagePlan plan;
    const char* why = nullptr;
    EXPECT(mark_check(&so, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_OK);
    EXPECT(mark_check(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(mark_check(&so, -1, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(mark_check(&so, 2, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(pairsel_check(&so, c.pes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, &plan, &why) == BWAGPU_OK);
    EXPECT(pairsel_check(&so, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, &plan, &why) ==
           BWAGPU_E_INVAL);
    EXPECT(pairsel_check(nullptr, c.pes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, &plan, &why) ==
           BWAGPU_E_INVAL);
    EXPECT(pairsel_check(&so, c.pes, -2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, &plan, &why) ==
           BWAGPU_E_INVAL);
    EXPECT(pairsel_check(&so, c.pes, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, &plan, &why) ==
           BWAGPU_E_INVAL);
  }
  {  // an odd read count: fine for the marking, refused by the selection
    Case c = base();
    c.n.pop_back(), c.reg_off.pop_back(), c.n_pri.pop_back();
    EXPECT(c.run_mark() == BWAGPU_OK);
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
  }
  {  // every read without regions: the (dangling) offsets are never used
    Case c = base();
    c.n = {0, 0, 0, 0};
    c.n_pri = {0, 0, 0, 0};
    c.reg_off = {std::numeric_limits<int64_t>::max(), -5, 1 << 30, 7};
    c.regs.clear();
    EXPECT(c.run_mark() == BWAGPU_OK && c.plan.n_regs == 0 && c.plan.lo == 0 && c.plan.hi == 0);
    EXPECT(c.run_sel() == BWAGPU_OK);
  }
  {  // negative counts; offsets that would overflow the byte arithmetic; overlapping spans
    Case c = base();
    c.n[2] = -3;
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
    c = base();
    c.reg_off[0] = std::numeric_limits<int64_t>::max() - 1;
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
    c.reg_off[0] = -1;
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
    c = base();
    c.reg_off[3] = 3;  // inside read 2's span
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
    c.reg_off[3] = 0;  // regs[0..1): touches read 2's span, does not overlap it
    EXPECT(c.run_mark() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 7);
  }
  {  // two spans that touch (off[a] + n[a] == off[b]) do not overlap: every span of this layout touches the next
    Case c = base();
    c.reg_off = {5, 0, 0, 3};  // read 2 at regs[0..3), read 3 at regs[3..4), read 0 at regs[5..7)
    EXPECT(c.run_mark() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 7 && c.plan.n_regs == 6);
    EXPECT(c.run_sel() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 7 && c.plan.n_regs == 6);
    c.reg_off = {4, 0, 0, 3};  // ... and read 0 at regs[4..6)
    EXPECT(c.run_mark() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 6);
    EXPECT(c.run_sel() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 6);
    c.reg_off = {3, 0, 0, 3};  // read 0 and read 3 start at the same record
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
  }
  {  // n_pri and rid
    Case c = base();
    c.n_pri[2] = 4;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    c.n_pri[2] = -1;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    c = base();
    c.regs[1].rid = 3;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    c.regs[1].rid = -1;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    c.regs[1].rid = 0;
    c.regs[2].rid = 7;  // read 2's second region lies beyond its n_pri: mem_pair never sees it
    c.regs[0].rid = 9;  // regs[0] belongs to no span
    EXPECT(c.run_sel() == BWAGPU_OK);
  }
  {  // options, flags and pes
    Case c = base();
    c.so.mask_level = std::numeric_limits<float>::quiet_NaN();
    EXPECT(c.run_mark() == BWAGPU_E_INVAL && c.run_sel() == BWAGPU_E_INVAL);
    c = base();
    c.so.flags = -1;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    for (int32_t f : {BWAGPU_MEM_F_ALL, BWAGPU_MEM_F_NO_MULTI, BWAGPU_MEM_F_PRIMARY5, BWAGPU_MEM_F_KEEP_SUPP_MAPQ}) {
      c.so = dflt(f | BWAGPU_MEM_F_NOPAIRING);
      EXPECT(c.run_sel() == BWAGPU_E_UNSUPPORTED);
      EXPECT(c.run_mark() == BWAGPU_OK);  // the marking reads mask_level only
    }
    c.so = dflt(BWAGPU_MEM_F_NOPAIRING | 0x2 | 0x20 | 0x200);  // bits the pass does not read
    EXPECT(c.run_sel() == BWAGPU_OK);
    c = base();
    c.pes[1].high = 199;
    EXPECT(c.run_sel() == BWAGPU_E_INVAL);
    c.pes[1].low = std::numeric_limits<int32_t>::min();
    c.pes[1].high = std::numeric_limits<int32_t>::max();
    EXPECT(c.run_sel() == BWAGPU_E_UNSUPPORTED);
    c.pes[1].failed = 1;  // a failed orientation's range is never used
    EXPECT(c.run_sel() == BWAGPU_OK);
  }
  {  // the tables: exact-size heap buffers
    Case c = base();
    EXPECT(erfc_table_len(c.pes[0]) == 0 && erfc_table_len(c.pes[1]) == 401);
    double* t = (double*)std::malloc(sizeof(double) * 401);
    fill_erfc_table(c.pes[1], t);
    EXPECT(t[200] == .721 * std::log(2. * std::erfc(0.)));                    // dist == avg
    EXPECT(t[0] == t[400] && t[0] < t[200] && std::isfinite(t[0]));             // symmetric about the mean
    std::free(t);
    bwagpu_pestat_t wide = {1, 1 << 20, 0, 0, 400., 50.};  // erfc underflows: log(0)
    const int64_t len = erfc_table_len(wide);
    EXPECT(len == 1 << 20);
    t = (double*)std::malloc(sizeof(double) * (size_t)len);
    fill_erfc_table(wide, t);
    EXPECT(std::isinf(t[len - 1]) && t[len - 1] < 0);
    std::free(t);
    bwagpu_pestat_t one = {5, 5, 0, 0, 5., 0.};  // std == 0 at the mean: 0 / 0
    double v = 0;
    EXPECT(erfc_table_len(one) == 1);
    fill_erfc_table(one, &v);
    EXPECT(std::isnan(v));
    double* lg = (double*)std::malloc(sizeof(double) * (size_t)kSelLogN);
    fill_log_table(lg, kSelLogN);
    EXPECT(std::isinf(lg[0]) && lg[1] == 0. && lg[kSelLogN - 1] == std::log((double)(kSelLogN - 1)));
    std::free(lg);
  }
  if (g_fail) {
    std::printf("pairsel_host_asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("pairsel_host_asan OK\n");
  return 0;
}
