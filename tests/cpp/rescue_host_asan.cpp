// rescue_host_asan.cpp — the host-side argument validation and span arithmetic
// of bwagpu_pestat and bwagpu_mate_rescue (bwa-flow_amd/csrc/stage_host.h)
// under the host sanitizers.  Stand-alone: no GPU, no HIP, not loaded into any
// other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/rescue_host_asan.cpp -o rescue_host_asan && ./rescue_host_asan
//
// Every array handed to the checks is a heap allocation of exactly the size the
// ABI promises, so a read past seq_off[n_reads], out_off[n_reads],
// reg_off[n_reads - 1], n[n_reads - 1] or a read's span is an AddressSanitizer
// report.
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

static bwagpu_pairopt_t dflt() { return bwagpu_pairopt_t{10000, 50, 17, 19, 10000, 0.95f, 0.50f, 3}; }

struct Case {
  std::vector<int64_t> seq_off, reg_off, out_off;
  std::vector<uint8_t> seq;
  std::vector<bwagpu_alnreg_t> regs;
  std::vector<int32_t> n;
  bwagpu_pairopt_t po = dflt();
  bwagpu_pestat_t pes[4] = {{0, 0, 1, 0, 0., 0.}, {200, 600, 0, 0, 400., 50.}, {0, 0, 1, 0, 0., 0.}, {0, 0, 1, 0, 0., 0.}};
  StagePlan plan;
  const char* why = nullptr;
  template <class V>
  static typename V::value_type* dup(const V& v) {  // exact-size copies: a vector's capacity may exceed its size
    using T = typename V::value_type;
    T* p = (T*)std::malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
  }
  int run() {
    int64_t *so = dup(seq_off), *ro = dup(reg_off), *oo = dup(out_off);
    uint8_t* sq = dup(seq);
    bwagpu_alnreg_t* rg = dup(regs);
    int32_t* nn = dup(n);
    const size_t nr = n.size();
    std::vector<bwagpu_alnreg_t> out(out_off.empty() || out_off.back() < 1 ? 1 : (size_t)out_off.back());
    std::vector<int32_t> out_n(nr + 1), status(nr / 2 + 1), n_sw(nr / 2 + 1);
    const int rc = rescue_check(&po, pes, (int32_t)nr, so, sq, ro, rg, nn, oo, out.data(), out_n.data(), status.data(),
                                n_sw.data(), &plan, &why);
    std::free(so), std::free(ro), std::free(oo), std::free(sq), std::free(rg), std::free(nn);
    return rc;
  }
  int run_pestat(int32_t n_reads) {
    int64_t* ro = dup(reg_off);
    bwagpu_alnreg_t* rg = dup(regs);
    int32_t* nn = dup(n);
    bwagpu_pestat_t out[4];
    const int rc = pestat_check(&po, n_reads, ro, rg, nn, out, &plan, &why);
    std::free(ro), std::free(rg), std::free(nn);
    return rc;
  }
};

static bwagpu_alnreg_t reg(int64_t rb, int64_t re, int qb, int qe) {
  bwagpu_alnreg_t r;
  std::memset(&r, 0, sizeof r);
  r.rb = rb, r.re = re, r.qb = qb, r.qe = qe, r.score = qe - qb;
  return r;
}

// two pairs of 100-base reads; input spans out of order and with a gap: read 0
// at regs[5..7), read 1 empty, read 2 at regs[1..4), read 3 at regs[4..5)
static Case base() {
  Case c;
  c.seq_off = {50, 150, 250, 350, 450};
  c.seq.assign(450, 0);
  c.regs.assign(7, reg(1000, 1100, 0, 100));
  c.reg_off = {5, 0, 1, 4};
  c.n = {2, 0, 3, 1};
  c.out_off = {10, 20, 28, 39, 48};
  return c;
}

int main() {
  {
    Case c = base();
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(c.plan.lo == 1 && c.plan.hi == 7 && c.plan.n_regs == 6);
    EXPECT(c.plan.seq_lo == 50 && c.plan.seq_hi == 450 && c.plan.out_lo == 10 && c.plan.out_hi == 48);
    EXPECT(c.run_pestat(4) == BWAGPU_OK && c.plan.lo == 1 && c.plan.hi == 7);
  }
  {  // an empty batch reads nothing at all
    bwagpu_pairopt_t po = dflt();
    Case c = base();
    StagePlan plan;
    const char* why = nullptr;
    bwagpu_pestat_t out[4];
    EXPECT(rescue_check(&po, c.pes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, &plan, &why) == BWAGPU_OK);
    EXPECT(rescue_check(nullptr, c.pes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(rescue_check(&po, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(rescue_check(&po, c.pes, -2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(rescue_check(&po, c.pes, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(pestat_check(&po, 0, nullptr, nullptr, nullptr, out, &plan, &why) == BWAGPU_OK);
    EXPECT(pestat_check(&po, 1, nullptr, nullptr, nullptr, out, &plan, &why) == BWAGPU_OK);  // n >> 1 == 0
    EXPECT(pestat_check(&po, 2, nullptr, nullptr, nullptr, out, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(pestat_check(&po, -1, nullptr, nullptr, nullptr, out, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(pestat_check(&po, 0, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
  }
  {  // an odd read count: refused by the rescue; mem_pestat ignores the last read (its arrays end before it)
    Case c = base();
    c.n.pop_back();
    c.reg_off.pop_back();
    c.seq_off.pop_back();
    c.out_off.pop_back();
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.n.pop_back();
    c.reg_off.pop_back();
    EXPECT(c.run_pestat(3) == BWAGPU_OK);
    EXPECT(c.plan.lo == 5 && c.plan.hi == 7 && c.plan.n_regs == 2);
  }
  {  // every read without regions: the (dangling) offsets are never used
    Case c = base();
    c.n = {0, 0, 0, 0};
    c.reg_off = {std::numeric_limits<int64_t>::max(), -5, 1 << 30, 7};
    c.regs.clear();
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(c.plan.n_regs == 0 && c.plan.lo == 0 && c.plan.hi == 0);
    EXPECT(c.run_pestat(4) == BWAGPU_OK);
  }
  {  // negative count; offsets that would overflow the byte arithmetic
    Case c = base();
    c.n[2] = -3;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    EXPECT(c.run_pestat(4) == BWAGPU_E_INVAL);
    c = base();
    c.reg_off[0] = std::numeric_limits<int64_t>::max() - 1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off[0] = std::numeric_limits<int64_t>::max() / 88;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off[0] = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    EXPECT(c.run_pestat(4) == BWAGPU_E_INVAL);
  }
  {  // overlapping input spans are legal here: neither pass writes its input (spans_check, disjoint = false)
    Case c = base();
    c.reg_off = {3, 0, 1, 4};  // read 0 at regs[3..5), inside read 2's regs[1..4) and over read 3's regs[4..5)
    EXPECT(c.run() == BWAGPU_OK && c.plan.lo == 1 && c.plan.hi == 5 && c.plan.n_regs == 6);
    EXPECT(c.run_pestat(4) == BWAGPU_OK && c.plan.lo == 1 && c.plan.hi == 5 && c.plan.n_regs == 6);
    c.reg_off = {1, 0, 1, 1};  // three spans from the same record on
    EXPECT(c.run() == BWAGPU_OK && c.plan.lo == 1 && c.plan.hi == 4);
    StagePlan p;
    const char* why = "";
    int64_t off[2] = {0, 1};
    int32_t n[2] = {3, 2};
    EXPECT(spans_check(2, off, c.regs.data(), n, false, &p, &why) == BWAGPU_OK && p.lo == 0 && p.hi == 3);
    EXPECT(spans_check(2, off, c.regs.data(), n, true, &p, &why) == BWAGPU_E_INVAL && !std::strcmp(why, "region spans overlap"));
  }
  {  // reads: descending offsets, a negative start, a base over 4
    Case c = base();
    c.seq_off[2] = 100;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.seq_off[0] = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.seq[449] = 5;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.seq[449] = 4;
    c.seq[49] = 9;  // before the first read: never looked at
    EXPECT(c.run() == BWAGPU_OK);
  }
  {  // output spans: descending, smaller than the input, exactly as large
    Case c = base();
    c.out_off = {10, 20, 19, 39, 48};
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.out_off = {10, 11, 11, 39, 48};
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.out_off = {10, 12, 12, 15, 16};
    EXPECT(c.run() == BWAGPU_OK);
    c.out_off[0] = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
  }
  {  // qb / qe against the read they belong to
    Case c = base();
    c.regs[3].qe = 101;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.regs[3].qe = 100;
    c.regs[3].qb = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.regs[3].qb = 60;
    c.regs[3].qe = 60;
    EXPECT(c.run() == BWAGPU_OK);
    c.regs[0].qe = 5000;  // regs[0] belongs to no span: never looked at
    EXPECT(c.run() == BWAGPU_OK);
  }
  {  // options and pes
    Case c = base();
    c.po.max_rounds = 0;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.po.max_rounds = kRescueHostMaxRounds + 1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.po.min_seed_len = 0;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.po.max_matesw = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.po.mask_level_redun = std::numeric_limits<float>::quiet_NaN();
    EXPECT(c.run() == BWAGPU_E_INVAL);
    EXPECT(c.run_pestat(4) == BWAGPU_E_INVAL);
    c = base();
    c.pes[1].high = 199;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.pes[1].low = std::numeric_limits<int32_t>::min();
    c.pes[1].high = std::numeric_limits<int32_t>::max();
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED);
    c.pes[1].failed = 1;  // a failed orientation's range is never used
    EXPECT(c.run() == BWAGPU_OK);
  }
  if (g_fail) {
    std::printf("rescue_host_asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("rescue_host_asan OK\n");
  return 0;
}
