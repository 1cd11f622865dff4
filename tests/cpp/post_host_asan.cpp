// post_host_asan.cpp — the host-side argument validation and span arithmetic
// of bwagpu_regs_post (bwa-flow_amd/csrc/stage_host.h) under the host
// sanitizers.  Stand-alone: no GPU, no HIP, not loaded into any other process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I bwa-flow_amd/csrc tests/cpp/post_host_asan.cpp -o post_host_asan && ./post_host_asan
//
// Every array handed to post_check is a heap allocation of exactly the size
// the ABI promises, so a read past seq_off[n_reads], reg_off[n_reads - 1],
// n[n_reads - 1] or a read's span is an AddressSanitizer report.
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

struct Case {
  std::vector<int64_t> seq_off, reg_off;
  std::vector<uint8_t> seq;
  std::vector<bwagpu_alnreg_t> regs;
  std::vector<int32_t> n;
  bwagpu_postopt_t po{10000, 0.95f, 0.50f, 0};
  int32_t flags = 3;
  StagePlan plan;
  const char* why = nullptr;
  int run() {
    // exact-size copies: the vectors' capacity may exceed their size
    auto dup = [](const auto& v) {
      using T = typename std::decay<decltype(v)>::type::value_type;
      T* p = (T*)std::malloc(v.size() ? v.size() * sizeof(T) : 1);
      if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
      return p;
    };
    int64_t* so = dup(seq_off);
    int64_t* ro = dup(reg_off);
    uint8_t* sq = dup(seq);
    bwagpu_alnreg_t* rg = dup(regs);
    int32_t* nn = dup(n);
    const int rc = post_check(&po, flags, (int32_t)n.size(), so, sq, ro, rg, nn, &plan, &why);
    std::free(so);
    std::free(ro);
    std::free(sq);
    std::free(rg);
    std::free(nn);
    return rc;
  }
};

static bwagpu_alnreg_t reg(int64_t rb, int64_t re, int qb, int qe) {
  bwagpu_alnreg_t r;
  std::memset(&r, 0, sizeof r);
  r.rb = rb;
  r.re = re;
  r.qb = qb;
  r.qe = qe;
  r.score = qe - qb;
  return r;
}

// three reads of 100 bases; spans out of order and with a gap: read 0 at
// regs[5..7), read 1 empty, read 2 at regs[1..4)
static Case base() {
  Case c;
  c.seq_off = {50, 150, 250, 350};
  c.seq.assign(350, 0);
  c.regs.assign(7, reg(1000, 1100, 0, 100));
  c.reg_off = {5, 0, 1};
  c.n = {2, 0, 3};
  return c;
}

int main() {
  {
    Case c = base();
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(c.plan.lo == 1 && c.plan.hi == 7 && c.plan.n_regs == 5);
    EXPECT(c.plan.seq_lo == 50 && c.plan.seq_hi == 350);
  }
  {  // an empty batch reads nothing at all
    bwagpu_postopt_t po{10000, 0.95f, 0.50f, 0};
    StagePlan plan;
    const char* why = nullptr;
    EXPECT(post_check(&po, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_OK);
    EXPECT(plan.n_regs == 0 && plan.hi == 0);
    EXPECT(post_check(nullptr, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(post_check(&po, 3, -1, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(post_check(&po, 3, 1, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(post_check(&po, 8, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
    EXPECT(post_check(&po, 4, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_UNSUPPORTED);
    EXPECT(post_check(&po, -1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &plan, &why) == BWAGPU_E_INVAL);
  }
  {  // every read without regions: the (dangling) offsets are never used
    Case c = base();
    c.n = {0, 0, 0};
    c.reg_off = {std::numeric_limits<int64_t>::max(), -5, 1 << 30};
    c.regs.clear();
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(c.plan.n_regs == 0 && c.plan.lo == 0 && c.plan.hi == 0);
  }
  {  // negative count
    Case c = base();
    c.n[2] = -3;
    EXPECT(c.run() == BWAGPU_E_INVAL);
  }
  {  // overlapping spans, in either order, and touching spans
    Case c = base();
    c.reg_off = {3, 0, 1};
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off = {0, 0, 1};
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off = {4, 0, 1};
    EXPECT(c.run() == BWAGPU_OK);
    EXPECT(c.plan.lo == 1 && c.plan.hi == 6);
  }
  {  // offsets that would overflow the byte arithmetic
    Case c = base();
    c.reg_off[0] = std::numeric_limits<int64_t>::max() - 1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off[0] = std::numeric_limits<int64_t>::max() / 88;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.reg_off[0] = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
  }
  {  // reads: descending offsets, a negative start, the length limit
    Case c = base();
    c.seq_off[2] = 100;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.seq_off[0] = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.seq_off = {0, BWAGPU_MAX_READ_LEN, 2 * BWAGPU_MAX_READ_LEN, 3 * BWAGPU_MAX_READ_LEN};
    c.seq.assign(3 * BWAGPU_MAX_READ_LEN, 0);
    EXPECT(c.run() == BWAGPU_OK);
    c.seq_off[3] += 1;
    c.seq.push_back(0);
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED);
  }
  {  // qb / qe against the read they belong to (the last region of the last span)
    Case c = base();
    c.regs[3].qe = 101;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.regs[3].qe = 100;
    c.regs[3].qb = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.regs[3].qb = 60;
    c.regs[3].qe = 59;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c.regs[3].qe = 60;  // an excluded hit (qe == qb) is legal input
    EXPECT(c.run() == BWAGPU_OK);
    c.regs[0].qe = 5000;  // regs[0] belongs to no span: never looked at
    EXPECT(c.run() == BWAGPU_OK);
  }
  {  // the order of verdicts: overlapping spans, then the length limit, then qb / qe
    Case c = base();
    c.seq_off = {0, 100, 200, 201 + BWAGPU_MAX_READ_LEN};  // read 2 is one base over the limit
    c.seq.assign((size_t)c.seq_off[3], 0);
    c.reg_off = {3, 0, 1};  // read 0's span starts inside read 2's
    EXPECT(c.run() == BWAGPU_E_INVAL && !std::strcmp(c.why, "region spans overlap"));
    EXPECT(c.plan.n_regs == 0 && c.plan.hi == 0 && c.plan.seq_hi == 0);  // a refused call has no plan
    c.reg_off = {5, 0, 1};
    c.regs[5].qe = 101;  // read 0 has 100 bases
    EXPECT(c.run() == BWAGPU_E_UNSUPPORTED && !std::strcmp(c.why, "read longer than BWAGPU_MAX_READ_LEN"));
    c.seq_off[3] -= 1;
    EXPECT(c.run() == BWAGPU_E_INVAL && !std::strcmp(c.why, "a region's qb/qe lie outside its read"));
  }
  {  // two spans that touch (off[a] + n[a] == off[b]) do not overlap
    Case c = base();
    c.reg_off = {4, 0, 1};  // read 2 at regs[1..4), read 0 at regs[4..6)
    EXPECT(c.run() == BWAGPU_OK && c.plan.lo == 1 && c.plan.hi == 6 && c.plan.n_regs == 5);
    c.reg_off = {0, 0, 2};  // read 0 at regs[0..2), read 2 at regs[2..5)
    EXPECT(c.run() == BWAGPU_OK && c.plan.lo == 0 && c.plan.hi == 5);
  }
  {  // options
    Case c = base();
    c.po.max_chain_gap = -1;
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.po.mask_level_redun = std::numeric_limits<float>::quiet_NaN();
    EXPECT(c.run() == BWAGPU_E_INVAL);
    c = base();
    c.po.mask_level = std::numeric_limits<float>::infinity();
    EXPECT(c.run() == BWAGPU_E_INVAL);
  }
  if (g_fail) {
    std::printf("post_host_asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("post_host_asan OK\n");
  return 0;
}
