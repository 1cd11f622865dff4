// pairsel_host.h — host-side argument validation, span arithmetic and tables
// of bwagpu_mark_primary and bwagpu_pair_select (capi.hip).  Plain C++:
// compiles without HIP, so that the checks run under the host sanitizers
// (tests/cpp/pairsel_host_asan.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bwagpu.h"
#include "rescue_host.h"

namespace bwagpu {

constexpr int32_t kSelLogN = 1 << 16;  // the context's log table: log(k), k < kSelLogN
constexpr int32_t kSelRefused =
    BWAGPU_MEM_F_ALL | BWAGPU_MEM_F_NO_MULTI | BWAGPU_MEM_F_PRIMARY5 | BWAGPU_MEM_F_KEEP_SUPP_MAPQ;

// What a validated call moves: regs[lo, hi) holds every read's span.
struct SelPlan {
  int64_t lo = 0, hi = 0;
  int64_t n_regs = 0;
};

inline bool sel_opt_ok(const bwagpu_selopt_t* s) {
  return s && std::isfinite(s->mask_level) && s->mask_level >= 0.f && std::isfinite(s->drop_ratio) &&
         std::isfinite(s->mapQ_coef_len) && s->min_seed_len >= 0 && s->min_seed_len <= 65535 && s->flags >= 0;
}

// spans_check (rescue_host.h) and pairwise disjoint spans: the passes write in place
inline int sel_spans_check(int32_t n_reads, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                           SelPlan* plan, const char** why) {
  if (int rc = spans_check(n_reads, reg_off, regs, n, &plan->lo, &plan->hi, &plan->n_regs, why)) return rc;
  std::vector<int32_t> used;
  for (int32_t r = 0; r < n_reads; ++r)
    if (n[r]) used.push_back(r);
  std::sort(used.begin(), used.end(), [&](int32_t x, int32_t y) { return reg_off[x] < reg_off[y]; });
  for (size_t k = 1; k < used.size(); ++k)
    if (reg_off[used[k - 1]] + n[used[k - 1]] > reg_off[used[k]]) return *why = "region spans overlap", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// bwagpu_mark_primary.  BWAGPU_OK, or BWAGPU_E_INVAL with *why set.  Nothing is
// read beyond reg_off[n_reads - 1] and n[n_reads - 1].
inline int mark_check(const bwagpu_selopt_t* sopt, int32_t n_reads, const int64_t* reg_off,
                      const bwagpu_alnreg_t* regs, const int32_t* n, const int32_t* n_pri, const int32_t* status,
                      SelPlan* plan, const char** why) {
  *plan = SelPlan{};
  *why = "";
  if (!sel_opt_ok(sopt)) return *why = "bad bwagpu_selopt_t", BWAGPU_E_INVAL;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!reg_off || !n || !n_pri || !status) return *why = "NULL array", BWAGPU_E_INVAL;
  return sel_spans_check(n_reads, reg_off, regs, n, plan, why);
}

// bwagpu_pair_select.  BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED with *why set.
inline int pairsel_check(const bwagpu_selopt_t* sopt, const bwagpu_pestat_t* pes, int32_t n_reads,
                         const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n, const int32_t* n_pri,
                         const bwagpu_pairsel_t* sel, const int32_t* out_mapq, int32_t n_seqs, SelPlan* plan,
                         const char** why) {
  *plan = SelPlan{};
  *why = "";
  if (!sel_opt_ok(sopt)) return *why = "bad bwagpu_selopt_t", BWAGPU_E_INVAL;
  if (sopt->flags & kSelRefused)
    return *why = "MEM_F_ALL, MEM_F_NO_MULTI, MEM_F_PRIMARY5 and MEM_F_KEEP_SUPP_MAPQ are not implemented",
           BWAGPU_E_UNSUPPORTED;
  if (int rc = pes_check(pes, why)) return rc;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads & 1) return *why = "odd read count: reads 2i and 2i+1 are a pair", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!reg_off || !n || !n_pri || !sel) return *why = "NULL array", BWAGPU_E_INVAL;
  if (int rc = sel_spans_check(n_reads, reg_off, regs, n, plan, why)) return rc;
  if (plan->n_regs && !out_mapq) return *why = "NULL out_mapq", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (n_pri[r] < 0 || n_pri[r] > n[r]) return *why = "n_pri outside [0, n]", BWAGPU_E_INVAL;
    const bwagpu_alnreg_t* a = regs + reg_off[r];
    for (int32_t k = 0; k < n_pri[r]; ++k)
      if (a[k].rid < 0 || a[k].rid >= n_seqs) return *why = "a region's rid lies outside the reference", BWAGPU_E_INVAL;
  }
  return BWAGPU_OK;
}

// The tables are filled with the host's libm in the reference's order of
// operations; its build (x86-64, -O2) has no fused multiply-add.
inline void fill_log_table(double* t, int32_t n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int32_t k = 0; k < n; ++k) t[k] = std::log((double)k);
}

// entries of a live orientation's table: dist - low for dist in [low, high]
inline int64_t erfc_table_len(const bwagpu_pestat_t& p) { return p.failed ? 0 : (int64_t)p.high - p.low + 1; }

// t[dist - low] = .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)), ns = (dist - avg) / std  (bwamem_pair.c:220-221)
inline void fill_erfc_table(const bwagpu_pestat_t& p, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int64_t len = erfc_table_len(p);
  for (int64_t d = 0; d < len; ++d) {
    const int64_t dist = (int64_t)p.low + d;
    const double ns = (dist - p.avg) / p.std;
    t[d] = .721 * std::log(2. * std::erfc(std::fabs(ns) * M_SQRT1_2));
  }
}

}  // namespace bwagpu
