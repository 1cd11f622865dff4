// stage_host.h — host-side argument validation, span arithmetic and tables of
// the stages that run after mem_chain2aln (capi_stages.hip): bwagpu_regs_post,
// bwagpu_pestat, bwagpu_mate_rescue, bwagpu_mark_primary, bwagpu_pair_select.
// Plain C++: compiles without HIP, so that the checks run under the host
// sanitizers (tests/cpp/*_host_asan.cpp).
//
// Every *_check returns BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED
// with *why set, and reads nothing beyond seq_off[n_reads], out_off[n_reads],
// reg_off[n_reads - 1], n[n_reads - 1] and the spans those describe.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bwagpu.h"

namespace bwagpu {

constexpr int kRescueHostMaxRounds = 8;       // == kRescueMaxRounds (rescue.h)
constexpr int64_t kRescueMaxRange = 1 << 20;  // pes[r].high - pes[r].low of a live orientation
constexpr int32_t kSelLogN = 1 << 16;         // the context's log table: log(k), k < kSelLogN

// What a validated call moves: regs[lo, hi) holds every read's input span,
// out_regs[out_lo, out_hi) every output span, the bases are seq[seq_lo, seq_hi).
// A stage without output spans or bases leaves those at 0.
struct StagePlan {
  int64_t lo = 0, hi = 0;
  int64_t out_lo = 0, out_hi = 0;
  int64_t seq_lo = 0, seq_hi = 0;
  int64_t n_regs = 0;  // sum of n
};

inline bool post_opt_ok(const bwagpu_postopt_t* p) {
  return p && p->max_chain_gap >= 0 && std::isfinite(p->mask_level_redun) && std::isfinite(p->mask_level) &&
         p->mask_level_redun >= 0.f && p->mask_level >= 0.f;
}

inline bool pair_opt_ok(const bwagpu_pairopt_t* p) {
  return p && p->max_ins >= 0 && p->max_matesw >= 0 && p->max_matesw <= (1 << 20) && p->min_seed_len >= 1 &&
         p->min_seed_len <= 65535 && p->max_chain_gap >= 0 && std::isfinite(p->mask_level_redun) &&
         std::isfinite(p->mask_level) && p->mask_level_redun >= 0.f && p->mask_level >= 0.f && p->max_rounds >= 1 &&
         p->max_rounds <= kRescueHostMaxRounds;
}

inline bool sel_opt_ok(const bwagpu_selopt_t* s) {
  return s && std::isfinite(s->mask_level) && s->mask_level >= 0.f && std::isfinite(s->drop_ratio) &&
         std::isfinite(s->mapQ_coef_len) && s->min_seed_len >= 0 && s->min_seed_len <= 65535 && s->flags >= 0;
}

// the BWAGPU_POST_* flags of bwagpu_regs_post*, bwagpu_set_regs_post
inline int post_flags_check(int32_t flags, const char** why) {
  const int32_t all = BWAGPU_POST_DEDUP_PATCH | BWAGPU_POST_MARK_ALT | BWAGPU_POST_PRIMARY;
  if (flags < 0 || (flags & ~all)) return *why = "unknown flag", BWAGPU_E_INVAL;
  if (flags & BWAGPU_POST_PRIMARY) return *why = "BWAGPU_POST_PRIMARY is not implemented", BWAGPU_E_UNSUPPORTED;
  return BWAGPU_OK;
}

// the mem_opt_t flags of bwagpu_pair_select*
inline int sel_flags_check(int32_t flags, const char** why) {
  if (flags & (BWAGPU_MEM_F_ALL | BWAGPU_MEM_F_NO_MULTI | BWAGPU_MEM_F_PRIMARY5 | BWAGPU_MEM_F_KEEP_SUPP_MAPQ))
    return *why = "MEM_F_ALL, MEM_F_NO_MULTI, MEM_F_PRIMARY5 and MEM_F_KEEP_SUPP_MAPQ are not implemented",
           BWAGPU_E_UNSUPPORTED;
  return BWAGPU_OK;
}

// a live orientation's range must be ordered and bounded: the windows of its
// calls are high - low + the mate's length bases long
inline int pes_check(const bwagpu_pestat_t* pes, const char** why) {
  if (!pes) return *why = "NULL pes", BWAGPU_E_INVAL;
  for (int r = 0; r < 4; ++r) {
    if (pes[r].failed) continue;
    if (pes[r].high < pes[r].low) return *why = "pes: high < low", BWAGPU_E_INVAL;
    if ((int64_t)pes[r].high - pes[r].low > kRescueMaxRange)
      return *why = "pes: an insert-size range over 2^20", BWAGPU_E_UNSUPPORTED;
  }
  return BWAGPU_OK;
}

// the input spans of n_reads reads: counts, offsets, address range -> plan's
// [lo, hi) and n_regs; with `disjoint` (a pass that writes in place) the spans
// must not overlap either.  A read without regions never has its offset looked at.
inline int spans_check(int32_t n_reads, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                       bool disjoint, StagePlan* plan, const char** why) {
  int64_t lo = INT64_MAX, hi = 0, total = 0;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (n[r] < 0) return *why = "negative region count", BWAGPU_E_INVAL;
    if (n[r] == 0) continue;
    if (reg_off[r] < 0 || reg_off[r] > (INT64_MAX / (int64_t)sizeof(bwagpu_alnreg_t)) - n[r])
      return *why = "region span outside the address range", BWAGPU_E_INVAL;
    lo = std::min(lo, reg_off[r]);
    hi = std::max(hi, reg_off[r] + n[r]);
    total += n[r];
  }
  if (total && !regs) return *why = "NULL regs", BWAGPU_E_INVAL;
  plan->lo = total ? lo : 0;
  plan->hi = total ? hi : 0;
  plan->n_regs = total;
  if (!disjoint) return BWAGPU_OK;
  std::vector<int32_t> used;
  for (int32_t r = 0; r < n_reads; ++r)
    if (n[r]) used.push_back(r);
  std::sort(used.begin(), used.end(), [&](int32_t x, int32_t y) { return reg_off[x] < reg_off[y]; });
  for (size_t k = 1; k < used.size(); ++k)
    if (reg_off[used[k - 1]] + n[used[k - 1]] > reg_off[used[k]]) return *why = "region spans overlap", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// the reads' bases: seq_off starts at >= 0 and ascends, seq is there when any
// base is -> plan's [seq_lo, seq_hi).  *too_long (when asked for): some read is
// over BWAGPU_MAX_READ_LEN; the caller decides when that verdict is due.
inline int seq_check(int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, StagePlan* plan, bool* too_long,
                     const char** why) {
  if (seq_off[0] < 0) return *why = "negative seq_off", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (seq_off[r + 1] < seq_off[r]) return *why = "seq_off not ascending", BWAGPU_E_INVAL;
    if (too_long && seq_off[r + 1] - seq_off[r] > BWAGPU_MAX_READ_LEN) *too_long = true;
  }
  if (seq_off[n_reads] > seq_off[0] && !seq) return *why = "NULL seq", BWAGPU_E_INVAL;
  plan->seq_lo = seq_off[0];
  plan->seq_hi = seq_off[n_reads];
  return BWAGPU_OK;
}

// every region of every (checked) span lies inside its read
inline int qbqe_check(int32_t n_reads, const int64_t* seq_off, const int64_t* reg_off, const bwagpu_alnreg_t* regs,
                      const int32_t* n, const char** why) {
  for (int32_t r = 0; r < n_reads; ++r) {
    if (n[r] == 0) continue;
    const int64_t l_seq = seq_off[r + 1] - seq_off[r];
    const bwagpu_alnreg_t* a = regs + reg_off[r];
    for (int32_t k = 0; k < n[r]; ++k)
      if (a[k].qb < 0 || a[k].qe < a[k].qb || a[k].qe > l_seq)
        return *why = "a region's qb/qe lie outside its read", BWAGPU_E_INVAL;
  }
  return BWAGPU_OK;
}

// bwagpu_regs_post.  The plan is filled only when the call is accepted.
inline int post_check(const bwagpu_postopt_t* popt, int32_t flags, int32_t n_reads, const int64_t* seq_off,
                      const uint8_t* seq, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                      StagePlan* plan, const char** why) {
  *plan = StagePlan{};
  *why = "";
  if (!post_opt_ok(popt)) return *why = "bad bwagpu_postopt_t", BWAGPU_E_INVAL;
  if (int rc = post_flags_check(flags, why)) return rc;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!seq_off || !reg_off || !n) return *why = "NULL array", BWAGPU_E_INVAL;
  StagePlan p;
  bool too_long = false;
  if (int rc = seq_check(n_reads, seq_off, seq, &p, &too_long, why)) return rc;
  if (int rc = spans_check(n_reads, reg_off, regs, n, true, &p, why)) return rc;
  if (too_long) return *why = "read longer than BWAGPU_MAX_READ_LEN", BWAGPU_E_UNSUPPORTED;
  if (int rc = qbqe_check(n_reads, seq_off, reg_off, regs, n, why)) return rc;
  *plan = p;
  return BWAGPU_OK;
}

// bwagpu_pestat: an odd trailing read is ignored as mem_pestat's n >> 1 does
inline int pestat_check(const bwagpu_pairopt_t* po, int32_t n_reads, const int64_t* reg_off,
                        const bwagpu_alnreg_t* regs, const int32_t* n, const bwagpu_pestat_t* pes, StagePlan* plan,
                        const char** why) {
  *plan = StagePlan{};
  *why = "";
  if (!pair_opt_ok(po)) return *why = "bad bwagpu_pairopt_t", BWAGPU_E_INVAL;
  if (!pes) return *why = "NULL pes", BWAGPU_E_INVAL;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  const int32_t used = n_reads & ~1;
  if (used == 0) return BWAGPU_OK;
  if (!reg_off || !n) return *why = "NULL array", BWAGPU_E_INVAL;
  return spans_check(used, reg_off, regs, n, false, plan, why);
}

// bwagpu_mate_rescue
inline int rescue_check(const bwagpu_pairopt_t* po, const bwagpu_pestat_t* pes, int32_t n_reads,
                        const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off,
                        const bwagpu_alnreg_t* regs, const int32_t* n, const int64_t* out_off,
                        const bwagpu_alnreg_t* out_regs, const int32_t* out_n, const int32_t* status,
                        const int32_t* n_sw, StagePlan* plan, const char** why) {
  *plan = StagePlan{};
  *why = "";
  if (!pair_opt_ok(po)) return *why = "bad bwagpu_pairopt_t", BWAGPU_E_INVAL;
  if (int rc = pes_check(pes, why)) return rc;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads & 1) return *why = "odd read count: reads 2i and 2i+1 are a pair", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!seq_off || !reg_off || !n || !out_off || !out_n || !status || !n_sw) return *why = "NULL array", BWAGPU_E_INVAL;
  StagePlan p;
  if (int rc = seq_check(n_reads, seq_off, seq, &p, nullptr, why)) return rc;
  for (int64_t i = seq_off[0]; i < seq_off[n_reads]; ++i)
    if (seq[i] > 4) return *why = "base > 4", BWAGPU_E_INVAL;
  if (int rc = spans_check(n_reads, reg_off, regs, n, false, plan, why)) return rc;
  if (out_off[0] < 0 || out_off[n_reads] > INT64_MAX / (int64_t)sizeof(bwagpu_alnreg_t))
    return *why = "output span outside the address range", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (out_off[r + 1] < out_off[r]) return *why = "out_off not ascending", BWAGPU_E_INVAL;
    if (out_off[r + 1] - out_off[r] < n[r]) return *why = "an output span is smaller than its input", BWAGPU_E_INVAL;
  }
  if (out_off[n_reads] > out_off[0] && !out_regs) return *why = "NULL out_regs", BWAGPU_E_INVAL;
  if (int rc = qbqe_check(n_reads, seq_off, reg_off, regs, n, why)) return rc;
  plan->out_lo = out_off[0];
  plan->out_hi = out_off[n_reads];
  plan->seq_lo = p.seq_lo;
  plan->seq_hi = p.seq_hi;
  return BWAGPU_OK;
}

// bwagpu_mark_primary
inline int mark_check(const bwagpu_selopt_t* sopt, int32_t n_reads, const int64_t* reg_off,
                      const bwagpu_alnreg_t* regs, const int32_t* n, const int32_t* n_pri, const int32_t* status,
                      StagePlan* plan, const char** why) {
  *plan = StagePlan{};
  *why = "";
  if (!sel_opt_ok(sopt)) return *why = "bad bwagpu_selopt_t", BWAGPU_E_INVAL;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!reg_off || !n || !n_pri || !status) return *why = "NULL array", BWAGPU_E_INVAL;
  return spans_check(n_reads, reg_off, regs, n, true, plan, why);
}

// bwagpu_pair_select
inline int pairsel_check(const bwagpu_selopt_t* sopt, const bwagpu_pestat_t* pes, int32_t n_reads,
                         const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n, const int32_t* n_pri,
                         const bwagpu_pairsel_t* sel, const int32_t* out_mapq, int32_t n_seqs, StagePlan* plan,
                         const char** why) {
  *plan = StagePlan{};
  *why = "";
  if (!sel_opt_ok(sopt)) return *why = "bad bwagpu_selopt_t", BWAGPU_E_INVAL;
  if (int rc = sel_flags_check(sopt->flags, why)) return rc;
  if (int rc = pes_check(pes, why)) return rc;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads & 1) return *why = "odd read count: reads 2i and 2i+1 are a pair", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!reg_off || !n || !n_pri || !sel) return *why = "NULL array", BWAGPU_E_INVAL;
  if (int rc = spans_check(n_reads, reg_off, regs, n, true, plan, why)) return rc;
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
