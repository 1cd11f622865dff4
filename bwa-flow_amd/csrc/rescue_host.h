// rescue_host.h — host-side argument validation and span arithmetic of
// bwagpu_pestat and bwagpu_mate_rescue (capi.hip).  Plain C++: compiles without
// HIP, so that the checks run under the host sanitizers
// (tests/cpp/rescue_host_asan.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "bwagpu.h"

namespace bwagpu {

constexpr int kRescueHostMaxRounds = 8;          // == kRescueMaxRounds (rescue.h)
constexpr int64_t kRescueMaxRange = 1 << 20;     // pes[r].high - pes[r].low of a live orientation

// What a validated call moves: regs[lo, hi) holds every read's input span,
// out_regs[out_lo, out_hi) every output span, the bases are seq[seq_lo, seq_hi).
struct RescuePlan {
  int64_t lo = 0, hi = 0;
  int64_t out_lo = 0, out_hi = 0;
  int64_t seq_lo = 0, seq_hi = 0;
  int64_t n_regs = 0;
};

inline bool pair_opt_ok(const bwagpu_pairopt_t* p) {
  return p && p->max_ins >= 0 && p->max_matesw >= 0 && p->max_matesw <= (1 << 20) && p->min_seed_len >= 1 &&
         p->min_seed_len <= 65535 && p->max_chain_gap >= 0 && std::isfinite(p->mask_level_redun) &&
         std::isfinite(p->mask_level) && p->mask_level_redun >= 0.f && p->mask_level >= 0.f && p->max_rounds >= 1 &&
         p->max_rounds <= kRescueHostMaxRounds;
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

// the input spans of n_reads reads: counts, offsets, address range; -> [lo, hi) and the region total.
// Nothing is read beyond reg_off[n_reads - 1] and n[n_reads - 1].
inline int spans_check(int32_t n_reads, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                       int64_t* plo, int64_t* phi, int64_t* ptotal, const char** why) {
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
  *plo = total ? lo : 0;
  *phi = total ? hi : 0;
  *ptotal = total;
  return BWAGPU_OK;
}

// bwagpu_pestat: an odd trailing read is ignored as mem_pestat's n >> 1 does
inline int pestat_check(const bwagpu_pairopt_t* po, int32_t n_reads, const int64_t* reg_off,
                        const bwagpu_alnreg_t* regs, const int32_t* n, const bwagpu_pestat_t* pes, RescuePlan* plan,
                        const char** why) {
  *plan = RescuePlan{};
  *why = "";
  if (!pair_opt_ok(po)) return *why = "bad bwagpu_pairopt_t", BWAGPU_E_INVAL;
  if (!pes) return *why = "NULL pes", BWAGPU_E_INVAL;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  const int32_t used = n_reads & ~1;
  if (used == 0) return BWAGPU_OK;
  if (!reg_off || !n) return *why = "NULL array", BWAGPU_E_INVAL;
  return spans_check(used, reg_off, regs, n, &plan->lo, &plan->hi, &plan->n_regs, why);
}

// bwagpu_mate_rescue.  BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED with *why set.
inline int rescue_check(const bwagpu_pairopt_t* po, const bwagpu_pestat_t* pes, int32_t n_reads,
                        const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off,
                        const bwagpu_alnreg_t* regs, const int32_t* n, const int64_t* out_off,
                        const bwagpu_alnreg_t* out_regs, const int32_t* out_n, const int32_t* status,
                        const int32_t* n_sw, RescuePlan* plan, const char** why) {
  *plan = RescuePlan{};
  *why = "";
  if (!pair_opt_ok(po)) return *why = "bad bwagpu_pairopt_t", BWAGPU_E_INVAL;
  if (int rc = pes_check(pes, why)) return rc;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads & 1) return *why = "odd read count: reads 2i and 2i+1 are a pair", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!seq_off || !reg_off || !n || !out_off || !out_n || !status || !n_sw) return *why = "NULL array", BWAGPU_E_INVAL;
  if (seq_off[0] < 0) return *why = "negative seq_off", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r)
    if (seq_off[r + 1] < seq_off[r]) return *why = "seq_off not ascending", BWAGPU_E_INVAL;
  if (seq_off[n_reads] > seq_off[0] && !seq) return *why = "NULL seq", BWAGPU_E_INVAL;
  for (int64_t i = seq_off[0]; i < seq_off[n_reads]; ++i)
    if (seq[i] > 4) return *why = "base > 4", BWAGPU_E_INVAL;
  if (int rc = spans_check(n_reads, reg_off, regs, n, &plan->lo, &plan->hi, &plan->n_regs, why)) return rc;
  if (out_off[0] < 0 || out_off[n_reads] > INT64_MAX / (int64_t)sizeof(bwagpu_alnreg_t))
    return *why = "output span outside the address range", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (out_off[r + 1] < out_off[r]) return *why = "out_off not ascending", BWAGPU_E_INVAL;
    if (out_off[r + 1] - out_off[r] < n[r]) return *why = "an output span is smaller than its input", BWAGPU_E_INVAL;
  }
  if (out_off[n_reads] > out_off[0] && !out_regs) return *why = "NULL out_regs", BWAGPU_E_INVAL;
  for (int32_t r = 0; r < n_reads; ++r) {
    const int64_t l_seq = seq_off[r + 1] - seq_off[r];
    const bwagpu_alnreg_t* a = regs + reg_off[r];
    for (int32_t k = 0; k < n[r]; ++k)
      if (a[k].qb < 0 || a[k].qe < a[k].qb || a[k].qe > l_seq)
        return *why = "a region's qb/qe lie outside its read", BWAGPU_E_INVAL;
  }
  plan->out_lo = out_off[0];
  plan->out_hi = out_off[n_reads];
  plan->seq_lo = seq_off[0];
  plan->seq_hi = seq_off[n_reads];
  return BWAGPU_OK;
}

}  // namespace bwagpu
