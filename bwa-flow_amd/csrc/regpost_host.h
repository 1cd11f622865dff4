// regpost_host.h — host-side argument validation and span arithmetic of
// bwagpu_regs_post (capi.hip).  Plain C++: compiles without HIP, so that the
// checks run under the host sanitizers (tests/cpp/post_host_asan.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bwagpu.h"

namespace bwagpu {

// What a validated call moves: regs[lo, hi) holds every read's span, the reads'
// bases are seq[seq_lo, seq_hi).
struct PostPlan {
  int64_t lo = 0, hi = 0;
  int64_t seq_lo = 0, seq_hi = 0;
  int64_t n_regs = 0;  // sum of n
};

inline bool post_opt_ok(const bwagpu_postopt_t* p) {
  return p && p->max_chain_gap >= 0 && std::isfinite(p->mask_level_redun) && std::isfinite(p->mask_level) &&
         p->mask_level_redun >= 0.f && p->mask_level >= 0.f;
}

// BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED with *why set.  Nothing
// is read beyond seq_off[n_reads], reg_off[n_reads - 1], n[n_reads - 1] and the
// spans those describe.
inline int post_check(const bwagpu_postopt_t* popt, int32_t flags, int32_t n_reads, const int64_t* seq_off,
                      const uint8_t* seq, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                      PostPlan* plan, const char** why) {
  const int32_t all = BWAGPU_POST_DEDUP_PATCH | BWAGPU_POST_MARK_ALT | BWAGPU_POST_PRIMARY;
  *plan = PostPlan{};
  *why = "";
  if (!post_opt_ok(popt)) return *why = "bad bwagpu_postopt_t", BWAGPU_E_INVAL;
  if (flags < 0 || (flags & ~all)) return *why = "unknown flag", BWAGPU_E_INVAL;
  if (flags & BWAGPU_POST_PRIMARY) return *why = "BWAGPU_POST_PRIMARY is not implemented", BWAGPU_E_UNSUPPORTED;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  if (!seq_off || !reg_off || !n) return *why = "NULL array", BWAGPU_E_INVAL;
  if (seq_off[0] < 0) return *why = "negative seq_off", BWAGPU_E_INVAL;
  bool too_long = false;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (seq_off[r + 1] < seq_off[r]) return *why = "seq_off not ascending", BWAGPU_E_INVAL;
    if (seq_off[r + 1] - seq_off[r] > BWAGPU_MAX_READ_LEN) too_long = true;
  }
  if (seq_off[n_reads] > seq_off[0] && !seq) return *why = "NULL seq", BWAGPU_E_INVAL;
  // spans: non-negative, inside int64 arithmetic, pairwise disjoint
  std::vector<int32_t> used;
  int64_t lo = INT64_MAX, hi = 0, total = 0;
  for (int32_t r = 0; r < n_reads; ++r) {
    if (n[r] < 0) return *why = "negative region count", BWAGPU_E_INVAL;
    if (n[r] == 0) continue;
    if (reg_off[r] < 0 || reg_off[r] > (INT64_MAX / (int64_t)sizeof(bwagpu_alnreg_t)) - n[r])
      return *why = "region span outside the address range", BWAGPU_E_INVAL;
    used.push_back(r);
    lo = std::min(lo, reg_off[r]);
    hi = std::max(hi, reg_off[r] + n[r]);
    total += n[r];
  }
  if (!used.empty() && !regs) return *why = "NULL regs", BWAGPU_E_INVAL;
  std::sort(used.begin(), used.end(), [&](int32_t x, int32_t y) { return reg_off[x] < reg_off[y]; });
  for (size_t k = 1; k < used.size(); ++k)
    if (reg_off[used[k - 1]] + n[used[k - 1]] > reg_off[used[k]]) return *why = "region spans overlap", BWAGPU_E_INVAL;
  if (too_long) return *why = "read longer than BWAGPU_MAX_READ_LEN", BWAGPU_E_UNSUPPORTED;
  for (int32_t r : used) {
    const int64_t l_seq = seq_off[r + 1] - seq_off[r];
    const bwagpu_alnreg_t* a = regs + reg_off[r];
    for (int32_t k = 0; k < n[r]; ++k)
      if (a[k].qb < 0 || a[k].qe < a[k].qb || a[k].qe > l_seq)
        return *why = "a region's qb/qe lie outside its read", BWAGPU_E_INVAL;
  }
  plan->lo = used.empty() ? 0 : lo;
  plan->hi = used.empty() ? 0 : hi;
  plan->seq_lo = seq_off[0];
  plan->seq_hi = seq_off[n_reads];
  plan->n_regs = total;
  return BWAGPU_OK;
}

}  // namespace bwagpu
