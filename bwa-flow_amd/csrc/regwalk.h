// regwalk.h — mem_sort_dedup_patch's body for n >= 2 (bwa/bwamem.c:450-497) on
// the device, one implementation for its two callers: the region
// post-processing (regpost.hip: with mem_patch_reg) and mate rescue
// (rescue.hip: mem_matesw calls mem_sort_dedup_patch(opt, 0, 0, 0, ...), where
// mem_patch_reg returns 0 at bwamem.c:419, so the walk never merges).
// Wave-uniform: every lane runs the same code on the same records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"
#include "global_dp.h"
#include "ksort_dev.h"

namespace bwagpu {

using R = bwagpu_alnreg_t;
static_assert(sizeof(R) == 88, "mem_alnreg_t layout");
constexpr uint32_t kCompMask = 0x3fffffffu;

__device__ __forceinline__ int alt_of(const R& x) { return (int)x.n_comp_is_alt >> 30; }  // int is_alt:2

struct LtRe {  // alnreg_slt2, bwamem.c:400
  __device__ bool operator()(const R& x, const R& y) const { return x.re < y.re; }
};
struct LtScore {  // alnreg_slt, bwamem.c:403
  __device__ bool operator()(const R& x, const R& y) const {
    return x.score > y.score || (x.score == y.score && (x.rb < y.rb || (x.rb == y.rb && x.qb < y.qb)));
  }
};
// The records are reached through a generic pointer (flat accesses, LDS or HBM)
// and copied with ds accesses; the two kinds reach LDS by different paths, so a
// phase change waits for every outstanding access of both.
__device__ __forceinline__ void post_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// kPatch: patch(q, p, &w) is mem_patch_reg(q, p) -> score (0: no merge);
// !kPatch: the branch is compiled out (the "no patch" form)
template <bool kPatch, class Patch>
__device__ int sort_dedup_walk(int gap, float red, int n, R* a, Patch patch) {
  c_introsort(n, a, LtRe{});  // by the END position
  for (int i = 0; i < n; ++i) a[i].n_comp_is_alt = (a[i].n_comp_is_alt & ~kCompMask) | 1u;
  for (int i = 1; i < n; ++i) {
    R* p = a + i;
    if (uni(p->rid) != uni(a[i - 1].rid) || uni64(p->rb) >= uni64(a[i - 1].re) + gap) continue;
    for (int j = i - 1; j >= 0; --j) {
      R* q = a + j;
      const int64_t prb = uni64(p->rb), qre = uni64(q->re);
      if (!(uni(p->rid) == uni(q->rid) && prb < qre + gap)) break;
      const int qqb = uni(q->qb), qqe = uni(q->qe);
      if (qqe == qqb) continue;  // a[j] has been excluded
      const int pqb = uni(p->qb), pqe = uni(p->qe);
      const int64_t pre = uni64(p->re), qrb = uni64(q->rb);
      const int64_t orr = qre - prb;
      const int64_t oq = qqb < pqb ? qqe - pqb : pqe - qqb;
      const int64_t mr = qre - qrb < pre - prb ? qre - qrb : pre - prb;
      const int64_t mq = qqe - qqb < pqe - pqb ? qqe - qqb : pqe - pqb;
      if ((float)orr > red * (float)mr && (float)oq > red * (float)mq) {  // one of the hits is redundant
        if (uni(p->score) < uni(q->score)) {
          p->qe = pqb;
          break;
        } else {
          q->qe = qqb;
        }
      } else if constexpr (kPatch) {
        int score, w = 0;
        if (qrb < prb && (score = patch(q, p, &w)) > 0) {  // merge q into p
          const uint32_t pc = p->n_comp_is_alt, qc = q->n_comp_is_alt;
          p->n_comp_is_alt = (pc & ~kCompMask) | (((pc & kCompMask) + (qc & kCompMask) + 1u) & kCompMask);
          p->seedcov = max(p->seedcov, q->seedcov);
          p->sub = max(p->sub, q->sub);
          p->csub = max(p->csub, q->csub);
          p->qb = qqb;
          p->rb = qrb;
          p->truesc = p->score = score;
          p->w = w;
          q->qb = qqe;
        }
      }
    }
  }
  int m = 0;
  for (int i = 0; i < n; ++i)  // exclude the marked hits
    if (uni(a[i].qe) > uni(a[i].qb)) {
      if (m != i) a[m] = a[i];
      ++m;
    }
  n = m;
  if (n == 0) return 0;
  c_introsort(n, a, LtScore{});
  for (int i = 1; i < n; ++i)  // mark identical hits
    if (a[i].score == a[i - 1].score && a[i].rb == a[i - 1].rb && a[i].qb == a[i - 1].qb) a[i].qe = a[i].qb;
  m = 1;
  for (int i = 1; i < n; ++i)
    if (uni(a[i].qe) > uni(a[i].qb)) {
      if (m != i) a[m] = a[i];
      ++m;
    }
  return m;
}

}  // namespace bwagpu
