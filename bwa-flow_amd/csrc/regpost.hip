// regpost.hip — MI355X (gfx950) post-processing of a batch's regions, the
// step bwa-flow's RegionsToSam::compute runs on host threads between
// mem_chain2aln and mem_reg2aln (src/Pipeline.cpp:560-575, 612):
//   mem_sort_dedup_patch (bwa/bwamem.c:446-498) with mem_patch_reg (415-444),
//   the is_alt flag (Pipeline.cpp:570-574).
// (mem_mark_primary_se, Pipeline.cpp:612, is not here yet: BWAGPU_POST_PRIMARY
// is refused by the C ABI.)
//
// One launch, no lists: a wave owns kPostReadsPerWave consecutive reads.
//  * Lane-parallel classification: lane l < kPostReadsPerWave loads its read's
//    count and span.  Reads with n <= 1 never enter mem_sort_dedup_patch's
//    body (bwamem.c:449); their lane sets the ALT bit itself.
//  * The reads with n >= 2 (a ballot) are taken one at a time by the whole
//    wave.  The walk is serial in the reference (it breaks early and mutates
//    qb/qe/rb that later iterations read), so every lane runs the same code on
//    the same data — wave-uniform, as chain.hip's per-read pass does: reads
//    broadcast, every lane stores the same value.  The records sit in LDS for
//    n <= kPostLdsRegs and are worked on in place in HBM otherwise.
//  * When a pair passes mem_patch_reg's gates the wave runs bwa_gen_cigar2's
//    score-only global DP there and then (global_dp.h: the wave DP of the CIGAR
//    step without its direction matrix): a successful patch rewrites p, which
//    the next iterations of the walk read.
//  * Sorts: klib's introsort step for step on the 88-byte records (ksort_dev.h),
//    so ties on re, the identical hits of alnreg_slt, and the unstable
//    partitions above 17 elements fall as in the reference.
// Float rules: mask_level_redun * (float)int64 is a float32 product compared
// against an integer converted to float; the patch's
// relative band and score ratio are double, the predicted scores are a double
// divide, multiply and add, each rounded on its own (no fused multiply-add).
#include <hip/hip_runtime.h>

#include "engine.h"
#include "global_dp.h"
#include "ksort_dev.h"
#include "regpost.h"
#include "regwalk.h"
#include "wave_ops.h"

namespace bwagpu {

namespace {

constexpr int kPostReadsPerWave = 8;
constexpr int kPostLdsRegs = 32;  // records per wave held in LDS
constexpr int kPostQCap = 1024;   // BWAGPU_MAX_READ_LEN + 1
constexpr int kPostWaveLds = kPostLdsRegs * (int)sizeof(R) + kPostQCap + kPostRefCap;

struct PostCtx {
  int64_t qoff;   // the read's first base in RegPostArgs::seq
  int lq;         // its length
  uint8_t *q, *r; // the wave's LDS: query slice, reference window
  int dps;        // patch DPs run
  int err;        // ERR_POST
};

// mem_patch_reg (bwamem.c:415-444); x = a (the earlier hit), y = b
__device__ int patch_reg(const DevOpt& o, const DevRef& ref, const RegPostArgs& g, const R* x, const R* y,
                         PostCtx& c, int* w_out) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t l_pac = ref.l_pac, two = l_pac << 1;
  const int64_t arb = uni64(x->rb), are = uni64(x->re), brb = uni64(y->rb), bre = uni64(y->re);
  const int aqb = uni(x->qb), aqe = uni(x->qe), bqb = uni(y->qb), bqe = uni(y->qe);
  if (arb < l_pac && brb >= l_pac) return 0;                // on different strands
  if (aqb >= bqb || aqe >= bqe || are >= bre) return 0;     // not colinear
  int w = (int)((are - brb) - (aqe - bqb));                 // required bandwidth
  w = w > 0 ? w : -w;
  double r = (double)(are - brb) / (double)(bre - arb) - (double)(aqe - bqb) / (double)(bqe - aqb);
  r = r > 0. ? r : -r;
  const float max_r = 0.05f;  // PATCH_MAX_R_BW; x 2 is a float product
  if (are < brb || aqe < bqb) {
    if (w > o.w << 1 || r >= (double)max_r) return 0;
  } else if (w > o.w << 2 || r >= (double)(max_r * 2)) {
    return 0;
  }
  w += uni(x->w) + uni(y->w);
  w = w < o.w << 2 ? w : o.w << 2;
  // bwa_gen_cigar2(..., w, l_pac, pac, b->qe - a->qb, query + a->qb, a->rb, b->re, &score, 0, 0), bwa.c:121-207
  const int lql = bqe - aqb;
  const int64_t rb = arb, re = bre, rl64 = re - rb;
  if (lql <= 0 || rb >= re || (rb < l_pac && re > l_pac)) return 0;  // bwa.c:132 (score is not written there)
  {
    const int64_t beg = rb < 0 ? 0 : rb, end = re > two ? two : re;  // bns_get_seq, bntseq.c:375-408
    if (!(beg >= l_pac || end <= l_pac) || end - beg != rl64) return 0;  // bwa.c:134
  }
  if (aqb < 0 || bqe > c.lq || lql >= kPostQCap || rl64 > kPostRefCap) {
    c.err |= ERR_POST;
    return 0;
  }
  const int rl = (int)rl64;
  const bool rev = rb >= l_pac;
  post_sync();
  for (int k = lane; k < lql; k += 64) c.q[k] = g.seq[c.qoff + aqb + (rev ? lql - 1 - k : k)];
  for (int k = lane; k < rl; k += 64) {
    const int64_t p = rev ? re - 1 - k : rb + k;
    const int64_t f = p >= l_pac ? two - 1 - p : p;
    const int b = (ref.pac[f >> 2] >> ((~f & 3) << 1)) & 3;
    c.r[k] = (uint8_t)(p >= l_pac ? 3 - b : b);
  }
  post_sync();
  int score;
  if (lql == rl && w == 0) {  // bwa.c:141-149
    int s = 0;
    for (int k = lane; k < lql; k += 64) s += o.mat[c.r[k] * 5 + c.q[k]];
    score = wave_sum(s);
  } else {  // bwa.c:151-167
    const int half = (lql + 1) >> 1;
    const int mi = (int)((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
    const int md = (int)((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
    const int mg = max(max(mi, md), 1);
    const int dl = lql > rl ? lql - rl : rl - lql;
    int wb = min((mg + dl + 1) >> 1, w);
    wb = max(wb, dl + 3);
    int64_t cells = 0;
    if (2 * wb + 1 <= 64)
      score = uni(band_dp<1, false>(o, lql, c.q, rl, c.r, wb, 0, nullptr, cells));
    else if (2 * wb + 1 <= 128)
      score = uni(band_dp<2, false>(o, lql, c.q, rl, c.r, wb, 0, nullptr, cells));
    else if (lql < 256)
      score = uni(global_dp<4, false>(o, lql, c.q, rl, c.r, wb, 0, nullptr, cells));
    else
      score = uni(global_dp<16, false>(o, lql, c.q, rl, c.r, wb, 0, nullptr, cells));
    c.dps += 1;
  }
  const int asc = uni(x->score), bsc = uni(y->score);
  // predicted scores from the query and from the reference: divide, multiply, add
  const double fq = (double)(bqe - aqb) / (double)((bqe - bqb) + (aqe - aqb));
  const double fr = (double)(bre - arb) / (double)((bre - brb) + (are - arb));
  const int q_s = (int)__dadd_rn(__dmul_rn(fq, (double)(bsc + asc)), .499);
  const int r_s = (int)__dadd_rn(__dmul_rn(fr, (double)(bsc + asc)), .499);
  const float min_ratio = 0.90f;  // PATCH_MIN_SC_RATIO
  if ((double)score / (double)(q_s > r_s ? q_s : r_s) < (double)min_ratio) return 0;
  *w_out = w;
  return score;
}

// mem_sort_dedup_patch's body for n >= 2 (regwalk.h) with mem_patch_reg
__device__ int sort_dedup_patch(const DevOpt& o, const DevRef& ref, const RegPostArgs& g, int n, R* a, PostCtx& c) {
  return sort_dedup_walk<true>(g.po.max_chain_gap, g.po.mask_level_redun, n, a,
                               [&](const R* x, const R* y, int* w) { return patch_reg(o, ref, g, x, y, c, w); });
}

__device__ __forceinline__ void set_alt(const DevRef& ref, const RegPostArgs& g, R* p) {
  const int rid = p->rid;
  if (rid >= 0 && rid < ref.n_seqs && g.alt[rid]) p->n_comp_is_alt = (p->n_comp_is_alt & kCompMask) | (1u << 30);
}

}  // namespace

__global__ void __launch_bounds__(256) regpost_kernel(DevOpt o, DevRef ref, RegPostArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int lane = (int)(threadIdx.x & 63);
  const int wib = uni((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * (int)(blockDim.x >> 6) + wib;
  const int base = wave * kPostReadsPerWave;
  if (base >= g.n_reads) return;
  uint8_t* const wl = lds + (size_t)wib * kPostWaveLds;
  R* const lregs = reinterpret_cast<R*>(wl);
  PostCtx c;
  c.q = wl + kPostLdsRegs * sizeof(R);
  c.r = c.q + kPostQCap;
  c.dps = 0;
  c.err = 0;
  // ---- classification: one lane per read
  const int rd = base + lane;
  const bool mine = lane < kPostReadsPerWave && rd < g.n_reads;
  int nr = mine ? g.n[rd] : 0;
  int64_t off = 0;
  if (mine && nr > 0) off = g.reg_off ? g.reg_off[rd] : (int64_t)g.cso[g.rco[rd]];
  if (mine && nr == 1) {  // mem_sort_dedup_patch returns at once (bwamem.c:449)
    R* p = g.regs + off;
    if ((g.flags & BWAGPU_POST_MARK_ALT) && g.alt) set_alt(ref, g, p);
  }
  uint64_t heavy = __builtin_amdgcn_ballot_w64(nr >= 2);
  // ---- reads with n >= 2: the whole wave, one read at a time
  while (heavy) {
    const int l = uni(__builtin_ctzll(heavy));
    heavy &= heavy - 1;
    const int n0 = __builtin_amdgcn_readlane(nr, l);
    const int64_t off0 = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(off >> 32), l) << 32 |
                                   (uint32_t)__builtin_amdgcn_readlane((int)off, l));
    const int rd0 = base + l;
    c.qoff = uni64(g.seq_off[rd0]);
    c.lq = (int)(uni64(g.seq_off[rd0 + 1]) - c.qoff);
    R* const gl = g.regs + off0;
    const bool in_lds = n0 <= kPostLdsRegs;
    R* const a = in_lds ? lregs : gl;
    constexpr int kW = (int)(sizeof(R) / 8);
    if (in_lds) {
      const uint2* src = reinterpret_cast<const uint2*>(gl);
      uint2* dst = reinterpret_cast<uint2*>(lregs);
      for (int w = lane; w < n0 * kW; w += 64) dst[w] = src[w];
    }
    post_sync();
    int m = n0;
    if (g.flags & BWAGPU_POST_DEDUP_PATCH) m = uni(sort_dedup_patch(o, ref, g, n0, a, c));
    post_sync();
    if ((g.flags & BWAGPU_POST_MARK_ALT) && g.alt)
      for (int i = lane; i < m; i += 64) set_alt(ref, g, a + i);
    post_sync();
    if (in_lds) {
      const uint2* src = reinterpret_cast<const uint2*>(lregs);
      uint2* dst = reinterpret_cast<uint2*>(gl);
      for (int w = lane; w < m * kW; w += 64) dst[w] = src[w];
    }
    if (lane == 0) g.n[rd0] = m;
    post_sync();
  }
  if (g.stats && lane == 0) {
    if (c.dps) atomicAdd((unsigned long long*)&g.stats[ST_CALLS], (unsigned long long)c.dps);
    if (c.err) atomicOr((unsigned long long*)&g.stats[ST_ERR], (unsigned long long)c.err);
  }
}

hipError_t launch_regpost(const DevOpt& o, const DevRef& ref, const RegPostArgs& a, hipStream_t st) {
  if (a.n_reads <= 0) return hipSuccess;
  constexpr int kWpb = 4;
  const int per_block = kWpb * kPostReadsPerWave;
  const unsigned blocks = (unsigned)((a.n_reads + per_block - 1) / per_block);
  hipLaunchKernelGGL(regpost_kernel, dim3(blocks), dim3(64 * kWpb), (size_t)kWpb * kPostWaveLds, st, o, ref, a);
  return hipGetLastError();
}

}  // namespace bwagpu
