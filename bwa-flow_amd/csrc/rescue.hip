// rescue.hip — MI355X (gfx950) insert-size statistics and mate rescue of a
// batch of read pairs: mem_pestat (bwa/bwamem_pair.c:49-112) and the rescue loop
// at the top of mem_sam_pe (bwamem_pair.c:268-279) with mem_matesw (:114-183).
// Reads 2i and 2i+1 are the two ends of pair i.
//
// mem_pestat: a lane per pair appends its insert size to one of four lists
// (atomic counter), a block per orientation sorts its list (bitonic, the keys
// are plain uint64 so any correct sort gives the reference's array) and one
// lane finishes the statistics in the reference's order of operations: the sum
// of squares is one dependent chain of separately rounded multiplies and adds
// over the sorted values, as the x86-64 build of the reference has no FMA.
//
// Mate rescue, speculate and replay.  A call's windows depend
// only on the candidate (a snapshot of the input regions) and pes; only whether
// the call is made depends on the regions rescued before it.  So
//   plan   per pair, every candidate's unskipped orientations (skip test on
//          the input regions) become ksw_align2 tasks: window fetched from the
//          resident pac, mate taken from a pool holding both strands;
//   align2 the batched ksw_align2 (align2.hip) on the list;
//   apply  a wave per pair replays bwamem_pair.c:271-277 on a copy of the input
//          in the output span with the results from a table (pair, read,
//          candidate, orientation) -> task.  Results of calls the rescued
//          regions made unnecessary are ignored.  A call that is needed and was
//          not computed stops the replay: the pair's remaining calls are marked
//          wanted in every live orientation, the next round's plan emits them
//          and the replay starts over from the input.
// No kernel waits on another wave; every loop is bounded by counts loaded
// before it starts.  The replay is wave-uniform as regpost.hip's walk is: every
// lane runs the same code on the same records in HBM.
#include <hip/hip_runtime.h>

#include "engine.h"
#include "regwalk.h"
#include "rescue.h"

// mem_pestat's doubles are compared with the reference's bit for bit, and its
// build (x86-64, -O2) has no fused multiply-add.  hipcc contracts a * b + c by
// default, and __dmul_rn / __dadd_rn do not stop it: without
// OCML_BASIC_ROUNDED_OPERATIONS they are inline `x * y` and `x + y` that carry
// the `contract` flag of the header they come from.  So this file is compiled
// without contraction and the statistics use plain operators.
#pragma clang fp contract(off)

namespace bwagpu {

namespace {

constexpr int kWpb = 4;  // waves per block of the wave-per-pair kernels

// mem_infer_dir (bwamem_pair.c:26-33)
__device__ __forceinline__ int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t* dist) {
  const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
  const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;  // read 2 on the strand of read 1
  *dist = p2 > b1 ? p2 - b1 : b1 - p2;
  return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// bns_pos2rid (bntseq.c:346-361) of a forward position
__device__ int pos2rid(const DevRef& ref, int64_t pos_f) {
  if (pos_f >= ref.l_pac) return -1;
  int left = 0, mid = 0, right = ref.n_seqs;
  while (left < right) {
    mid = (left + right) >> 1;
    if (pos_f >= ref.ann_offset[mid]) {
      if (mid == ref.n_seqs - 1) break;
      if (pos_f < ref.ann_offset[mid + 1]) break;
      left = mid + 1;
    } else {
      right = mid;
    }
  }
  return mid;
}

// ---------------------------------------------------------------- mem_pestat
// cal_sub (bwamem_pair.c:35-47): the overlap test compares an int with an
// int * float product
__device__ int cal_sub(const DevOpt& o, const bwagpu_pairopt_t& po, const R* a, int n) {
  const int qb0 = a[0].qb, qe0 = a[0].qe;
  int j;
  for (j = 1; j < n; ++j) {
    const int qb = a[j].qb, qe = a[j].qe;
    const int b_max = qb > qb0 ? qb : qb0, e_min = qe < qe0 ? qe : qe0;
    if (e_min > b_max) {
      const int min_l = qe - qb < qe0 - qb0 ? qe - qb : qe0 - qb0;
      if ((float)(e_min - b_max) >= (float)min_l * po.mask_level) break;
    }
  }
  return j < n ? a[j].score : po.min_seed_len * o.a;
}

__global__ void __launch_bounds__(256) pestat_collect_kernel(DevOpt o, DevRef ref, PestatArgs g) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= g.n_pairs) return;
  const int n0 = g.n[2 * p], n1 = g.n[2 * p + 1];
  if (n0 <= 0 || n1 <= 0) return;
  const R* a0 = g.regs + g.reg_off[2 * p];
  const R* a1 = g.regs + g.reg_off[2 * p + 1];
  const double min_ratio = 0.8;  // MIN_RATIO
  if (cal_sub(o, g.po, a0, n0) > min_ratio * a0[0].score) return;
  if (cal_sub(o, g.po, a1, n1) > min_ratio * a1[0].score) return;
  if (a0[0].rid != a1[0].rid) return;
  int64_t is;
  const int dir = infer_dir(ref.l_pac, a0[0].rb, a1[0].rb, &is);
  if (is && is <= g.po.max_ins) {
    const int k = atomicAdd(&g.cnt[dir], 1);
    if (k < g.cap) g.isize[(size_t)dir * g.cap + k] = (uint64_t)is;
  }
}

__global__ void __launch_bounds__(256) pestat_finish_kernel(PestatArgs g) {
  const int d = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int n = min(g.cnt[d], g.cap);
  uint64_t* q = g.isize + (size_t)d * g.cap;
  bwagpu_pestat_t* r = g.pes + d;
  if (n < 10) {  // MIN_DIR_CNT
    if (tid == 0) *r = bwagpu_pestat_t{0, 0, 1, 0, 0., 0.};
    return;
  }
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += 256) q[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t u = q[i], v = q[x];
          if ((i & k) == 0 ? u > v : u < v) {
            q[i] = v;
            q[x] = u;
          }
        }
      }
      __syncthreads();
    }
  if (tid != 0) return;
  // plain operators under `fp contract(off)` (top of this file): one rounding per operation
  const int p25 = (int)q[(int)(.25 * n + .499)];
  const int p75 = (int)q[(int)(.75 * n + .499)];
  int low = (int)(p25 - 2.0 * (p75 - p25) + .499);  // OUTLIER_BOUND
  if (low < 1) low = 1;
  int high = (int)(p75 + 2.0 * (p75 - p25) + .499);
  const uint64_t lo = (uint64_t)(int64_t)low, hi = (uint64_t)(int64_t)high;
  double avg = 0.;
  int x = 0;
  for (int i = 0; i < n; ++i)
    if (q[i] >= lo && q[i] <= hi) avg += (double)q[i], ++x;
  avg /= x;
  double sd = 0.;
  for (int i = 0; i < n; ++i)  // ascending, each square and each add rounded on its own
    if (q[i] >= lo && q[i] <= hi) {
      const double t = (double)q[i] - avg;
      const double t2 = t * t;
      sd = sd + t2;
    }
  sd = __builtin_sqrt(sd / x);  // correctly rounded (the f64 square root's expansion)
  low = (int)(p25 - 3.0 * (p75 - p25) + .499);  // MAPPING_BOUND
  high = (int)(p75 + 3.0 * (p75 - p25) + .499);
  const double dlo = avg - 4.0 * sd, dhi = avg + 4.0 * sd;  // MAX_STDDEV
  if (low > dlo) low = (int)(dlo + .499);
  if (high < dhi) high = (int)(dhi + .499);
  if (low < 1) low = 1;
  *r = bwagpu_pestat_t{low, high, 0, 0, avg, sd};
}

__global__ void pestat_ratio_kernel(PestatArgs g) {  // MIN_DIR_RATIO, bwamem_pair.c:105-111
  if (threadIdx.x != 0) return;
  int mx = 0;
  for (int d = 0; d < 4; ++d) mx = max(mx, g.cnt[d]);
  for (int d = 0; d < 4; ++d)
    if (g.pes[d].failed == 0 && g.cnt[d] < mx * 0.05) g.pes[d].failed = 1;
}

// ---------------------------------------------------------------- mate rescue
struct Pes4 {
  int low[4], high[4], failed[4];
};
__device__ __forceinline__ Pes4 load_pes(const bwagpu_pestat_t* pes) {
  Pes4 s;
  for (int r = 0; r < 4; ++r) {
    s.low[r] = uni(pes[r].low);
    s.high[r] = uni(pes[r].high);
    s.failed[r] = uni(pes[r].failed) ? 1 : 0;
  }
  return s;
}

// the window of orientation r around candidate (arb, arid) for a mate of l_ms
// bases (bwamem_pair.c:133-150): the clamps, bns_fetch_seq's contig clip around
// (rb + re) >> 1 and the gate a->rid == rid && re - rb >= min_seed_len
__device__ bool rescue_window(const DevRef& ref, const Pes4& pes, int min_seed_len, int64_t arb, int arid, int l_ms,
                              int r, int64_t* prb, int64_t* pre) {
  const int64_t l_pac = ref.l_pac, two = l_pac << 1;
  const bool is_rev = (r >> 1) != (r & 1), is_larger = !(r >> 1);
  int64_t rb, re;
  if (!is_rev) {
    rb = is_larger ? arb + pes.low[r] : arb - pes.high[r];
    re = (is_larger ? arb + pes.high[r] : arb - pes.low[r]) + l_ms;
  } else {
    rb = (is_larger ? arb + pes.low[r] : arb - pes.high[r]) - l_ms;
    re = is_larger ? arb + pes.high[r] : arb - pes.low[r];
  }
  if (rb < 0) rb = 0;
  if (re > two) re = two;
  if (!(rb < re)) return false;
  const int64_t mid = (rb + re) >> 1;
  const bool rev = mid >= l_pac;
  const int rid = pos2rid(ref, rev ? two - 1 - mid : mid);
  if (rid < 0) return false;
  int64_t fb = ref.ann_offset[rid], fe = fb + ref.ann_len[rid];
  if (rev) {
    const int64_t x = fb;
    fb = two - fe;
    fe = two - x;
  }
  rb = rb > fb ? rb : fb;
  re = re < fe ? re : fe;
  *prb = rb;
  *pre = re;
  return arid == rid && re - rb >= min_seed_len;
}

// skip[] of one mem_matesw call against the regions ma[0, mn) (bwamem_pair.c:119-127);
// -> the number of set entries
__device__ int skip_test(int64_t l_pac, const Pes4& pes, int64_t arb, const R* ma, int mn, int* skip) {
  for (int r = 0; r < 4; ++r) skip[r] = pes.failed[r];
  for (int x = 0; x < mn; ++x) {
    int64_t dist;
    const int r = infer_dir(l_pac, arb, uni64(ma[x].rb), &dist);
    if (dist >= pes.low[r] && dist <= pes.high[r]) skip[r] = 1;
  }
  return skip[0] + skip[1] + skip[2] + skip[3];
}

__global__ void __launch_bounds__(256) rescue_pool_kernel(RescueArgs g) {
  const int rd = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = (int)(threadIdx.x & 63);
  if (rd >= 2 * g.n_pairs) return;
  const int64_t s0 = g.seq_off[rd];
  const int l = (int)(g.seq_off[rd + 1] - s0);
  for (int i = lane; i < l; i += 64) {
    const uint8_t c = g.seq[s0 + i];
    g.qpool[s0 + i] = c;
    g.qpool[g.rc_base + s0 + (l - 1 - i)] = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4;
  }
}

__global__ void __launch_bounds__(256) rescue_init_kernel(DevOpt o, RescueArgs g) {
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= g.n_pairs) return;
  int nb[2];
  bool unsup = false;
  for (int i = 0; i < 2; ++i) {
    const int rd = 2 * p + i, n = g.n[rd];
    const int64_t l = g.seq_off[rd + 1] - g.seq_off[rd];
    // align2's limits: the query length, and 16-bit scores that cannot saturate
    if (l > BWAGPU_MAX_READ_LEN || (l * o.a >= 250 && l * o.max_mat > 32767)) unsup = true;
    int k = 0;
    if (n > 0) {
      const R* a = g.regs + g.reg_off[rd];
      const int thr = a[0].score - g.po.pen_unpaired;
      for (int j = 0; j < n && k < g.po.max_matesw; ++j) k += a[j].score >= thr;
    }
    nb[i] = k;
  }
  if (unsup) nb[0] = nb[1] = 0;
  g.nb0[p] = nb[0];
  g.nslot[p] = 4 * (nb[0] + nb[1]);
  g.pstate[p] = unsup ? RP_DONE : RP_PENDING;
  g.status[p] = unsup ? BWAGPU_RESCUE_UNSUPPORTED : BWAGPU_RESCUE_DONE;
  g.n_sw[p] = unsup ? -1 : 0;
}

template <bool kEmit>
__global__ void __launch_bounds__(64 * kWpb) rescue_plan_kernel(DevOpt o, DevRef ref, RescueArgs g) {
  const int lane = (int)(threadIdx.x & 63);
  const int p = uni((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (p >= g.n_pairs) return;
  if (uni(g.pstate[p]) != RP_PENDING) {
    if (!kEmit && lane == 0) g.ntask[p] = 0, g.tbytes[p] = 0;
    return;
  }
  const Pes4 pes = load_pes(g.pes);
  const int64_t l_pac = ref.l_pac, two = l_pac << 1;
  const int64_t slot0 = uni64(g.slot_off[p]);
  const int nb0 = uni(g.nb0[p]);
  const int64_t t0 = kEmit ? uni64(g.task_off[p]) : 0, b0 = kEmit ? uni64(g.tb_off[p]) : 0;
  int nt = 0;
  int64_t nbytes = 0;
  for (int i = 0; i < 2; ++i) {
    const int rd = 2 * p + i, mate = 2 * p + (1 - i);
    const int nin = uni(g.n[rd]), mn = uni(g.n[mate]);
    if (nin <= 0) continue;
    const R* a = g.regs + uni64(g.reg_off[rd]);
    const R* ma = mn > 0 ? g.regs + uni64(g.reg_off[mate]) : nullptr;
    const int64_t ms0 = uni64(g.seq_off[mate]);
    const int l_ms = (int)(uni64(g.seq_off[mate + 1]) - ms0);
    const int thr = uni(a[0].score) - g.po.pen_unpaired;
    const int kmax = i ? (int)(uni(g.nslot[p]) / 4) - nb0 : nb0;
    int k = 0;
    for (int j = 0; j < nin && k < kmax; ++j) {
      if (uni(a[j].score) < thr) continue;
      const int64_t sbase = slot0 + (int64_t)((i ? nb0 : 0) + k) * 4;
      ++k;
      const int64_t arb = uni64(a[j].rb);
      const int arid = uni(a[j].rid);
      int want[4];
      if (g.round == 0) {  // the skip test on the input regions
        int skip[4];
        const int ns = skip_test(l_pac, pes, arb, ma, mn > 0 ? mn : 0, skip);
        for (int r = 0; r < 4; ++r) want[r] = ns < 4 && !skip[r];
      } else {
        for (int r = 0; r < 4; ++r) want[r] = uni(g.tab[sbase + r]) == RS_WANTED;
      }
      for (int r = 0; r < 4; ++r) {
        int64_t rb, re;
        if (!want[r] || !rescue_window(ref, pes, g.po.min_seed_len, arb, arid, l_ms, r, &rb, &re)) continue;
        const int len = (int)(re - rb);
        if (kEmit) {
          const int64_t t = t0 + nt, off = b0 + nbytes;
          uint8_t* dst = g.tpool + off;
          for (int x = lane; x < len; x += 64) {  // bns_get_seq (bntseq.c:375-408)
            const int64_t pos = rb + x;
            const int64_t f = pos >= l_pac ? two - 1 - pos : pos;
            const int b = (ref.pac[f >> 2] >> ((~f & 3) << 1)) & 3;
            dst[x] = (uint8_t)(pos >= l_pac ? 3 - b : b);
          }
          if (lane == 0) {
            const bool is_rev = (r >> 1) != (r & 1);
            const bool dropped = g.drop > 0 && (int)(t % g.drop) == g.drop - 1;
            bwagpu_align2_task_t task;
            task.qoff = (is_rev ? g.rc_base : 0) + ms0;
            task.toff = off;
            task.qlen = l_ms;
            task.tlen = len;
            task.xtra = BWAGPU_KSW_XSUBO | BWAGPU_KSW_XSTART | (l_ms * o.a < 250 ? BWAGPU_KSW_XBYTE : 0) |
                        (g.po.min_seed_len * o.a);
            task.pad_ = 0;
            g.tasks[t] = task;
            g.tab[sbase + r] = dropped ? RS_NONE : (int32_t)((g.round << kRescueIdxBits) | (int32_t)t);
          }
        }
        ++nt;
        nbytes += len;
      }
    }
  }
  if (!kEmit && lane == 0) g.ntask[p] = nt, g.tbytes[p] = (int32_t)nbytes;
}

// copy read rd's input regions into its output span (lanes stride over 8-byte words)
__device__ __forceinline__ void copy_in(const RescueArgs& g, int rd, int n, int lane) {
  constexpr int kW = (int)(sizeof(R) / 8);
  if (n <= 0) return;
  const uint2* src = reinterpret_cast<const uint2*>(g.regs + uni64(g.reg_off[rd]));
  uint2* dst = reinterpret_cast<uint2*>(g.out_regs + uni64(g.out_off[rd]));
  for (int w = lane; w < n * kW; w += 64) dst[w] = src[w];
}

__global__ void __launch_bounds__(64 * kWpb) rescue_apply_kernel(DevOpt o, DevRef ref, RescueArgs g) {
  const int lane = (int)(threadIdx.x & 63);
  const int p = uni((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (p >= g.n_pairs) return;
  const int st = uni(g.pstate[p]);
  if (g.round > 0 && st != RP_PENDING) return;
  int nin[2], cap[2], cnt[2];
  for (int i = 0; i < 2; ++i) {
    const int rd = 2 * p + i;
    nin[i] = max(uni(g.n[rd]), 0);
    const int64_t c = uni64(g.out_off[rd + 1]) - uni64(g.out_off[rd]);
    cap[i] = (int)(c < 0 ? 0 : c > INT32_MAX ? INT32_MAX : c);
  }
  if (nin[0] > cap[0] || nin[1] > cap[1]) {  // not even the copy fits
    if (lane == 0) {
      g.out_n[2 * p] = g.out_n[2 * p + 1] = 0;
      g.status[p] = BWAGPU_RESCUE_OVERFLOW;
      g.n_sw[p] = -1;
      g.pstate[p] = RP_DONE;
    }
    return;
  }
  for (int i = 0; i < 2; ++i) {
    copy_in(g, 2 * p + i, nin[i], lane);
    if (lane == 0) g.out_n[2 * p + i] = nin[i];
    cnt[i] = nin[i];
  }
  if (st != RP_PENDING) return;  // refused by rescue_init_kernel: the copy is its output
  if (g.round == 0 && uni(g.ntask[p]) == 0) {  // no call runs ksw_align2: nothing changes
    if (lane == 0) g.pstate[p] = RP_DONE;
    return;
  }
  post_sync();
  const Pes4 pes = load_pes(g.pes);
  const int64_t l_pac = ref.l_pac, two = l_pac << 1;
  const int64_t slot0 = uni64(g.slot_off[p]);
  const int nb0 = uni(g.nb0[p]), ncall = uni(g.nslot[p]) / 4;
  int code = 0;       // 1: a needed call was not computed, 2: a push did not fit
  int miss_call = 0;  // the call it happened in
  int total = 0, used = 0;
  for (int i = 0; i < 2 && !code; ++i) {
    const int rd = 2 * p + i, mate = 2 * p + (1 - i), mi = 1 - i;
    if (nin[i] <= 0) continue;
    const R* a = g.regs + uni64(g.reg_off[rd]);  // b[i]: the input is the snapshot
    R* ma = g.out_regs + uni64(g.out_off[mate]);
    const int l_ms = (int)(uni64(g.seq_off[mate + 1]) - uni64(g.seq_off[mate]));
    const int thr = uni(a[0].score) - g.po.pen_unpaired;
    const int kmax = i ? ncall - nb0 : nb0;
    int k = 0;
    for (int j = 0; j < nin[i] && k < kmax && !code; ++j) {
      if (uni(a[j].score) < thr) continue;
      const int call = (i ? nb0 : 0) + k;
      const int64_t sbase = slot0 + (int64_t)call * 4;
      ++k;
      // ---- mem_matesw(opt, bns, pac, pes, &b[i].a[j], l_ms, ms, &a[!i])
      const int64_t arb = uni64(a[j].rb);
      const int arid = uni(a[j].rid);
      const uint32_t aalt = (uint32_t)uni((int)a[j].n_comp_is_alt) & ~kCompMask;
      int skip[4];
      if (skip_test(l_pac, pes, arb, ma, cnt[mi], skip) == 4) continue;
      int n = 0;
      for (int r = 0; r < 4; ++r) {
        if (skip[r]) continue;
        int64_t rb, re;
        if (rescue_window(ref, pes, g.po.min_seed_len, arb, arid, l_ms, r, &rb, &re)) {
          const int tv = uni(g.tab[sbase + r]);
          if (tv < 0) {
            code = 1;
            miss_call = call;
            break;
          }
          const int rnd = tv >> kRescueIdxBits, t = tv & ((1 << kRescueIdxBits) - 1);
          const bwagpu_kswr_t* res = g.res[rnd] + t;
          const int sc = uni(res->score), aqb = uni(res->qb), aqe = uni(res->qe), atb = uni(res->tb),
                    ate = uni(res->te), sc2 = uni(res->score2);
          ++used;
          if (sc >= g.po.min_seed_len && aqb >= 0) {  // something goes wrong if aln.qb < 0
            if (cnt[mi] >= cap[mi]) {
              code = 2;
              break;
            }
            const bool is_rev = (r >> 1) != (r & 1);
            R b{};
            b.rid = arid;
            b.n_comp_is_alt = aalt;  // is_alt of a, n_comp = 0
            b.qb = is_rev ? l_ms - (aqe + 1) : aqb;
            b.qe = is_rev ? l_ms - aqb : aqe + 1;
            b.rb = is_rev ? two - (rb + ate + 1) : rb + atb;
            b.re = is_rev ? two - (rb + atb) : rb + ate + 1;
            b.score = sc;
            b.csub = sc2;
            b.secondary = -1;
            const int64_t rl = b.re - b.rb, ql = b.qe - b.qb;
            b.seedcov = (int)((rl < ql ? rl : ql) >> 1);
            const int mn = ++cnt[mi];  // kv_push, then move b so that ma stays sorted
            int x;
            for (x = 0; x < mn - 1; ++x)
              if (uni(ma[x].score) < b.score) break;
            const int at = x;
            for (x = mn - 1; x > at; --x) ma[x] = ma[x - 1];
            ma[at] = b;
          }
          ++n;
        }
        if (n && cnt[mi] > 1)  // mem_sort_dedup_patch(opt, 0, 0, 0, ...): returns at once for n <= 1
          cnt[mi] = uni(sort_dedup_walk<false>(g.po.max_chain_gap, g.po.mask_level_redun, cnt[mi], ma, 0));
      }
      total += n;
    }
  }
  post_sync();
  if (code) {  // the pair's output is a copy of its input
    for (int i = 0; i < 2; ++i) copy_in(g, 2 * p + i, nin[i], lane);
    if (code == 1)  // ask for this call's and every later call's live orientations
      for (int s = miss_call * 4 + lane; s < ncall * 4; s += 64)
        if (!pes.failed[s & 3] && g.tab[slot0 + s] == RS_NONE) g.tab[slot0 + s] = RS_WANTED;
    if (lane == 0) {
      g.out_n[2 * p] = nin[0];
      g.out_n[2 * p + 1] = nin[1];
      g.status[p] = code == 1 ? BWAGPU_RESCUE_UNFINISHED : BWAGPU_RESCUE_OVERFLOW;
      g.n_sw[p] = -1;
      g.pstate[p] = code == 1 ? RP_PENDING : RP_DONE;
      if (code == 1) atomicAdd(&g.ctr[RC_PENDING], 1);
    }
    return;
  }
  if (lane == 0) {
    g.out_n[2 * p] = cnt[0];
    g.out_n[2 * p + 1] = cnt[1];
    g.status[p] = BWAGPU_RESCUE_DONE;
    g.n_sw[p] = total;
    g.pstate[p] = RP_DONE;
    atomicAdd(&g.ctr[RC_USED], used);
  }
}

unsigned wave_blocks(int n_pairs) { return (unsigned)((n_pairs + kWpb - 1) / kWpb); }

}  // namespace

hipError_t launch_pestat(const DevOpt& o, const DevRef& ref, const PestatArgs& a, hipStream_t st) {
  if (a.n_pairs > 0)
    hipLaunchKernelGGL(pestat_collect_kernel, dim3((unsigned)((a.n_pairs + 255) / 256)), dim3(256), 0, st, o, ref, a);
  hipLaunchKernelGGL(pestat_finish_kernel, dim3(4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(pestat_ratio_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_rescue_pool(const RescueArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rescue_pool_kernel, dim3((unsigned)((2 * a.n_pairs + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_rescue_init(const DevOpt& o, const RescueArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rescue_init_kernel, dim3((unsigned)((a.n_pairs + 255) / 256)), dim3(256), 0, st, o, a);
  return hipGetLastError();
}

hipError_t launch_rescue_plan(const DevOpt& o, const DevRef& ref, const RescueArgs& a, bool emit, hipStream_t st) {
  if (emit)
    hipLaunchKernelGGL(rescue_plan_kernel<true>, dim3(wave_blocks(a.n_pairs)), dim3(64 * kWpb), 0, st, o, ref, a);
  else
    hipLaunchKernelGGL(rescue_plan_kernel<false>, dim3(wave_blocks(a.n_pairs)), dim3(64 * kWpb), 0, st, o, ref, a);
  return hipGetLastError();
}

hipError_t launch_rescue_apply(const DevOpt& o, const DevRef& ref, const RescueArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rescue_apply_kernel, dim3(wave_blocks(a.n_pairs)), dim3(64 * kWpb), 0, st, o, ref, a);
  return hipGetLastError();
}

}  // namespace bwagpu
