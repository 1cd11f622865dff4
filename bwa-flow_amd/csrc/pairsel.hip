// mem_approx_mapq_se and raw_mapq are compared with the reference's results bit
// for bit, and its build (x86-64, -O2) has no fused multiply-add: no
// contraction in this file (rescue.hip says why the intrinsics do not suffice).
#pragma clang fp contract(off)
// pairsel.hip — MI355X (gfx950) primary marking and pair selection of a batch
// of read pairs: mem_mark_primary_se (bwa/bwamem.c:502-567), and mem_sam_pe
// from bwamem_pair.c:286 to its first mem_reg2aln: mem_pair (:185-246), the
// proper-pair / unpaired decision and the mapq arithmetic (:288-336, :374-390,
// mem_approx_mapq_se, bwamem.c:967-991).  DESIGN.md §17.
//
// Both kernels run one wave per block.  A block takes 64 consecutive reads
// (pairs): first a lane per read settles the ones that need no sort (n <= 1;
// pairs with at most one primary region per read), then the wave takes the
// others one after another with lane = region and the keys in LDS.
//   * every loop is bounded by a count loaded before it starts;
//   * no wave waits for another: a block is one wave, __syncthreads() only
//     orders that wave's own LDS and scratch traffic and always sits under
//     wave-uniform control;
//   * LDS is reached only by indexing the __shared__ arrays below, never
//     through a generic pointer.
// The sorts' keys are unique (hash_64 is a bijection over distinct ids; v's y
// carries the index and the read), so a rank sort gives klib's introsort order.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "engine.h"
#include "pairsel.h"

namespace bwagpu {

namespace {

using R = bwagpu_alnreg_t;
constexpr int kWave = 64;
constexpr int kRegWords = (int)(sizeof(R) / sizeof(uint32_t));  // 22

// utils.h:98-109
__device__ __forceinline__ uint64_t hash_64(uint64_t key) {
  key += ~(key << 32);
  key ^= (key >> 22);
  key += ~(key << 13);
  key ^= (key >> 8);
  key += (key << 3);
  key ^= (key >> 15);
  key += ~(key << 27);
  key ^= (key >> 31);
  return key;
}

__device__ __forceinline__ int is_alt_of(const R& r) { return (int)(r.n_comp_is_alt >> 30); }

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

// ---------------------------------------------------------------- mem_mark_primary_se
// One read's regions, two banks: a sort reads one and writes the other.
// s_as = is_alt << 16 | the region's index in the input.
__shared__ int s_score[2][kSelCap], s_qb[2][kSelCap], s_qe[2][kSelCap], s_as[2][kSelCap];
__shared__ int s_sub[2][kSelCap], s_subn[2][kSelCap], s_altsc[2][kSelCap], s_sec[2][kSelCap], s_secall[2][kSelCap];
__shared__ uint64_t s_hash[2][kSelCap];
__shared__ int s_z[kSelCap], s_pos[kSelCap];

// mem_mark_primary_se_core (bwamem.c:502-528) on the first m entries of bank b:
// one i at a time, the test against z across the lanes.  z is ascending, so
// the first hit is the lowest set lane of the first ballot that has one.
__device__ void mark_core(int b, int m, int tmp, float mask_level, int lane) {
  if (lane == 0) s_z[0] = 0;
  int zn = 1;
  __syncthreads();
  for (int i = 1; i < m; ++i) {
    const int qbi = s_qb[b][i], qei = s_qe[b][i];
    int first = -1;
    for (int base = 0; base < zn; base += kWave) {
      const int k = base + lane;
      bool hit = false;
      if (k < zn) {
        const int j = s_z[k];
        const int qbj = s_qb[b][j], qej = s_qe[b][j];
        const int b_max = qbj > qbi ? qbj : qbi, e_min = qej < qei ? qej : qei;
        if (e_min > b_max) {
          const int min_l = qei - qbi < qej - qbj ? qei - qbi : qej - qbj;
          hit = (float)(e_min - b_max) >= (float)min_l * mask_level;  // int against int * float
        }
      }
      const uint64_t mask = __ballot(hit);
      if (mask) {
        first = base + __ffsll((unsigned long long)mask) - 1;
        break;
      }
    }
    if (lane == 0) {
      if (first >= 0) {
        const int j = s_z[first];
        if (s_sub[b][j] == 0) s_sub[b][j] = s_score[b][i];
        if (s_score[b][j] - s_score[b][i] <= tmp && ((s_as[b][j] >> 16) || !(s_as[b][i] >> 16))) ++s_subn[b][j];
        s_sec[b][i] = j;
      } else {
        s_z[zn] = i;
      }
    }
    if (first < 0) ++zn;
    __syncthreads();
  }
}

// alnreg_hlt / alnreg_hlt2 (bwamem.c:406, :409) of entries x, y of bank b
__device__ __forceinline__ bool hlt(int b, int x, int y) {
  const int sx = s_score[b][x], sy = s_score[b][y];
  if (sx != sy) return sx > sy;
  const int ax = s_as[b][x] >> 16, ay = s_as[b][y] >> 16;
  if (ax != ay) return ax < ay;
  return s_hash[b][x] < s_hash[b][y];
}
__device__ __forceinline__ bool hlt2(int b, int x, int y) {
  const int ax = s_as[b][x] >> 16, ay = s_as[b][y] >> 16;
  if (ax != ay) return ax < ay;
  const int sx = s_score[b][x], sy = s_score[b][y];
  if (sx != sy) return sx > sy;
  return s_hash[b][x] < s_hash[b][y];
}

// one read of 2 <= n <= kSelCap regions, the whole wave; -> n_pri
__device__ int mark_wave(const MarkArgs& g, int r, int n, int lane) {
  R* a = g.regs + g.reg_off[r];
  const uint64_t id = (uint64_t)(g.id0 + r);
  __syncthreads();  // the previous read's LDS is dead
  // bank 0: the keys in input order
  int n_pri = 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    bool pri = false;
    if (i < n) {
      const int alt = is_alt_of(a[i]);
      s_score[0][i] = a[i].score;
      s_qb[0][i] = a[i].qb;
      s_qe[0][i] = a[i].qe;
      s_as[0][i] = alt << 16 | i;
      s_subn[0][i] = a[i].sub_n;
      s_hash[0][i] = hash_64(id + (uint64_t)i);
      pri = alt == 0;
    }
    n_pri += __popcll(__ballot(pri));
  }
  __syncthreads();
  // bank 1: sorted by mem_ars_hash, bwamem.c:536's initial values
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += j != i && hlt(0, j, i);
      s_score[1][rank] = s_score[0][i];
      s_qb[1][rank] = s_qb[0][i];
      s_qe[1][rank] = s_qe[0][i];
      s_as[1][rank] = s_as[0][i];
      s_subn[1][rank] = s_subn[0][i];
      s_hash[1][rank] = s_hash[0][i];
      s_sub[1][rank] = 0;
      s_altsc[1][rank] = 0;
      s_sec[1][rank] = -1;
    }
  }
  mark_core(1, n, g.tmp, g.mask_level, lane);
  // bwamem.c:541-546
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      const int sec = s_sec[1][i];
      if (!(s_as[1][i] >> 16) && sec >= 0 && (s_as[1][sec] >> 16)) s_altsc[1][i] = s_score[1][sec];
    }
  }
  // bwamem.c:547-564 into bank 0: the position under mem_ars_hash2 when the
  // read has both kinds of hits, the same position otherwise
  const bool mixed = n_pri < n;
  const bool resort = mixed && n_pri > 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      int rank = i;
      if (resort) {
        rank = 0;
        for (int j = 0; j < n; ++j) rank += j != i && hlt2(1, j, i);
      }
      s_pos[i] = rank;
    }
  }
  __syncthreads();
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    if (i < n) {
      const int p = s_pos[i], sec = s_sec[1][i], alt = s_as[1][i] >> 16;
      s_score[0][p] = s_score[1][i];
      s_qb[0][p] = s_qb[1][i];
      s_qe[0][p] = s_qe[1][i];
      s_as[0][p] = s_as[1][i];
      s_subn[0][p] = s_subn[1][i];
      s_hash[0][p] = s_hash[1][i];
      s_altsc[0][p] = s_altsc[1][i];
      if (mixed) {
        s_secall[0][p] = sec >= 0 ? s_pos[sec] : -1;
        const bool pri = resort && p < n_pri;  // :558
        s_sec[0][p] = pri ? -1 : (sec >= 0 && alt) ? INT_MAX : sec;
        s_sub[0][p] = pri ? 0 : s_sub[1][i];
      } else {
        s_secall[0][p] = sec;
        s_sec[0][p] = sec;
        s_sub[0][p] = s_sub[1][i];
      }
    }
  }
  if (resort) mark_core(0, n_pri, g.tmp, g.mask_level, lane);
  else __syncthreads();
  // the records move once: by final position into the block's scratch, then back as words
  R* tmp = g.scratch + (size_t)blockIdx.x * kSelCap;
  for (int base = 0; base < n; base += kWave) {
    const int p = base + lane;
    if (p < n) {
      R rec = a[s_as[0][p] & 0xffff];
      rec.sub = s_sub[0][p];
      rec.sub_n = s_subn[0][p];
      rec.alt_sc = s_altsc[0][p];
      rec.secondary = s_sec[0][p];
      rec.secondary_all = s_secall[0][p];
      rec.hash = s_hash[0][p];
      tmp[p] = rec;
    }
  }
  __syncthreads();
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tmp);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a);
  const int words = n * kRegWords;
  for (int w = lane; w < words; w += kWave) dst[w] = src[w];
  return n_pri;
}

__global__ void __launch_bounds__(kWave) mark_primary_kernel(MarkArgs g) {
  const int lane = (int)threadIdx.x;
  const int groups = (g.n_reads + kWave - 1) / kWave;
  for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
    const int r0 = grp * kWave, r = r0 + lane;
    int nr = 0;
    if (r < g.n_reads) {
      nr = g.n[r];
      if (nr < 0) nr = 0;
      int n_pri = 0;
      if (nr == 1) {  // the closed form of bwamem.c:534-566 for one region
        R* a = g.regs + g.reg_off[r];
        a->sub = a->alt_sc = 0;
        a->secondary = a->secondary_all = -1;
        a->hash = hash_64((uint64_t)(g.id0 + r));
        n_pri = is_alt_of(*a) == 0;
      }
      if (nr <= 1 || nr > kSelCap) {
        g.n_pri[r] = n_pri;
        g.status[r] = nr > kSelCap ? BWAGPU_SEL_TOO_MANY : BWAGPU_SEL_DONE;
      }
    }
    const int cnt = g.n_reads - r0 < kWave ? g.n_reads - r0 : kWave;
    for (int k = 0; k < cnt; ++k) {
      const int nk = uni(__shfl(nr, k));
      if (nk < 2 || nk > kSelCap) continue;
      const int n_pri = mark_wave(g, r0 + k, nk, lane);
      if (lane == 0) {
        g.n_pri[r0 + k] = n_pri;
        g.status[r0 + k] = BWAGPU_SEL_DONE;
      }
    }
  }
}

// ---------------------------------------------------------------- mem_pair and the decision
__shared__ uint64_t s_vx[2][kSelCap], s_vy[2][kSelCap];

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
  return (uint64_t)hi << 32 | lo;
}

// log(k) from the context's table; an argument outside [1, log_n) sets *bad
__device__ __forceinline__ double tab_log(const PairSelArgs& g, int k, bool* bad) {
  if (k < 1 || k >= g.log_n) {
    *bad = true;
    return 0.;
  }
  return g.log_tab[k];
}

__device__ __forceinline__ int raw_mapq(int diff, int a) { return (int)(6.02 * diff / a + .499); }

// mem_approx_mapq_se (bwamem.c:967-991) of region r with `sub` in place of r.sub
__device__ int approx_mapq(const PairSelArgs& g, const R& r, int r_sub, bool* bad) {
  int mapq, sub = r_sub ? r_sub : g.so.min_seed_len * g.a;
  sub = r.csub > sub ? r.csub : sub;
  if (sub >= r.score) return 0;
  const int l = (int)((int64_t)(r.qe - r.qb) > r.re - r.rb ? (int64_t)(r.qe - r.qb) : r.re - r.rb);
  if (l <= 0) {
    *bad = true;
    return 0;
  }
  const double identity = 1. - (double)(l * g.a - r.score) / (g.a + g.b) / l;
  if (r.score == 0) {
    mapq = 0;
  } else if (g.so.mapQ_coef_len > 0) {
    double tmp = (float)l < g.so.mapQ_coef_len ? 1. : g.so.mapQ_coef_fac / tab_log(g, l, bad);
    tmp *= identity * identity;
    mapq = (int)(6.02 * (r.score - sub) / g.a * tmp * tmp + .499);
  } else {
    mapq = (int)(30.0 * (1. - (double)sub / r.score) * tab_log(g, r.seedcov, bad) + .499);
    mapq = identity < 0.95 ? (int)(mapq * identity * identity + .499) : mapq;
  }
  if (r.sub_n > 0) mapq -= (int)(4.343 * tab_log(g, r.sub_n + 1, bad) + .499);
  if (mapq > 60) mapq = 60;
  if (mapq < 0) mapq = 0;
  mapq = (int)(mapq * (1. - r.frac_rep) + .499);
  return mapq;
}

// mem_infer_dir (bwamem_pair.c:26-33)
__device__ __forceinline__ int infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t* dist) {
  const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
  const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
  *dist = p2 > b1 ? p2 - b1 : b1 - p2;
  return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// v's key of region i of read r (bwamem_pair.c:195-197)
__device__ __forceinline__ void v_key(const DevRef& ref, const R& e, int i, int r, uint64_t* x, uint64_t* y) {
  const int64_t pos = e.rb < ref.l_pac ? e.rb : (ref.l_pac << 1) - 1 - e.rb;
  const int64_t off = e.rid >= 0 && e.rid < ref.n_seqs ? ref.ann_offset[e.rid] : 0;
  *x = (uint64_t)e.rid << 32 | (uint64_t)(pos - off);
  *y = (uint64_t)e.score << 32 | (uint64_t)(uint32_t)(i << 2 | (e.rb >= ref.l_pac) << 1 | r);
}

// u's entry for sorted positions k < i of v, if the two hits pair up
// (bwamem_pair.c:205-226; of the two directions only r = k's strand can pass
// the test on `which`) -> false, or true with the entry's 128-bit key
__device__ __forceinline__ bool u_entry(const PairSelArgs& g, uint64_t idt, uint64_t xi, uint64_t yi, uint64_t xk,
                                        uint64_t yk, int i, int k, uint64_t* ux, uint64_t* uy) {
  if (((yk ^ yi) & 1) == 0) return false;  // the same read
  const int r = (int)(yk >> 1 & 1), dir = r << 1 | (int)(yi >> 1 & 1);
  if (g.pes[dir].failed) return false;
  const int64_t dist = (int64_t)xi - (int64_t)xk;
  if (dist > g.pes[dir].high || dist < g.pes[dir].low) return false;
  int q = (int)((double)((yi >> 32) + (yk >> 32)) + g.erfc_tab[dir][dist - g.pes[dir].low] * g.a + .499);
  if (q < 0) q = 0;
  *uy = (uint64_t)k << 32 | (uint64_t)i;
  *ux = (uint64_t)q << 32 | (hash_64(*uy ^ idt) & 0xffffffffU);
  return true;
}

struct PairRes {
  int o, sub, n_sub, z[2];
};

// hash_64(p->y ^ id<<8) of pair p: the reference's id is an int, so id << 8
// wraps and is sign-extended into the XOR
__device__ __forceinline__ uint64_t id_term(const PairSelArgs& g, int p) {
  return (uint64_t)(int64_t)(int32_t)((uint32_t)(g.pair_id0 + p) << 8);
}

// mem_pair of pair p with 2 < np0 + np1 <= kSelCap (or any count), the whole wave
__device__ PairRes pair_wave(const DevRef& ref, const PairSelArgs& g, int p, int np0, int np1, int lane) {
  const uint64_t idt = id_term(g, p);
  const R* a0 = g.regs + g.reg_off[2 * p];
  const R* a1 = g.regs + g.reg_off[2 * p + 1];
  const int m = np0 + np1;
  __syncthreads();  // the previous pair's LDS is dead
  for (int base = 0; base < m; base += kWave) {
    const int idx = base + lane;
    if (idx < m) {
      const int r = idx >= np0, i = r ? idx - np0 : idx;
      v_key(ref, r ? a1[i] : a0[i], i, r, &s_vx[0][idx], &s_vy[0][idx]);
    }
  }
  __syncthreads();
  for (int base = 0; base < m; base += kWave) {
    const int idx = base + lane;
    if (idx < m) {
      const uint64_t x = s_vx[0][idx], y = s_vy[0][idx];
      int rank = 0;
      for (int j = 0; j < m; ++j) {
        const uint64_t xj = s_vx[0][j], yj = s_vy[0][j];
        rank += xj < x || (xj == x && yj < y);
      }
      s_vx[1][rank] = x;
      s_vy[1][rank] = y;
    }
  }
  __syncthreads();
  // u is never stored: its maximum, the maximum of the rest, and the count of
  // the rest within tmp of that are three passes over the candidate pairs
  PairRes res{0, 0, 0, {0, 0}};
  uint64_t bx = 0, by = 0;  // below every entry: an entry's y holds i >= 1
  int cnt = 0;
  for (int i = lane; i < m; i += kWave) {
    const uint64_t xi = s_vx[1][i], yi = s_vy[1][i];
    for (int k = 0; k < i; ++k) {
      uint64_t ux, uy;
      if (!u_entry(g, idt, xi, yi, s_vx[1][k], s_vy[1][k], i, k, &ux, &uy)) continue;
      ++cnt;
      if (ux > bx || (ux == bx && uy > by)) bx = ux, by = uy;
    }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint64_t ox = shfl_xor_u64(bx, o), oy = shfl_xor_u64(by, o);
    if (ox > bx || (ox == bx && oy > by)) bx = ox, by = oy;
    cnt += __shfl_xor(cnt, o);
  }
  if (cnt == 0) return res;
  uint64_t cx = 0, cy = 0;
  for (int i = lane; i < m; i += kWave) {
    const uint64_t xi = s_vx[1][i], yi = s_vy[1][i];
    for (int k = 0; k < i; ++k) {
      uint64_t ux, uy;
      if (!u_entry(g, idt, xi, yi, s_vx[1][k], s_vy[1][k], i, k, &ux, &uy) || uy == by) continue;
      if (ux > cx || (ux == cx && uy > cy)) cx = ux, cy = uy;
    }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint64_t ox = shfl_xor_u64(cx, o), oy = shfl_xor_u64(cy, o);
    if (ox > cx || (ox == cx && oy > cy)) cx = ox, cy = oy;
  }
  res.o = (int)(bx >> 32);
  res.sub = cnt > 1 ? (int)(cx >> 32) : 0;
  int n_sub = 0;
  for (int i = lane; i < m; i += kWave) {
    const uint64_t xi = s_vx[1][i], yi = s_vy[1][i];
    for (int k = 0; k < i; ++k) {
      uint64_t ux, uy;
      if (!u_entry(g, idt, xi, yi, s_vx[1][k], s_vy[1][k], i, k, &ux, &uy) || uy == by) continue;
      n_sub += res.sub - (int)(ux >> 32) <= g.tmp;
    }
  }
  for (int o = kWave / 2; o > 0; o >>= 1) n_sub += __shfl_xor(n_sub, o);
  res.n_sub = n_sub;
  const uint64_t y1 = s_vy[1][(int)(by >> 32)], y2 = s_vy[1][(int)(uint32_t)by];
  res.z[y1 & 1] = (int)((uint32_t)y1 >> 2);
  res.z[y2 & 1] = (int)((uint32_t)y2 >> 2);
  return res;
}

// mem_pair of a pair with one primary region per read: v has two entries, u at most one
__device__ PairRes pair_single(const DevRef& ref, const PairSelArgs& g, int p) {
  uint64_t x[2], y[2];
  v_key(ref, g.regs[g.reg_off[2 * p]], 0, 0, &x[0], &y[0]);
  v_key(ref, g.regs[g.reg_off[2 * p + 1]], 0, 1, &x[1], &y[1]);
  const int k = x[0] < x[1] || (x[0] == x[1] && y[0] < y[1]) ? 0 : 1;  // the earlier of the two
  PairRes res{0, 0, 0, {0, 0}};
  uint64_t ux, uy;
  if (u_entry(g, id_term(g, p), x[k ^ 1], y[k ^ 1], x[k], y[k], 1, 0, &ux, &uy)) res.o = (int)(ux >> 32);
  return res;
}

// Everything after mem_pair for pair p, one lane: `called` says whether res is
// mem_pair's result.  Nothing is written to the regions before the pair is known
// to finish.
__device__ void pair_tail(const DevRef& ref, const PairSelArgs& g, int p, bool called, PairRes res) {
  R* a[2] = {g.regs + g.reg_off[2 * p], g.regs + g.reg_off[2 * p + 1]};
  int32_t* om[2] = {g.out_mapq + g.reg_off[2 * p], g.out_mapq + g.reg_off[2 * p + 1]};
  int n[2], np[2];
  for (int i = 0; i < 2; ++i) {
    n[i] = g.n[2 * p + i] < 0 ? 0 : g.n[2 * p + i];
    np[i] = g.n_pri[2 * p + i] < 0 ? 0 : g.n_pri[2 * p + i] > n[i] ? n[i] : g.n_pri[2 * p + i];
  }
  const bool nopair = (g.so.flags & BWAGPU_MEM_F_NOPAIRING) != 0;
  bwagpu_pairsel_t s{};
  s.status = BWAGPU_SEL_DONE;
  s.n_pri[0] = np[0];
  s.n_pri[1] = np[1];
  s.z[0] = s.z[1] = -1;
  s.alt[0] = s.alt[1] = -1;
  s.extra_flag = 1;
  if (called) s.o = res.o, s.subo = res.sub, s.n_sub = res.n_sub;
  bool bad = false, paired = false;
  if (called && res.o > 0) {  // bwamem_pair.c:292-297
    paired = true;
    for (int i = 0; i < 2; ++i)
      for (int j = 1; j < np[i]; ++j)
        if (a[i][j].secondary < 0 && a[i][j].score >= g.so.T) {
          paired = false;
          break;
        }
  }
  if (paired) {
    int z[2] = {res.z[0], res.z[1]}, q_se[2], new_sub[2] = {0, 0}, gq[2] = {0, 0};
    bool promote[2] = {false, false};
    const int score_un = a[0][0].score + a[1][0].score - g.so.pen_unpaired;
    const int subo = res.sub > score_un ? res.sub : score_un;
    int q_pe = raw_mapq(res.o - subo, g.a);
    if (res.n_sub > 0) q_pe -= (int)(4.343 * tab_log(g, res.n_sub + 1, &bad) + .499);
    if (q_pe < 0) q_pe = 0;
    if (q_pe > 60) q_pe = 60;
    q_pe = (int)(q_pe * (1. - .5 * (a[0][0].frac_rep + a[1][0].frac_rep)) + .499);
    if (res.o > score_un) {  // the paired alignment is preferred
      for (int i = 0; i < 2; ++i) {
        const R& c = a[i][z[i]];
        new_sub[i] = c.sub;
        if (c.secondary >= n[i]) bad = true;
        else if (c.secondary >= 0) new_sub[i] = a[i][c.secondary].score, promote[i] = true;
        q_se[i] = approx_mapq(g, c, new_sub[i], &bad);
        q_se[i] = q_se[i] > q_pe ? q_se[i] : q_pe < q_se[i] + 40 ? q_pe : q_se[i] + 40;
        const int cap = raw_mapq(c.score - c.csub, g.a);  // the tandem repeat score
        q_se[i] = (q_se[i] < cap ? q_se[i] : cap) & 0xff;  // mem_aln_t.mapq has 8 bits: a negative cap (csub > score) wraps
      }
      s.extra_flag |= 2;
    } else {  // the unpaired alignment is preferred
      z[0] = z[1] = 0;
      for (int i = 0; i < 2; ++i) q_se[i] = approx_mapq(g, a[i][0], a[i][0].sub, &bad);
    }
    for (int i = 0; i < 2; ++i)  // g[i], bwamem_pair.c:348-354: secondary_all does not enter its mapq
      if (np[i] < n[i]) {
        const R& h = a[i][np[i]];
        if (h.score < g.so.T || h.secondary >= 0 || !is_alt_of(h)) continue;
        s.alt[i] = np[i];
        gq[i] = approx_mapq(g, h, h.sub, &bad);
      }
    if (!bad) {
      s.branch = BWAGPU_SEL_PAIRED;
      for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < n[i]; ++j) om[i][j] = -1;
        R& c = a[i][z[i]];
        if (promote[i]) c.sub = new_sub[i], c.secondary = -2;
        const int k = c.secondary_all;
        if (k >= 0 && k < np[i]) {  // switch secondary and primary, :327-336
          for (int j = 0; j < n[i]; ++j)
            if (a[i][j].secondary_all == k || j == k) a[i][j].secondary_all = z[i];
          c.secondary_all = -1;
        }
        s.z[i] = z[i];
        s.mapq[i] = q_se[i];
        om[i][z[i]] = q_se[i];
        if (s.alt[i] >= 0) om[i][s.alt[i]] = gq[i];
      }
    }
  } else {  // no_pairing, bwamem_pair.c:374-392 and mem_reg2sam's selection
    int rid[2];
    for (int i = 0; i < 2; ++i) {
      int which = -1;
      if (n[i]) {
        if (a[i][0].score >= g.so.T) which = 0;
        else if (np[i] < n[i] && a[i][np[i]].score >= g.so.T) which = np[i];
      }
      rid[i] = -1;
      if (which >= 0) {
        const R& h = a[i][which];
        if (h.rb >= 0 && h.re >= 0) rid[i] = h.rid;
        s.mapq[i] = h.secondary < 0 ? approx_mapq(g, h, h.sub, &bad) : 0;  // mem_reg2aln, bwamem.c:1121
      }
      s.z[i] = which;
      int l = 0, first = 0;
      for (int j = 0; j < n[i]; ++j) {  // bwamem.c:1030-1047 without MEM_F_ALL
        const R& h = a[i][j];
        int q = -1;
        if (h.score >= g.so.T && h.secondary < 0) {
          q = approx_mapq(g, h, h.sub, &bad);
          if (l && !is_alt_of(h) && q > first) q = first;
          if (!l) first = q;
          ++l;
        }
        om[i][j] = q;
      }
    }
    if (!nopair && rid[0] == rid[1] && rid[0] >= 0) {
      int64_t dist;
      const int d = infer_dir(ref.l_pac, a[0][0].rb, a[1][0].rb, &dist);
      if (!g.pes[d].failed && dist >= g.pes[d].low && dist <= g.pes[d].high) s.extra_flag |= 2;
    }
  }
  if (bad) {
    bwagpu_pairsel_t t{};
    t.status = BWAGPU_SEL_TOO_MANY;
    t.n_pri[0] = np[0];
    t.n_pri[1] = np[1];
    t.z[0] = t.z[1] = t.alt[0] = t.alt[1] = -1;
    s = t;
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < n[i]; ++j) om[i][j] = -1;
  }
  g.sel[p] = s;
}

// a pair that is not evaluated: its record and out_mapq entries, the regions untouched
__device__ void pair_refuse(const PairSelArgs& g, int p, int status) {
  bwagpu_pairsel_t t{};
  t.status = status;
  t.z[0] = t.z[1] = t.alt[0] = t.alt[1] = -1;
  for (int i = 0; i < 2; ++i) {
    const int n = g.n[2 * p + i];
    t.n_pri[i] = g.n_pri[2 * p + i];
    int32_t* om = g.out_mapq + g.reg_off[2 * p + i];
    for (int j = 0; j < n; ++j) om[j] = -1;
  }
  g.sel[p] = t;
}

enum { PK_NONE = 0, PK_WAVE = 1 };

__global__ void __launch_bounds__(kWave) pair_select_kernel(DevRef ref, PairSelArgs g) {
  const int lane = (int)threadIdx.x;
  const int groups = (g.n_pairs + kWave - 1) / kWave;
  const bool nopair = (g.so.flags & BWAGPU_MEM_F_NOPAIRING) != 0;
  for (int grp = (int)blockIdx.x; grp < groups; grp += (int)gridDim.x) {
    const int p0 = grp * kWave, p = p0 + lane;
    int kind = PK_NONE, np0 = 0, np1 = 0;
    if (p < g.n_pairs) {
      const int n0 = g.n[2 * p] < 0 ? 0 : g.n[2 * p], n1 = g.n[2 * p + 1] < 0 ? 0 : g.n[2 * p + 1];
      np0 = g.n_pri[2 * p] < 0 ? 0 : g.n_pri[2 * p] > n0 ? n0 : g.n_pri[2 * p];
      np1 = g.n_pri[2 * p + 1] < 0 ? 0 : g.n_pri[2 * p + 1] > n1 ? n1 : g.n_pri[2 * p + 1];
      if (g.in_status && g.in_status[p] != 0) {
        pair_refuse(g, p, BWAGPU_SEL_SKIPPED);
      } else if ((int64_t)np0 + np1 > kSelCap) {
        pair_refuse(g, p, BWAGPU_SEL_TOO_MANY);
      } else if (nopair || np0 == 0 || np1 == 0) {
        pair_tail(ref, g, p, false, PairRes{0, 0, 0, {0, 0}});
      } else if (np0 == 1 && np1 == 1) {
        pair_tail(ref, g, p, true, pair_single(ref, g, p));
      } else {
        kind = PK_WAVE;
      }
    }
    const int cnt = g.n_pairs - p0 < kWave ? g.n_pairs - p0 : kWave;
    for (int k = 0; k < cnt; ++k) {
      if (uni(__shfl(kind, k)) != PK_WAVE) continue;
      const PairRes res = pair_wave(ref, g, p0 + k, uni(__shfl(np0, k)), uni(__shfl(np1, k)), lane);
      if (lane == 0) pair_tail(ref, g, p0 + k, true, res);
    }
  }
}

int grid_of(int items) {
  const int groups = (items + kWave - 1) / kWave;
  return groups < kSelMaxBlocks ? (groups > 0 ? groups : 1) : kSelMaxBlocks;
}

}  // namespace

hipError_t launch_mark_primary(const MarkArgs& a, hipStream_t st) {
  if (a.n_reads <= 0) return hipSuccess;
  hipLaunchKernelGGL(mark_primary_kernel, dim3(grid_of(a.n_reads)), dim3(kWave), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pair_select(const DevRef& ref, const PairSelArgs& a, hipStream_t st) {
  if (a.n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(pair_select_kernel, dim3(grid_of(a.n_pairs)), dim3(kWave), 0, st, ref, a);
  return hipGetLastError();
}

}  // namespace bwagpu
