// spec.hip — the speculative mem_chain2aln (default path of
// bwagpu_chain2aln): extension task rounds on persistent grids
// (one, two or four ksw_extend2 calls per wave, ksw_dev.h) and the selection
// passes that replay bwa's sequential seed logic (bwamem.c:641-795) exactly
// over the precomputed extensions.  The phased extension (the first bin's
// side kernels and their lists' sort) is a translation unit of its own,
// spec_side.hip; spec_dev.h has what the two share.
#include "spec_dev.h"

namespace bwagpu {

// per-read selection trace (bwagpu_debug_set_trace; this file's copy)
__device__ uint32_t* g_trace = nullptr;
hipError_t set_trace_spec(void* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &p, sizeof(p)); }

// ============================================================ speculative chain2aln
// mem_chain2aln (bwamem.c:641-795) restructured for load balance on
// reference-seeded batches, where a few reads (tandem repeats: hundreds of
// seeds, one region each) carry more DP than thousands of ordinary reads and,
// run serially by one wave, set the stage's critical path.
//
// The one sequential dependency of mem_chain2aln is the decision whether a
// seed is extended at all: the containment test against the read's regions so
// far (bwamem.c:678-697) and the overlapping-seed test (698-707).  The
// extension itself (717-792: left ksw_extend2 with the band retry, right
// ksw_extend2 from the left score, local vs to-end choice) depends only on the
// seed, the read and its chain's window.  So:
//   round A   extend the first seed (processing order) of every chain — it is
//             almost always extended; one wave per task, dynamic queue;
//   emulate   replay the sequential logic per read with the round-A regions:
//             every seed that would be extended and has no result yet becomes
//             a round-B task (its region unknown, so later seeds of the read
//             are tested against fewer regions: a superset is predicted);
//   round B   extend those;
//   final     replay the sequential logic exactly, with every result it needs
//             precomputed except rare mispredictions, which it computes inline.
// Output = the reference's regions, byte for byte; the stats count only the DP
// of extensions mem_chain2aln performs (spec work is a separate diagnostic).

// lane per chain: window (bwamem.c:648-668 + bns_fetch_seq's clipping), the
// round-A task (the chain's first seed in processing order) and, for chains
// of up to kOrderLane seeds, the processing order; longer chains are listed
// for spec_order_kernel, which does their window and order one workgroup
// each (a lane looping over ~170 seeds was this kernel's tail).  chain_read
// comes from spec_reads_kernel.
__global__ void __launch_bounds__(256) spec_chain_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a) {
  sel_prio();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  bool task = false, longc = false;
  int bin = 0, s0 = 0;
  if (c < b.n_chains) {
    const int rd = a.chain_read[c];
    s0 = b.chain_seed_off[c];
    const int ns = b.chain_seed_off[c + 1] - s0;
    const int lq = (int)(b.seq_off[rd + 1] - b.seq_off[rd]);
    if (ns <= 0) {
      a.win[c] = ChainWin{0, 0};
    } else {
      int64_t wlo = ref.l_pac << 1, whi = 0;
      longc = ns > kOrderLane;
      if (!longc) {
        // the processing order (descending key score<<32|i, bwamem.c:671-676),
        // ranked in registers
        uint64_t key[kOrderLane];
#pragma unroll
        for (int t = 0; t < kOrderLane; ++t) {
          key[t] = ~0ull;
          if (t < ns) {
            const bwagpu_seed_t v = b.seeds[s0 + t];
            key[t] = (uint64_t)(uint32_t)v.score << 32 | (uint32_t)t;
            seed_reach(o, v, lq, wlo, whi);
          }
        }
#pragma unroll
        for (int t = 0; t < kOrderLane; ++t) {
          if (t < ns) {
            int rank = 0;
#pragma unroll
            for (int u = 0; u < kOrderLane; ++u) rank += key[u] < key[t];
            bwagpu_seed_t v = b.seeds[s0 + t];
            v.pad_ = key[t] == 0 ? 1 : 0;
            a.prog[s0 + ns - 1 - rank] = v;
            a.seedchain[s0 + ns - 1 - rank] = c;
          }
        }
      }
      const bool ok = finish_window(ref, b.chain_rid[c], b.seeds[s0].rbeg, wlo, whi);
      if (!ok) {
        atomicOr((unsigned long long*)&a.stats[ST_ERR], (unsigned long long)ERR_RID);
        a.win[c] = ChainWin{0, -1};
      } else {
        if (!longc) a.win[c] = ChainWin{wlo, whi};
        task = lq <= a.lq_bound;
        bin = spec_bin(lq);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kSpecBins; ++k) {
    const int p = wave_append(&a.ctr[SPC_CNT + k], task && bin == k);
    if (p >= 0) a.tasks[(size_t)k * b.n_chains + p] = make_int2(s0, c);
  }
  const int p = wave_append(&a.ctr[SPC_LONG_N], longc);
  if (p >= 0) a.longc[p] = c;
}

// lane per read: length check, and the list of heavy reads (selected first)
__global__ void __launch_bounds__(256) spec_reads_kernel(DevBatch b, SpecArgs a) {
  sel_prio();
  const int rd = blockIdx.x * blockDim.x + threadIdx.x;
  bool heavy = false;
  int ns = 0;
  if (rd < b.n_reads) {
    const int lq = (int)(b.seq_off[rd + 1] - b.seq_off[rd]);
    if (lq > a.lq_bound) atomicOr((unsigned long long*)&a.stats[ST_ERR], (unsigned long long)ERR_LEN);
    ReadDesc d;
    d.qoff = b.seq_off[rd];
    d.rd = rd;
    d.lq = lq;
    d.c0 = b.read_chain_off[rd];
    d.nch = b.read_chain_off[rd + 1] - d.c0;
    d.s0 = b.chain_seed_off[d.c0];
    d.ns = b.chain_seed_off[d.c0 + d.nch] - d.s0;
    a.rdesc[rd] = d;
    for (int c = d.c0; c < d.c0 + d.nch; ++c) a.chain_read[c] = rd;
    heavy = d.ns > kSelLight || d.nch > kSelLight;
    ns = d.ns;
  }
  const int p = wave_append(&a.ctr[SPC_HEAVY_N], heavy);
  if (p >= 0) {
    a.heavy[p] = rd;
    // the read's pair matrices (kSelMatMaxSeeds seeds at most, and room left)
    const long long words = 2 * tri_off(ns);
    int woff = -1, col = 0;
    if (ns <= kSelMatMaxSeeds) {
      const long long o = (long long)atomicAdd(reinterpret_cast<unsigned long long*>(&a.ctr[SPC_MATW64]),
                                               (unsigned long long)words);
      if (o + words <= a.mat_words) {
        woff = (int)o;
        col = atomicAdd(&a.ctr[SPC_HCOLS], ns);
        for (int i = 0; i < ns; ++i) a.colent[col + i] = p;
      }
    }
    a.hinfo[p] = make_int4(rd, woff, col, ns);
  }
}

// The processing order (descending key score<<32|i, bwamem.c:671-676) of
// the chains spec_chain_kernel listed (more than kOrderLane seeds), by
// ranking: keys are unique, so rank = the number of smaller keys.  One
// workgroup per chain with the keys staged in LDS (a lane looping over global
// keys made the longest chain, ~170 seeds, a 250 us tail).  pad_ = 1 flags
// the key that is 0 from the start (skipped by the overlap test like a
// marked seed, bwamem.c:700).
constexpr int kOrderBlocks = 1024;
constexpr int kOrderLds = 4096;  // longer chains rank against global memory
__device__ __forceinline__ uint64_t order_key(const bwagpu_seed_t* sd, int i) {
  return (uint64_t)(uint32_t)sd[i].score << 32 | (uint32_t)i;
}
__global__ void __launch_bounds__(256) spec_order_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a) {
  sel_prio();
  __shared__ uint64_t keys[kOrderLds];
  __shared__ int64_t wred[2][4];
  const int tid = (int)threadIdx.x;
  const int n_long = __hip_atomic_load(&a.ctr[SPC_LONG_N], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int gi = (int)blockIdx.x; gi < n_long; gi += (int)gridDim.x) {
    const int g = a.longc[gi];
    const int s0 = b.chain_seed_off[g], ns = b.chain_seed_off[g + 1] - s0;
    const bwagpu_seed_t* sd = b.seeds + s0;
    const bool in_lds = ns <= kOrderLds;
    const int rd = a.chain_read[g];
    const int lq = (int)(b.seq_off[rd + 1] - b.seq_off[rd]);
    int64_t wlo = ref.l_pac << 1, whi = 0;
    for (int i = tid; i < ns; i += 256) {
      const bwagpu_seed_t v = sd[i];
      if (in_lds) keys[i] = (uint64_t)(uint32_t)v.score << 32 | (uint32_t)i;
      seed_reach(o, v, lq, wlo, whi);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      wlo = min(wlo, (int64_t)__shfl_xor((long long)wlo, m, 64));
      whi = max(whi, (int64_t)__shfl_xor((long long)whi, m, 64));
    }
    if ((tid & 63) == 0) {
      wred[0][tid >> 6] = wlo;
      wred[1][tid >> 6] = whi;
    }
    __syncthreads();
    if (tid == 0) {
      wlo = min(min(wred[0][0], wred[0][1]), min(wred[0][2], wred[0][3]));
      whi = max(max(wred[1][0], wred[1][1]), max(wred[1][2], wred[1][3]));
      if (finish_window(ref, b.chain_rid[g], sd[0].rbeg, wlo, whi)) a.win[g] = ChainWin{wlo, whi};
    }
    for (int i = tid; i < ns; i += 256) {
      bwagpu_seed_t v = sd[i];
      const uint64_t ki = (uint64_t)(uint32_t)v.score << 32 | (uint32_t)i;
      int rank = 0;
      if (in_lds)
        for (int j = 0; j < ns; ++j) rank += keys[j] < ki;
      else
        for (int j = 0; j < ns; ++j) rank += order_key(sd, j) < ki;
      v.pad_ = ki == 0 ? 1 : 0;
      a.prog[s0 + ns - 1 - rank] = v;
      a.seedchain[s0 + ns - 1 - rank] = g;
    }
    __syncthreads();
  }
}


// Extension tasks of one list (round * kSpecBins + bin): one wave per task,
// claimed one at a time from the sharded queue (a wave holding a second task
// while others idle at the end of the list cost more: DESIGN.md §5).
template <int C>
__global__ void __launch_bounds__(kBlock) spec_ext_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int list,
                                                          int tb_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int wib = uni((int)(threadIdx.x >> 6));
  uint8_t* const tbl = lds + wib * 2 * tb_bytes;
  uint8_t* const tbr = tbl + tb_bytes;
  const int n = uni(__hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const int2* tl = a.tasks + spec_list_off(list, b.n_chains, b.n_seeds);
  ShardQ qq;
  qq.init(a.qh + 8 * kQHStride * list, n);
  long long spec_cells = 0;
  int m0, cap;
  while (qq.claim(1, m0, cap)) {
    for (int m = m0; m < m0 + 1 && m < cap; ++m) {
      const int2 tk = tl[qq.shard + 8 * m];
      const int pos = uni(tk.x), c = uni(tk.y);
      const int rd = uni(a.chain_read[c]);
      const int64_t qoff = uni64(b.seq_off[rd]);
      const int lq = uni((int)(b.seq_off[rd + 1] - qoff));
      const bwagpu_seed_t s = uni_seed(a.prog[pos]);
      ChainWin cw = a.win[c];
      cw.lo = uni64(cw.lo);
      cw.hi = uni64(cw.hi);
      const SeedExt e = extend_seed<C>(o, ref, s, lq, b.seq + qoff, cw, tbl, tbr);
      store_ext(a.ext + pos, e);
      spec_cells += e.cells;
    }
  }
  if ((threadIdx.x & 63) == 0 && spec_cells)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), (unsigned long long)spec_cells);
}

// ---------------------------------------------------- two seeds per wave
// The same extension tasks with one seed per 32-lane half (extend_pair).
// Everything below is per lane and uniform over a half; the halves diverge
// only through EXEC (a half without a left side, a retry or a task waits for
// the other).

// One half's task and the state of its extension, in LDS for the whole task:
// re-read (volatile, LDS address space) around every call, so that none of it
// occupies VGPRs across the DP loop.
struct PairCtx {
  int64_t rbeg, lo, hi, qoff;  // the seed, its chain's window, its read
  int32_t qbeg, len, lq, phase;
  int64_t rb, re;              // the region so far
  int32_t score, truesc, qb, qe, sc0, aw0, aw1, cells, rows, calls, pad_[2];
};
static_assert(sizeof(PairCtx) == 112, "PairCtx layout");
typedef volatile __attribute__((address_space(3))) PairCtx LdsCtx;

// extend_seed (bwamem.c:717-792) for the half's seed, as a state machine with
// ONE extend_pair call site: phase 0/1 = left side try 0/1 (MAX_BAND_TRY,
// bwamem.c:639), 2/3 = right side, 4 = done; a half whose phases are over
// leaves the loop (EXEC) while the other finishes.
template <int PMAX>
__device__ __forceinline__ SeedExt extend_seed2(const DevOpt& o, const DevRef& ref, LdsCtx* cx, const uint8_t* seq,
                                                uint8_t* tbl, uint8_t* tbr) {
  {
    const int64_t rbeg = cx->rbeg, lo = cx->lo, hi = cx->hi;
    const int qbeg = cx->qbeg, len = cx->len, lq = cx->lq;
    const int qlenL = qbeg, qlenR = lq - (qbeg + len);
    const int64_t x0R = rbeg + len;
    fill_two_half(tbl, rbeg - 1, qlenL ? rows_needed(o, qlenL, (int)(rbeg - lo), o.w << 1, o.pen_clip5) : 0, tbr, x0R,
                  qlenR ? rows_needed(o, qlenR, (int)(hi - x0R), o.w << 1, o.pen_clip3) : 0, ref);
    cx->phase = qbeg != 0 ? 0 : (qlenR != 0 ? 2 : 4);
    const int sc = qbeg != 0 ? -1 : len * o.a;  // bwamem.c:753
    cx->score = sc;
    cx->truesc = sc;
    cx->qb = 0;
    cx->qe = lq;
    cx->sc0 = 0;
    cx->aw0 = o.w;
    cx->aw1 = o.w;
    cx->rb = rbeg;
    cx->re = rbeg + len;
    cx->cells = 0;
    cx->rows = 0;
    cx->calls = 0;
  }
  for (;;) {
    const int phase = cx->phase;
    if (phase >= 4) break;
    const int64_t rbeg = cx->rbeg;
    const int qbeg = cx->qbeg, len = cx->len, lq = cx->lq;
    const bool left = phase < 2;
    const int t = phase & 1;
    const int qlenR = lq - (qbeg + len);
    const int qlen = left ? qbeg : qlenR;
    const int64_t x0 = left ? rbeg - 1 : rbeg + len;
    const int tlen = left ? (int)(rbeg - cx->lo) : (int)(cx->hi - x0);
    const int qa = left ? qbeg - 1 : qbeg + len;
    const int eb = left ? o.pen_clip5 : o.pen_clip3;
    if (t == 0) cx->sc0 = cx->score;
    const int h0 = left ? len * o.a : cx->sc0;
    const int aw = o.w << t;
    if (left) cx->aw0 = aw;
    else cx->aw1 = aw;
    Tally32 tl{0, 0, 0};
    const ExtOut x = extend_pair_dispatch<PMAX>(o, qlen, seq + cx->qoff, qa, left ? -1 : 1, tlen, left ? tbl : tbr, aw,
                                             eb, o.zdrop, h0, tl);
    cx->cells = cx->cells + tl.cells;
    cx->rows = cx->rows + tl.rows;
    cx->calls = cx->calls + tl.calls;
    const int prev = cx->score;
    const int score = x.score;
    cx->score = score;
    if (t == 0 && !(score == prev || x.max_off < (aw >> 1) + (aw >> 2))) {
      cx->phase = phase + 1;  // the band retry
      continue;
    }
    const bool local = x.gscore <= 0 || x.gscore <= score - eb;
    if (left) {
      cx->qb = local ? qbeg - x.qle : 0;
      cx->rb = rbeg - (local ? x.tle : x.gtle);
      cx->truesc = local ? score : x.gscore;
      cx->phase = qlenR != 0 ? 2 : 4;
    } else {
      cx->qe = local ? qa + x.qle : lq;
      cx->re = x0 + (local ? x.tle : x.gtle);
      cx->truesc = cx->truesc + (local ? score : x.gscore) - cx->sc0;
      cx->phase = 4;
    }
  }
  SeedExt e;
  e.rb = cx->rb;
  e.re = cx->re;
  e.qb = cx->qb;
  e.qe = cx->qe;
  e.score = cx->score;
  e.truesc = cx->truesc;
  const int aw0 = cx->aw0, aw1 = cx->aw1;
  e.w = aw0 > aw1 ? aw0 : aw1;
  e.cells = cx->cells;
  e.rows = cx->rows;
  e.calls = cx->calls + 1;  // + 1: a computed slot is never all-zero
  return e;
}

// Extension tasks of one list, two per wave: a wave claims two consecutive
// entries of a shard (one atomic), lanes 0-31 take the first, 32-63 the second.
// PMAX = the bin's largest CPL: ceil(read length / 32) (qlen + 1 <= read length)
template <int PMAX>
__global__ void __launch_bounds__(kBlock) spec_ext2_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int list,
                                                           int tb_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int hf = (int)(threadIdx.x >> 5) & 1;
  // per half: left rows, right rows, the task context
  uint8_t* const tbl = lds + (size_t)(threadIdx.x >> 5) * (2 * tb_bytes + sizeof(PairCtx));
  uint8_t* const tbr = tbl + tb_bytes;
  LdsCtx* const cx = (LdsCtx*)(tbr + tb_bytes);
  const int n = uni(__hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const int2* tl = a.stasks + spec_list_off(list, b.n_chains, b.n_seeds);  // in pair order (spec_sort_*)
  ShardQ qq;
  qq.init(a.qh + 8 * kQHStride * list, n);
  long long spec_cells = 0;
  int m0, cap;
  while (qq.claim(2, m0, cap)) {
    const int m = m0 + hf;
    if (m < cap) {
      const int2 tk = tl[qq.shard + 8 * m];
      const int pos = tk.x, c = tk.y;
      if ((threadIdx.x & 31) == 0) {
        const int rd = a.chain_read[c];
        const bwagpu_seed_t s = a.prog[pos];
        const ChainWin cw = a.win[c];
        const int64_t qoff = b.seq_off[rd];
        cx->rbeg = s.rbeg;
        cx->lo = cw.lo;
        cx->hi = cw.hi;
        cx->qoff = qoff;
        cx->qbeg = s.qbeg;
        cx->len = s.len;
        cx->lq = (int)(b.seq_off[rd + 1] - qoff);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const SeedExt e = extend_seed2<PMAX>(o, ref, cx, b.seq, tbl, tbr);
      store_ext_half(a.ext + pos, e);
      spec_cells += e.cells;
    }
  }
  if ((threadIdx.x & 31) == 0 && spec_cells)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), (unsigned long long)spec_cells);
}

// LDS bytes of a spec_ext2_kernel workgroup
static size_t ext2_lds(int tb_bytes) { return (size_t)(kBlock / 32) * (2 * (size_t)tb_bytes + sizeof(PairCtx)); }

// ---------------------------------------------------- four seeds per wave
// The same extension tasks with two seeds per 32-lane half, packed in the
// 16-bit halves of the DP registers (extend_quad).  Each sub-slot (half x
// low/high) walks its own seed through extend_seed's state machine
// (bwamem.c:717-792: left side with the band retry, right side from the left
// score, local vs to-end), held in registers; the four sub-slots call
// extend_quad together, and a sub-slot whose seed is done takes the next task
// of the list at once (one claim per call boundary for all the sub-slots that
// need one), so a wave idles only inside a call whose four rows counts differ.
struct QTask {
  int64_t rbeg, wlo, whi, qoff, rb, re;
  int pos, qbeg, len, lq, phase, score, truesc, qb, qe, sc0, aw0, aw1, cells, rows, calls;
};

// the task's seed, window and read; both target windows into the sub-slot's LDS rows
template <int G>
__device__ __forceinline__ void qtask_start(QTask& t, const DevOpt& o, const DevRef& ref, const DevBatch& b,
                                            const SpecArgs& a, int2 tk, uint8_t* tl, uint8_t* tr) {
  const int rd = a.chain_read[tk.y];
  const bwagpu_seed_t s = a.prog[tk.x];
  const ChainWin cw = a.win[tk.y];
  t.pos = tk.x;
  t.rbeg = s.rbeg;
  t.wlo = cw.lo;
  t.whi = cw.hi;
  t.qoff = b.seq_off[rd];
  t.lq = (int)(b.seq_off[rd + 1] - t.qoff);
  t.qbeg = s.qbeg;
  t.len = s.len;
  const int qlenL = t.qbeg, qlenR = t.lq - (t.qbeg + t.len);
  const int64_t x0R = t.rbeg + t.len;
  fill_two_half<G>(tl, t.rbeg - 1, qlenL ? rows_needed(o, qlenL, (int)(t.rbeg - t.wlo), o.w << 1, o.pen_clip5) : 0, tr,
                x0R, qlenR ? rows_needed(o, qlenR, (int)(t.whi - x0R), o.w << 1, o.pen_clip3) : 0, ref);
  t.phase = qlenL != 0 ? 0 : (qlenR != 0 ? 2 : 4);
  const int sc = qlenL != 0 ? -1 : t.len * o.a;  // bwamem.c:753
  t.score = sc;
  t.truesc = sc;
  t.qb = 0;
  t.qe = t.lq;
  t.sc0 = 0;
  t.aw0 = o.w;
  t.aw1 = o.w;
  t.rb = t.rbeg;
  t.re = t.rbeg + t.len;
  t.cells = t.rows = t.calls = 0;
}

// the same from the task's FatTask record (spec_sort_scatter)
template <int G>
__device__ __forceinline__ void qtask_start_fat(QTask& t, const DevOpt& o, const DevRef& ref, const FatTask& f,
                                                uint8_t* tl, uint8_t* tr) {
  t.pos = f.pos;
  t.rbeg = f.rbeg;
  t.wlo = f.rbeg - f.dlo;
  t.whi = f.rbeg + f.dhi;
  t.qoff = f.qoff;
  t.qbeg = (int)(f.qls & 1023u);
  t.len = (int)((f.qls >> 10) & 1023u);
  t.lq = (int)(f.qls >> 20);
  const int qlenL = t.qbeg, qlenR = t.lq - (t.qbeg + t.len);
  const int64_t x0R = t.rbeg + t.len;
  fill_two_fast<G>(tl, t.rbeg - 1, qlenL ? rows_needed(o, qlenL, f.dlo, o.w << 1, o.pen_clip5) : 0, tr, x0R,
                   qlenR ? rows_needed(o, qlenR, (int)(t.whi - x0R), o.w << 1, o.pen_clip3) : 0, ref);
  t.phase = qlenL != 0 ? 0 : (qlenR != 0 ? 2 : 4);
  const int sc = qlenL != 0 ? -1 : t.len * o.a;  // bwamem.c:753
  t.score = sc;
  t.truesc = sc;
  t.qb = 0;
  t.qe = t.lq;
  t.sc0 = 0;
  t.aw0 = o.w;
  t.aw1 = o.w;
  t.rb = t.rbeg;
  t.re = t.rbeg + t.len;
  t.cells = t.rows = t.calls = 0;
}

// the ksw_extend2 call of the task's phase (0/1: left try 0/1, 2/3: right)
__device__ __forceinline__ QCall qtask_call(QTask& t, const DevOpt& o, const uint8_t* seq, const uint8_t* tl,
                                            const uint8_t* tr) {
  const bool left = t.phase < 2;
  const int tt = t.phase & 1;
  const int qlenR = t.lq - (t.qbeg + t.len);
  const int64_t x0 = left ? t.rbeg - 1 : t.rbeg + t.len;
  QCall q;
  q.qlen = left ? t.qbeg : qlenR;
  q.tlen = left ? (int)(t.rbeg - t.wlo) : (int)(t.whi - x0);
  q.qa = left ? t.qbeg - 1 : t.qbeg + t.len;
  q.qd = left ? -1 : 1;
  q.eb = left ? o.pen_clip5 : o.pen_clip3;
  if (tt == 0) t.sc0 = t.score;
  q.h0 = left ? t.len * o.a : t.sc0;
  q.w = o.w << tt;
  if (left) t.aw0 = q.w;
  else t.aw1 = q.w;
  q.zdrop = o.zdrop;
  q.q = seq + t.qoff;
  q.tb = left ? tl : tr;
  // rows past qlen + w + 1 have an empty band (ksw.c:415-419: m == 0 breaks
  // there), so the cap changes no result; it keeps tlen inside the packed
  // kernels' 16-bit row counters for chain windows of 32 kb and more
  q.tlen = rows_needed(o, q.qlen, q.tlen, q.w, q.eb);
  return q;
}

// the call's result into the task (bwamem.c:737-792); true = the seed is done
__device__ __forceinline__ bool qtask_advance(QTask& t, const DevOpt& o, const ExtOut& x, const Tally32& tl) {
  const bool left = t.phase < 2;
  const int tt = t.phase & 1;
  t.cells += tl.cells;
  t.rows += tl.rows;
  t.calls += tl.calls;
  const int prev = t.score;
  t.score = x.score;
  const int aw = o.w << tt;
  if (tt == 0 && !(x.score == prev || x.max_off < (aw >> 1) + (aw >> 2))) {  // the band retry (MAX_BAND_TRY)
    t.phase += 1;
    return false;
  }
  const int eb = left ? o.pen_clip5 : o.pen_clip3;
  const bool local = x.gscore <= 0 || x.gscore <= x.score - eb;
  if (left) {
    t.qb = local ? t.qbeg - x.qle : 0;
    t.rb = t.rbeg - (local ? x.tle : x.gtle);
    t.truesc = local ? x.score : x.gscore;
    t.phase = t.lq - (t.qbeg + t.len) != 0 ? 2 : 4;
  } else {
    t.qe = local ? t.qbeg + t.len + x.qle : t.lq;
    t.re = t.rbeg + t.len + (local ? x.tle : x.gtle);
    t.truesc += (local ? x.score : x.gscore) - t.sc0;
    t.phase = 4;
  }
  return t.phase >= 4;
}

__device__ __forceinline__ SeedExt qtask_ext(const QTask& t) {
  SeedExt e;
  e.rb = t.rb;
  e.re = t.re;
  e.qb = t.qb;
  e.qe = t.qe;
  e.score = t.score;
  e.truesc = t.truesc;
  e.w = t.aw0 > t.aw1 ? t.aw0 : t.aw1;
  e.cells = t.cells;
  e.rows = t.rows;
  e.calls = t.calls + 1;  // + 1: a computed slot is never all-zero
  return e;
}

// The sub-slots' task states wait in LDS while a call runs (loaded before and
// stored after it): kept in registers across extend_quad they cost ~50 VGPRs,
// which at 2 waves per SIMD left the other caller stream's selection kernels
// no room on the SIMD.
static_assert(sizeof(QTask) <= 112, "QTask layout");
constexpr int kQTaskLds = 112;
// Not volatile: a volatile access makes the memory legalizer wait for every
// outstanding global access first (s_waitcnt vmcnt(0) at each qload / qpark:
// the SeedExt stores and the task loads of the other sub-slots, ~30 % of the
// waves' cycles outside the DP in the diagnostic build's clock split).  An
// empty asm with a memory clobber after the stores and before the loads keeps
// the state really parked in LDS (LLVM may not carry it in VGPRs across it).
typedef __attribute__((address_space(3))) QTask LdsQ;
__device__ __forceinline__ void qpark(LdsQ* p, const QTask& t) {
  p->rbeg = t.rbeg;
  p->wlo = t.wlo;
  p->whi = t.whi;
  p->qoff = t.qoff;
  p->rb = t.rb;
  p->re = t.re;
  p->pos = t.pos;
  p->qbeg = t.qbeg;
  p->len = t.len;
  p->lq = t.lq;
  p->phase = t.phase;
  p->score = t.score;
  p->truesc = t.truesc;
  p->qb = t.qb;
  p->qe = t.qe;
  p->sc0 = t.sc0;
  p->aw0 = t.aw0;
  p->aw1 = t.aw1;
  p->cells = t.cells;
  p->rows = t.rows;
  p->calls = t.calls;
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ QTask qload(LdsQ* p) {
  asm volatile("" ::: "memory");
  QTask t;
  t.rbeg = p->rbeg;
  t.wlo = p->wlo;
  t.whi = p->whi;
  t.qoff = p->qoff;
  t.rb = p->rb;
  t.re = p->re;
  t.pos = p->pos;
  t.qbeg = p->qbeg;
  t.len = p->len;
  t.lq = p->lq;
  t.phase = p->phase;
  t.score = p->score;
  t.truesc = p->truesc;
  t.qb = p->qb;
  t.qe = p->qe;
  t.sc0 = p->sc0;
  t.aw0 = p->aw0;
  t.aw1 = p->aw1;
  t.cells = p->cells;
  t.rows = p->rows;
  t.calls = p->calls;
  return t;
}

// Extension tasks of one list (in pair order, spec_sort_*), two per G-lane
// group: four (G = 32) or eight (G = 16) per wave.
// PMAX = the bin's largest CPL: ceil(read length / G).
// Every sub-slot keeps its NEXT task's FatTask record in registers, claimed and
// loaded one generation ahead: the loads run while the current generation's
// DP runs (the row loop has no global memory operation), so a sub-slot whose
// task ends starts the next at once — only its target rows (fill_two_half)
// are fetched at the call boundary.  At one wave per SIMD nothing else hides a
// generation start's dependent loads (the claim, the task entry, its seed,
// window and read).
template <int G, int PMAX, bool K8>
__global__ void __launch_bounds__(kBlock) spec_ext4_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int list,
                                                           int tb_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  // the groups' first lanes, and those below this lane's group
  constexpr uint64_t kLead = G == 16 ? 0x0001000100010001ull : 0x0000000100000001ull;
  const uint64_t below = kLead & ((1ull << ((int)threadIdx.x & (64 - G))) - 1);
  // per group: A left, A right, B left, B right target rows, then A's and B's task states
  uint8_t* const tal = lds + (size_t)(threadIdx.x / G) * (4 * (size_t)tb_bytes + 2 * kQTaskLds);
  uint8_t* const tar = tal + tb_bytes;
  uint8_t* const tbl = tar + tb_bytes;
  uint8_t* const tbr = tbl + tb_bytes;
  LdsQ* const qa = (LdsQ*)(tbr + tb_bytes);
  LdsQ* const qb = (LdsQ*)(tbr + tb_bytes + kQTaskLds);
  const int n = uni(__hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const FatTask* fl = a.ftask + spec_list_off(list, b.n_chains, b.n_seeds);
  ShardQ qq;
  qq.init(a.qh + 8 * kQHStride * list, n);
  // ha / hb: the sub-slot has a task (state parked in LDS); pa / pb: its next
  // task's record (fa / fb) is claimed and loaded (or in flight)
  bool ha = false, hb = false, pa = false, pb = false, more = n > 0;
  FatTask fa{}, fb{};
  long long spec_cells = 0;
  // claim-ahead while plenty of the list is left (a.ext_prefetch): near the
  // end, tasks held ahead by a busy wave would idle the others
  const int ahead_min = a.ext_prefetch * 8 * (int)((gridDim.x * (kBlock / 64) + 7) / 8);
  int rem = n;
#ifdef BWAGPU_OCC_DIAG
  unsigned long long tw[6] = {0, 0, 0, 0, 0, 0}, occ[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  for (;;) {
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
    // sub-slots without a task start their prefetched one
    if (!ha && pa) {
      QTask t;
      qtask_start_fat<G>(t, o, ref, fa, tal, tar);
      if (t.phase >= 4) store_ext_half<G>(a.ext + t.pos, qtask_ext(t));  // a whole-read seed (bwamem.c:753, 781)
      else qpark(qa, t);
      ha = t.phase < 4;
      pa = false;
    }
    if (!hb && pb) {
      QTask t;
      qtask_start_fat<G>(t, o, ref, fb, tbl, tbr);
      if (t.phase >= 4) store_ext_half<G>(a.ext + t.pos, qtask_ext(t));
      else qpark(qb, t);
      hb = t.phase < 4;
      pb = false;
    }
    if (more) {  // one claim for the wave: sub-slots without a next task (ahead) / without a task (on demand)
      const bool ahead = ahead_min > 0 && rem > ahead_min;
      const bool wa = ahead ? !pa : (!ha && !pa), wb = ahead ? !pb : (!hb && !pb);
      const uint64_t na = __builtin_amdgcn_ballot_w64(wa) & kLead, nb = __builtin_amdgcn_ballot_w64(wb) & kLead;
      const int nn = __popcll(na) + __popcll(nb);
      if (nn > 0) {
        int m0, cap;
#ifdef BWAGPU_OCC_DIAG
        const unsigned long long ca0 = __builtin_amdgcn_s_memtime();
#endif
        const bool got = qq.claim(nn, m0, cap);
#ifdef BWAGPU_OCC_DIAG
        const unsigned long long ca1 = __builtin_amdgcn_s_memtime();
        tw[4] += ca1 - ca0;
#endif
        if (got) {
          rem = (cap - m0 - nn) * 8;
          const int ia = m0 + __popcll(na & below) + __popcll(nb & below), ib = ia + (wa ? 1 : 0);
          if (wa && ia < cap) {
            fa = fl[qq.shard + 8 * ia];
            pa = true;
          }
          if (wb && ib < cap) {
            fb = fl[qq.shard + 8 * ib];
            pb = true;
          }
#ifdef BWAGPU_OCC_DIAG
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the task records, timed on their own
          tw[5] += __builtin_amdgcn_s_memtime() - ca1;
#endif
          if (!ahead) {  // on demand: start them now
            if (!ha && pa) {
              QTask t;
              qtask_start_fat<G>(t, o, ref, fa, tal, tar);
              if (t.phase >= 4) store_ext_half<G>(a.ext + t.pos, qtask_ext(t));
              else qpark(qa, t);
              ha = t.phase < 4;
              pa = false;
            }
            if (!hb && pb) {
              QTask t;
              qtask_start_fat<G>(t, o, ref, fb, tbl, tbr);
              if (t.phase >= 4) store_ext_half<G>(a.ext + t.pos, qtask_ext(t));
              else qpark(qb, t);
              hb = t.phase < 4;
              pb = false;
            }
          }
        } else {
          more = false;
        }
      }
    }
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    tw[0] += c1 - c0;
#endif
    if (!__builtin_amdgcn_ballot_w64(ha || hb)) {
      if (!more && !__builtin_amdgcn_ballot_w64(pa || pb)) break;
      continue;
    }
    QCall ca = quad_idle(b.seq, tal), cb = quad_idle(b.seq, tbl);
    if (ha) {
      QTask t = qload(qa);
      ca = qtask_call(t, o, b.seq, tal, tar);
      qpark(qa, t);
    }
    if (hb) {
      QTask t = qload(qb);
      cb = qtask_call(t, o, b.seq, tbl, tbr);
      qpark(qb, t);
    }
    ExtOut xa, xb;
    Tally32 ta{0, 0, 0}, tb{0, 0, 0};
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c2 = __builtin_amdgcn_s_memtime();
    tw[1] += c2 - c1;
#endif
    extend_quad_dispatch<G, PMAX, K8>(o, ca, cb, xa, xb, ta, tb);
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c3 = __builtin_amdgcn_s_memtime();
    tw[2] += c3 - c2;
    occ_diag<G>(occ, ca, cb, ta, tb);
#endif
    if (ha) {
      QTask t = qload(qa);
      if (qtask_advance(t, o, xa, ta)) {
        store_ext_half<G>(a.ext + t.pos, qtask_ext(t));
        spec_cells += t.cells;
        ha = false;
      } else {
        qpark(qa, t);
      }
    }
    if (hb) {
      QTask t = qload(qb);
      if (qtask_advance(t, o, xb, tb)) {
        store_ext_half<G>(a.ext + t.pos, qtask_ext(t));
        spec_cells += t.cells;
        hb = false;
      } else {
        qpark(qb, t);
      }
    }
#ifdef BWAGPU_OCC_DIAG
    tw[3] += __builtin_amdgcn_s_memtime() - c3;
#endif
  }
  if ((threadIdx.x & (G - 1)) == 0 && spec_cells)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), (unsigned long long)spec_cells);
#ifdef BWAGPU_OCC_DIAG
  // shader-clock cycles of the waves: task starts + claims, call setup, DP (extend_quad), result
  // advance; of the first, the claims' and the task records' own
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 8; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + 32) + k, occ[k]);
    for (int k = 0; k < 6; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + 48) + k, tw[k]);
  }
#endif
}

// LDS bytes of a spec_ext4_kernel workgroup
static size_t ext4_lds(int tb_bytes, int g) { return (size_t)(kBlock / g) * (4 * (size_t)tb_bytes + 2 * kQTaskLds); }

// Task order for the pair kernel: the two seeds a wave takes should need the
// same phases for about as long — a half whose seed has no left side, or a
// much shorter one, idles while the other runs (EXEC).  A counting sort of
// the first two bins' lists of a round by key = (the longer side's qlen / 8,
// the shorter's / 8) — with calls of left and right phases mixed in one row
// loop, the longer side sets the columns run (by (left, right): 37.8 against
// 38.1-38.2 Mreads/s with eight per wave):
// count (per-block LDS histograms, one global atomic per block and key),
// scan (one block per list), scatter (per-block LDS ranks, one global atomic
// per block and key to reserve the block's range).  Claims then take entries
// 8 apart in the sorted list (the sharded queue), which have about the same
// key.  The order changes nothing but which seeds share a wave.
__device__ __forceinline__ int pair_key(const DevBatch& b, const SpecArgs& a, int2 tk) {
  const bwagpu_seed_t s = a.prog[tk.x];
  const int rd = a.chain_read[tk.y];
  const int lq = (int)(b.seq_off[rd + 1] - b.seq_off[rd]);
  const int ql = min(s.qbeg, 255), qr = min(max(lq - s.qbeg - s.len, 0), 255);
  // descending: the longest tasks first, so the grid's tail is short ones
  const int hi = max(ql, qr), lo = min(ql, qr);
  return (kSortKeys - 1) - ((hi >> 3) << 5 | (lo >> 3));
}

__global__ void __launch_bounds__(256) spec_sort_count(DevBatch b, SpecArgs a, int round, int bin0) {
  sel_prio();
  __shared__ int hist[kSortKeys];
  const int bin = bin0 + (int)blockIdx.y;
  const int list = round * kSpecBins + bin;
  int32_t* gh = a.sorth + (round * 2 + bin) * kSortKeys;
  for (int k = threadIdx.x; k < kSortKeys; k += 256) hist[k] = 0;
  __syncthreads();
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int2* tl = a.tasks + spec_list_off(list, b.n_chains, b.n_seeds);
  const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) atomicAdd(&hist[pair_key(b, a, tl[i])], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < kSortKeys; k += 256)
    if (hist[k]) atomicAdd(&gh[k], hist[k]);
}

__global__ void __launch_bounds__(256) spec_sort_scan(SpecArgs a, int round, int bin0) {
  sel_prio();
  __shared__ int part[256];
  int32_t* gh = a.sorth + (round * 2 + bin0 + (int)blockIdx.x) * kSortKeys;
  const int t = (int)threadIdx.x;  // 4 keys per thread
  int v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = gh[4 * t + k];
    s += v[k];
  }
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the per-thread sums
    const int x = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int base = part[t] - s;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    gh[4 * t + k] = base;  // the key's first position (a cursor from here on)
    base += v[k];
  }
}

__global__ void __launch_bounds__(256) spec_sort_scatter(DevBatch b, SpecArgs a, int round, int bin0) {
  sel_prio();
  __shared__ int cnt[kSortKeys];
  const int bin = bin0 + (int)blockIdx.y;
  const int list = round * kSpecBins + bin;
  int32_t* gh = a.sorth + (round * 2 + bin) * kSortKeys;
  for (int k = threadIdx.x; k < kSortKeys; k += 256) cnt[k] = 0;
  __syncthreads();
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t off = spec_list_off(list, b.n_chains, b.n_seeds);
  const int2* tl = a.tasks + off;
  int2* out = a.stasks + off;
  FatTask* fout = a.ftask + off;
  const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  constexpr int kPer = 16;  // entries per thread held across the barrier
  int keys[kPer], rank[kPer];
  int2 tk[kPer];
  for (int base = i0; base < i1; base += 256 * kPer) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int i = base + m * 256 + (int)threadIdx.x;
      keys[m] = -1;
      if (i < i1) {
        tk[m] = tl[i];
        keys[m] = pair_key(b, a, tk[m]);
        rank[m] = atomicAdd(&cnt[keys[m]], 1);
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kSortKeys; k += 256) {
      const int c = cnt[k];
      cnt[k] = c ? atomicAdd(&gh[k], c) : 0;  // this pass's range of key k
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kPer; ++m)
      if (keys[m] >= 0) {
        const int at = cnt[keys[m]] + rank[m];
        out[at] = tk[m];
        fout[at] = fat_task(b, a, tk[m]);
      }
    __syncthreads();
    for (int k = threadIdx.x; k < kSortKeys; k += 256) cnt[k] = 0;
    __syncthreads();
  }
}


// a bin's list in pair order (the task kernels EXT2 / EXT4)
static void launch_task_sort(const ExtRound& r, int bin0, int nbins) {
  hipLaunchKernelGGL(spec_sort_count, dim3(256, nbins), dim3(256), 0, r.st, r.b, r.a, r.round, bin0);
  hipLaunchKernelGGL(spec_sort_scan, dim3(nbins), dim3(256), 0, r.st, r.a, r.round, bin0);
  hipLaunchKernelGGL(spec_sort_scatter, dim3(256, nbins), dim3(256), 0, r.st, r.b, r.a, r.round, bin0);
}

// one launch of a task kernel (EXT2 / EXT4) for one list
template <class K>
static void launch_task(K kernel, size_t lds, const ExtRound& r, int list, bool quad) {
  const int nb = resident_blocks(kernel, lds);
  const int gr = r.round == 2 ? std::min(nb, 64) : ext2_grid(nb, quad);
  hipLaunchKernelGGL(kernel, dim3(gr), dim3(kBlock), lds, r.st, r.o, r.ref, r.b, r.a, list, r.tb_bytes);
}

// the task kernels compiled are exactly these cases
static void launch_task_bin(const ExtBin& k, const ExtRound& r, int list, bool quad) {
  const int tb = r.tb_bytes;
  switch (ext_key(k.family, k.G, k.PMAX, k.K8)) {
    // eight per wave, the row-max key widened per call (H may reach 256 and more)
    case ext_key(EXT4, 16, 16, false): return launch_task(spec_ext4_kernel<16, 16, false>, ext4_lds(tb, 16), r, list, quad);
    case ext_key(EXT4, 32, 8, false): return launch_task(spec_ext4_kernel<32, 8, false>, ext4_lds(tb, 32), r, list, quad);
    case ext_key(EXT2, 32, 5, false): return launch_task(spec_ext2_kernel<5>, ext2_lds(tb), r, list, quad);
    case ext_key(EXT2, 32, 8, false): return launch_task(spec_ext2_kernel<8>, ext2_lds(tb), r, list, quad);
    default: abort();  // ext_plan names no other task kernel (tests/cpp/ext_plan_asan.cpp)
  }
}

// the third bin: spec_ext_kernel<16>
static void launch_task_long(const ExtRound& r, int list) {
  const size_t lds = (size_t)(kBlock / 64) * 2 * r.tb_bytes;
  const int nb = resident_blocks(spec_ext_kernel<16>, lds);
  hipLaunchKernelGGL(spec_ext_kernel<16>, dim3(r.round == 2 ? std::min(nb, 64) : nb), dim3(kBlock), lds, r.st, r.o, r.ref,
                     r.b, r.a, list, r.tb_bytes);
}

// The pair kernel's grid: its waves pull tasks from the queue, so the grid
// only sets its occupancy.  2 workgroups per CU (8 waves per CU, 2 per SIMD)
// instead of the resident capacity (5 per SIMD): the batch on the other caller
// stream (the bench's ping-pong) and this batch's selection kernels keep the
// rest, and an even count per CU beats an uneven one.  Same-box sweep
// (DESIGN.md §3): capacity 19.87, 60 % 20.74, 50 % 20.66, 2/CU (40 %) 21.74,
// 30 % 20.16, 1/CU 19.72 Mreads/s.  The packed kernels (two 209 / 198-VGPR
// waves per SIMD at 2/CU) run at 1 workgroup per CU: 37.97-38.04 against
// 36.99-37.17 Mreads/s on C2, C3 0.66 against 0.78-0.79 ms per batch (same
// box).  BWAGPU_EXT2_BLOCKS_PER_CU overrides both.
int ext2_grid(int nb, bool packed) {
  static const int env_cu = [] {
    const char* e = getenv("BWAGPU_EXT2_BLOCKS_PER_CU");
    const int v = e ? atoi(e) : 0;
    return v < 0 ? 0 : v;
  }();
  const int per_cu = env_cu ? env_cu : (packed ? 1 : 2);
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      ncu <= 0)
    return nb;
  return std::max(1, std::min(nb, per_cu * ncu));
}


// The sequential logic of mem_chain2aln over one read's chains, by one wave.
// A seed that is extended but has no result yet:
//   SEL_EMULATE  becomes a round-B task (its region stays unknown in this pass);
//   SEL_FINAL    is listed (the round-C list, a diagnostic count) and the read goes to the redo list
//                (its later decisions depend on that region);
//   SEL_REDO     (the redo list only) is computed inline — the pass that
//                guarantees every read completes.
// SEL_FINAL and SEL_REDO write the read's mem_alnreg_v.
// Two shapes: LIGHT reads (<= kSelLight seeds, so every chain and the region
// list fit one lane slot) four waves per workgroup, 2 KB of LDS each; HEAVY
// reads one wave per workgroup with up to 64 KB of LDS region records (beyond
// that: the region's seed slot in regpos[] and its SeedExt, re-read with
// workgroup-scope atomics), chains of <= 256 seeds in four VGPR slots (longer:
// prog[] and skip flags in skipf[]).  The two shapes run concurrently on two
// streams.
enum { SEL_EMULATE = 0, SEL_FINAL = 1, SEL_REDO = 2 };
struct RegRec {  // a region's containment fields (bwamem.c:682-696)
  int64_t rb, re;
  int32_t qb, qe, w, seedlen0;
};
constexpr int kSelHeavyLds = 64 * 1024;
constexpr int kSelExtCache = 256;  // a heavy chain's SeedExt records staged in LDS
__host__ __device__ constexpr int sel_light_wave_lds() { return kSelLight * (int)sizeof(RegRec); }
__host__ __device__ constexpr int sel_heavy_cap(int mode, int tb) {
  return (kSelHeavyLds - 4 * (BWAGPU_MAX_READ_LEN + 1) - kSelExtCache * (int)(sizeof(SeedExt) + sizeof(bwagpu_seed_t)) -
          (mode == SEL_REDO ? 2 * tb : 0)) / (int)sizeof(RegRec);
}

// max_gap_len (cal_max_gap, bwamem.c:630-637) of every length a containment
// test can ask for (min(qd, rd) of a region holding the seed: 0..lq-1),
// tabulated in LDS per workgroup instead of two divisions per lane and region
constexpr int kMglN = BWAGPU_MAX_READ_LEN + 1;

// near(s, p): the two gap tests of bwamem.c:688-696 for a region p that holds s
__device__ __forceinline__ bool seed_near(const int32_t* MG, const bwagpu_seed_t& s, const RegRec& p) {
  const int qd1 = s.qbeg - p.qb;
  const int64_t rd1 = s.rbeg - p.rb;
  const int g1 = MG[min(max(qd1 < rd1 ? qd1 : (int)rd1, 0), kMglN - 1)];
  const int bw1 = g1 < p.w ? g1 : p.w;
  const int qd2 = p.qe - (s.qbeg + s.len);
  const int64_t rd2 = p.re - (s.rbeg + s.len);
  const int g2 = MG[min(max(qd2 < rd2 ? qd2 : (int)rd2, 0), kMglN - 1)];
  const int bw2 = g2 < p.w ? g2 : p.w;
  return (qd1 - rd1 < bw1 && rd1 - qd1 < bw1) || (qd2 - rd2 < bw2 && rd2 - qd2 < bw2);
}

// the 88-byte mem_alnreg_t (rest zero: bwamem.c:718); lane d writes dword d
__device__ __forceinline__ void write_region(bwagpu_alnreg_t* dst, const SeedExt& e, int rid, int cov, int slen,
                                             float frac) {
  const int r = (int)(threadIdx.x & 63);
  const int dw = r < 21 ? r : 21;
  uint32_t v = 0;
  v = dw == 0 ? (uint32_t)e.rb : v;
  v = dw == 1 ? (uint32_t)((uint64_t)e.rb >> 32) : v;
  v = dw == 2 ? (uint32_t)e.re : v;
  v = dw == 3 ? (uint32_t)((uint64_t)e.re >> 32) : v;
  v = dw == 4 ? (uint32_t)e.qb : v;
  v = dw == 5 ? (uint32_t)e.qe : v;
  v = dw == 6 ? (uint32_t)rid : v;
  v = dw == 7 ? (uint32_t)e.score : v;
  v = dw == 8 ? (uint32_t)e.truesc : v;
  v = dw == 13 ? (uint32_t)e.w : v;
  v = dw == 14 ? (uint32_t)cov : v;
  v = dw == 17 ? (uint32_t)slen : v;
  v = dw == 19 ? __float_as_uint(frac) : v;
  reinterpret_cast<uint32_t*>(dst)[dw] = v;
}

// a region's containment record into LDS (lanes 0-7 one field each)
__device__ __forceinline__ void put_regrec(RegRec* dst, const SeedExt& e, int slen) {
  const int r = (int)(threadIdx.x & 63);
  const int f = r < 8 ? r : 7;
  int32_t v = 0;
  v = f == 0 ? (int32_t)(uint32_t)e.rb : v;
  v = f == 1 ? (int32_t)((uint64_t)e.rb >> 32) : v;
  v = f == 2 ? (int32_t)(uint32_t)e.re : v;
  v = f == 3 ? (int32_t)((uint64_t)e.re >> 32) : v;
  v = f == 4 ? e.qb : v;
  v = f == 5 ? e.qe : v;
  v = f == 6 ? e.w : v;
  v = f == 7 ? slen : v;
  if (r < 8) reinterpret_cast<int32_t*>(dst)[f] = v;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// diagnostics (bwagpu_debug_set_trace): per read and selection pass, 8 words
// at g_trace[(pass * n_reads + rd) * 8]: start / end s_memrealtime (100 MHz),
// seeds, regions, XCC id, shape (1 light, 2 heavy)
__device__ __forceinline__ void trace_read(int pass, int n_reads, int rd, uint64_t t0, int ns, int nreg, int shape) {
  uint32_t* const tr = g_trace;
  if (!tr) return;
  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  const int r = (int)(threadIdx.x & 63);
  const int d = r < 7 ? r : 7;
  uint32_t v = (uint32_t)shape;
  v = d == 0 ? (uint32_t)t0 : v;
  v = d == 1 ? (uint32_t)(t0 >> 32) : v;
  v = d == 2 ? (uint32_t)t1 : v;
  v = d == 3 ? (uint32_t)(t1 >> 32) : v;
  v = d == 4 ? (uint32_t)ns : v;
  v = d == 5 ? (uint32_t)nreg : v;
  v = d == 6 ? __builtin_amdgcn_s_getreg((31 << 11) | 20) : v;
  if (r < 8) tr[((size_t)pass * n_reads + rd) * 8 + d] = v;
}

// One heavy read `rd` by the whole wave, seed by seed: the reads without a
// pair matrix and the redo list.  lds: kSelHeavyLds bytes (+ the redo pass's
// target rows): max_gap_len table | chain seeds (pad_ = skip flag | 2 *
// pending) | their SeedExt records | region records | (redo) target rows.
// fill_mg: the table is not there yet (a caller that runs one read after another
// with nothing else in that LDS fills it once itself).  tl: the finished read's
// work, wave-uniform.
template <int MODE>
__device__ __forceinline__ void select_heavy_read(const DevOpt& o, const DevRef& ref, const DevBatch& b,
                                                  const SpecArgs& a, int rd, uint8_t* lds, int tb_bytes, bool fill_mg,
                                                  Tally& tl) {
  constexpr bool WRITE = MODE != SEL_EMULATE;
  const int r = (int)(threadIdx.x & 63);
  int32_t* const MG = reinterpret_cast<int32_t*>(lds);
  bwagpu_seed_t* const SC = reinterpret_cast<bwagpu_seed_t*>(lds + 4 * kMglN);
  SeedExt* const EC = reinterpret_cast<SeedExt*>(SC + kSelExtCache);
  RegRec* const R = reinterpret_cast<RegRec*>(EC + kSelExtCache);
  const int cap_reg = sel_heavy_cap(MODE, tb_bytes);
  uint8_t* const tbl = reinterpret_cast<uint8_t*>(R + cap_reg);
  uint8_t* const tbr = tbl + tb_bytes;
  if (fill_mg)
    for (int x = r; x < kMglN; x += 64) MG[x] = max_gap_len(o, x);
  const uint64_t t_start = g_trace ? __builtin_amdgcn_s_memrealtime() : 0;
  const ReadDesc d = uniform_desc(a.rdesc[rd]);
  if (d.lq > a.lq_bound) return;  // flagged by spec_reads_kernel
  const uint8_t* const q = b.seq + d.qoff;
  const int rep_lim = (int)floor(.1 * d.lq) + 1;  // s->len - p->seedlen0 > .1 * l_query, bwamem.c:685
  bool redo = false;
  Tally rt{0, 0, 0};
  int nreg = 0, n_inline = 0;
  for (int c = d.c0; c < d.c0 + d.nch && !redo; ++c) {
    const int s0 = uni(b.chain_seed_off[c]), ns = uni(b.chain_seed_off[c + 1]) - s0;
    if (ns == 0) continue;
    ChainWin cw = a.win[c];
    cw.lo = uni64(cw.lo);
    cw.hi = uni64(cw.hi);
    if (cw.hi < cw.lo) continue;  // flagged by spec_chain_kernel (the reference would assert)
    const int rid = uni(b.chain_rid[c]);
    const float frac = __int_as_float(uni(__float_as_int(b.chain_frac_rep[c])));
    // the chain's seeds (processing order) and their extension results, staged
    // in LDS (chains of more than kSelExtCache seeds: prog[] / ext[] / skipf[])
    const bool big = ns > kSelExtCache;
    for (int i = r; i < min(ns, kSelExtCache); i += 64) {
      bwagpu_seed_t v = a.prog[s0 + i];
      v.pad_ = v.pad_ != 0 ? 1 : 0;
      SC[i] = v;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.ext + s0 + i);
      uint32_t* dst = reinterpret_cast<uint32_t*>(EC + i);
#pragma unroll
      for (int w = 0; w < 12; ++w) dst[w] = __hip_atomic_load(src + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (big)
      for (int i = r; i < ns; i += 64)
        __hip_atomic_store(&a.skipf[s0 + i], a.prog[s0 + i].pad_ != 0 ? 1 : 0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    mem_fence_group();
    auto seed_at = [&](int i) -> bwagpu_seed_t { return i < kSelExtCache ? SC[i] : a.prog[s0 + i]; };
    auto flag_at = [&](int i) -> int {
      return i < kSelExtCache ? SC[i].pad_
                              : __hip_atomic_load(&a.skipf[s0 + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto set_flag = [&](int i, int f) {
      if (r == 0) {
        if (i < kSelExtCache) SC[i].pad_ |= f;
        else __hip_atomic_store(&a.skipf[s0 + i], f | 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      mem_fence_group();
    };
    for (int k = 0; k < ns; ++k) {
      const bwagpu_seed_t s = uni_seed(seed_at(k));
      // containment in a region so far (bwamem.c:678-697), one region per lane
      bool hit = false;
      for (int base = 0; base < nreg && !hit; base += 64) {
        const int i = min(base + r, nreg - 1);
        RegRec p;
        if (i < cap_reg) {
          p = R[i];
        } else {
          const int pp = __hip_atomic_load(&a.regpos[d.s0 + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          const SeedExt* pe = a.ext + pp;
          p.rb = __hip_atomic_load(&pe->rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          p.re = __hip_atomic_load(&pe->re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          p.qb = __hip_atomic_load(&pe->qb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          p.qe = __hip_atomic_load(&pe->qe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          p.w = __hip_atomic_load(&pe->w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          p.seedlen0 = a.prog[pp].len;
        }
        const bool inside = base + r < nreg &&
                            !(s.rbeg < p.rb || s.rbeg + s.len > p.re || s.qbeg < p.qb || s.qbeg + s.len > p.qe) &&
                            !(s.len - p.seedlen0 >= rep_lim);
        if (__builtin_amdgcn_ballot_w64(inside) == 0) continue;
        hit = __builtin_amdgcn_ballot_w64(inside && seed_near(MG, s, p)) != 0;
      }
      if (hit) {
        // a long overlapping seed of this chain already visited (bwamem.c:698-707)
        const int len95 = uni((int)ceil(s.len * .95));  // t->len < s->len * .95 <=> t->len < ceil(...)
        bool ov = false;
        for (int base = 0; base < k && !ov; base += 64) {
          const int i = min(base + r, k - 1);
          const bwagpu_seed_t t = seed_at(i);
          const bool tsk = (flag_at(i) & 1) != 0;
          const bool a1 = s.qbeg <= t.qbeg && s.qbeg + s.len - t.qbeg >= s.len >> 2 && (int64_t)(t.qbeg - s.qbeg) != t.rbeg - s.rbeg;
          const bool b1 = t.qbeg <= s.qbeg && t.qbeg + t.len - s.qbeg >= s.len >> 2 && (int64_t)(s.qbeg - t.qbeg) != s.rbeg - t.rbeg;
          ov = __builtin_amdgcn_ballot_w64(base + r < k && !tsk && t.len >= len95 && (a1 || b1)) != 0;
        }
        if (!ov) {  // skipped: srt[k] = 0 (bwamem.c:709)
          set_flag(k, 1);
          continue;
        }
      }
      // ---- this seed is extended (bwamem.c:717-792)
      const int pos = s0 + k;
      const SeedExt* const pe = k < kSelExtCache ? EC + k : a.ext + pos;
      SeedExt e;
      e.calls = uni(__hip_atomic_load(&pe->calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (e.calls == 0) {  // no result yet
        if constexpr (MODE == SEL_REDO) {
          e = extend_seed<16>(o, ref, s, d.lq, q, cw, tbl, tbr);
          store_ext(a.ext + pos, e);
          mem_fence_group();
          if (r == 0) atomicAdd(&a.ctr[SPC_MISS], 1);
          ++n_inline;
        } else if constexpr (MODE == SEL_EMULATE) {
          set_flag(k, 2);  // pending: collected per chain below
          continue;        // its region stays unknown in this pass
        } else {
          const int list = 2 * kSpecBins + spec_bin(d.lq);
          if (r == 0) {
            const int p = atomicAdd(&a.ctr[SPC_CNT + list], 1);
            a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(pos, c);
            a.redo[atomicAdd(&a.ctr[SPC_REDO_N], 1)] = rd;
          }
          redo = true;  // the rest of this read waits for the redo pass
          break;
        }
      } else {
        e.rb = uni64(__hip_atomic_load(&pe->rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.re = uni64(__hip_atomic_load(&pe->re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.qb = uni(__hip_atomic_load(&pe->qb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.qe = uni(__hip_atomic_load(&pe->qe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.score = uni(__hip_atomic_load(&pe->score, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.truesc = uni(__hip_atomic_load(&pe->truesc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.w = uni(__hip_atomic_load(&pe->w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.cells = uni(__hip_atomic_load(&pe->cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        e.rows = uni(__hip_atomic_load(&pe->rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      }
      if constexpr (WRITE) {
        // seedcov over the chain's seeds (bwamem.c:784-788)
        long long cov = 0;
        for (int base = 0; base < ns; base += 64) {
          const int i = base + r;
          const bwagpu_seed_t t = seed_at(min(i, ns - 1));
          const bool in = i < ns && t.qbeg >= e.qb && t.qbeg + t.len <= e.qe && t.rbeg >= e.rb && t.rbeg + t.len <= e.re;
          cov += in ? t.len : 0;
        }
        cov = grp_sum64(cov, 64);
        write_region(a.out + d.s0 + nreg, e, rid, (int)cov, s.len, frac);
        rt.cells += e.cells;
        rt.rows += e.rows;
        rt.calls += e.calls - 1;
      }
      if (nreg < cap_reg) {
        put_regrec(R + nreg, e, s.len);
      } else {
        if (r == 0) __hip_atomic_store(&a.regpos[d.s0 + nreg], pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        mem_fence_group();
      }
      ++nreg;
    }
    if constexpr (MODE == SEL_EMULATE) {  // this chain's round-B tasks
      const int list = kSpecBins + spec_bin(d.lq);
      for (int base = 0; base < ns; base += 64) {
        const int i = base + r;
        const bool pnd = i < ns && (flag_at(min(i, ns - 1)) & 2) != 0;
        const int p = wave_append(&a.ctr[SPC_CNT + list], pnd);
        if (p >= 0) a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(s0 + i, c);
      }
    }
  }
  // (the redo pass as pass 2, its inline extensions in the shape word's upper bits)
  trace_read(MODE, b.n_reads, rd, t_start, d.ns, nreg, 2 | (MODE == SEL_REDO ? n_inline << 4 : 0));
  if constexpr (WRITE) {
    if (!redo) {
      a.out_n[rd] = nreg;
      tl.cells += rt.cells;
      tl.rows += rt.rows;
      tl.calls += rt.calls;
    }
  }
}

template <int MODE, bool HEAVY>
__global__ void __launch_bounds__(64) spec_select_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int tb_bytes) {
  sel_prio();
  static_assert(HEAVY, "one-wave heavy shape only");
  constexpr bool WRITE = MODE != SEL_EMULATE;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int r = (int)(threadIdx.x & 63);
  for (int x = r; x < kMglN; x += 64) reinterpret_cast<int32_t*>(lds)[x] = max_gap_len(o, x);
  Tally tl{0, 0, 0};
  const int n_list = uni(__hip_atomic_load(&a.ctr[MODE == SEL_REDO ? SPC_REDO_N : SPC_HEAVY_N], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT));
  const int32_t* const hlist = MODE == SEL_REDO ? a.redo : a.heavy;
  for (;;) {
    int t = 0;
    if (r == 0) t = atomicAdd(&a.ctr[SPC_SEL_CUR + MODE], 1);
    t = uni(__shfl(t, 0, 64));
    if (t >= n_list) break;
    if (MODE != SEL_REDO && uni(a.hinfo[t].y) >= 0) continue;  // the pair-matrix kernels' read
    select_heavy_read<MODE>(o, ref, b, a, uni(hlist[t]), lds, tb_bytes, false, tl);
  }
  if constexpr (WRITE) {
    if (r != 0) tl = Tally{0, 0, 0};
    block_stats<64>(tl, a.stats);
  }
}

// LIGHT reads (<= kSelLight seeds and chains): the whole read in registers,
// lane i = seed i of the read in processing order (chain-major, as prog[]
// stores them) with its SeedExt; lane c = chain c.  mem_chain2aln's
// sequential decisions depend on each other only through two bit sets — the
// seeds extended so far (their regions) and the seeds skipped so far — so:
//   1. pairs: for every seed k, the 64-bit masks of earlier seeds j whose
//      region would hold it (bwamem.c:678-697: C) and of earlier seeds of its
//      chain that overlap it (698-707, before the skip filter: O) —
//      lane-parallel, no loop-carried state;
//   2. scan: the sequential logic on scalar masks only:
//        hit = C[k] & extended;  skipped = hit && !(O[k] & ~skipped);
//   3. output: every extended seed's seedcov (784-788) and its record,
//      lane-parallel at its rank.
// A seed that must be extended but has no result: SEL_EMULATE marks it a
// round-B task (pending: neither extended nor skipped, as in the per-seed
// form); SEL_FINAL sends the read to the redo pass.
// A misprediction in the final pass of a light read (a seed the replay must
// extend has no result: 10-30 per C2 batch before round 6's strict emulation)
// was extended inline, which took the kernel to 129 VGPRs (3 waves per SIMD);
// sending it to the redo pass instead lost in rounds 3-4 (19.8-19.9 vs
// 21.6-21.7 Mreads/s on C2, then 29.4-30.2 vs 36.9-37.3), while
// the misses were there to extend.
// With the strict emulation (BWAGPU_EMU_STRICT, default) a light read's final
// pass has no miss; -DBWAGPU_LIGHT_INLINE=0 leaves the inline extension out
// (84 VGPRs instead of 131, no LDS rows; a miss, with BWAGPU_EMU_STRICT=0,
// then goes to the redo pass like one of a longer read), but the larger
// resident grid competes with the other records' extension kernels: C2
// fixture 49.3 / 50.6 vs 51.0 / 52.5 Mreads/s, stream 50.5 vs 51.8 (r06p).
#ifndef BWAGPU_LIGHT_INLINE
#define BWAGPU_LIGHT_INLINE 1
#endif
// One light read (1 <= ns <= kSelLight) by the whole wave; d is wave-uniform.
// -> (emulate, SpecArgs::emu_finish) the read is finished: it has no round-B
// task, so its regions are written here and the final pass leaves it out
// (DESIGN.md §25); a read that is not finished is appended to rlist.
template <int MODE>
__device__ __forceinline__ bool light_read(const DevOpt& o, const DevRef& ref, const DevBatch& b, const SpecArgs& a,
                                           const int32_t* MG, uint8_t* tbl, uint8_t* tbr, int rd, const ReadDesc& d,
                                           Tally& tl) {
  constexpr bool WRITE = MODE != SEL_EMULATE;
  const int r = (int)(threadIdx.x & 63);
  const uint64_t lt_mask = r ? (~0ull >> (64 - r)) : 0ull;  // lanes below r
  const uint64_t t_start = g_trace ? __builtin_amdgcn_s_memrealtime() : 0;
  bool finished = false;
    // a miss of the final pass is computed inline and the read starts over
    // with it (a region changes only later decisions; light reads are cheap)
    for (;;) {
    // everything of the read, one round trip
    const int ci = min(r, max(d.nch - 1, 0)), si = min(r, d.ns - 1);
    const int cs_l = b.chain_seed_off[d.c0 + ci] - d.s0, ce_l = b.chain_seed_off[d.c0 + ci + 1] - d.s0;
    const ChainWin cw_l = a.win[d.c0 + ci];
    const int rid_l = b.chain_rid[d.c0 + ci];
    const float fr_l = b.chain_frac_rep[d.c0 + ci];
    const bwagpu_seed_t sd = a.prog[d.s0 + si];
    const SeedExt x = a.ext[d.s0 + si];  // earlier launches, or this wave's inline extension
    // this seed's chain (a chain with a flagged window is never processed)
    int cid = 0, rid = 0;
    float frac = 0.f;
    bool vchain = false;
    for (int c = 0; c < d.nch; ++c) {
      const int cs = __builtin_amdgcn_readlane(cs_l, c), ce = __builtin_amdgcn_readlane(ce_l, c);
      const bool in = r >= cs && r < ce;
      const bool ok = readlane64(cw_l.hi, c) >= readlane64(cw_l.lo, c);
      cid = in ? c : cid;
      vchain = in ? ok : vchain;
      rid = in ? __builtin_amdgcn_readlane(rid_l, c) : rid;
      frac = in ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fr_l), c)) : frac;
    }
    const bool present = r < d.ns && vchain;
    const bool computed = present && x.calls != 0;
    const uint64_t present_m = __builtin_amdgcn_ballot_w64(present);
    const uint64_t computed_m = __builtin_amdgcn_ballot_w64(computed);
    const uint64_t pad_m = __builtin_amdgcn_ballot_w64(r < d.ns && sd.pad_ != 0);
    const int rep_lim = (int)floor(.1 * d.lq) + 1;  // s->len - p->seedlen0 > .1 * l_query, bwamem.c:685
    // ---- 1. pair masks: lane p = (k, j) = (p / S, p % S) with S the seed count
    // rounded up to a power of two (8..64), 64 / S values of k per pass; pass
    // `it`'s ballots land in lane it (c_*, o_*); seedcov of k's region in lane k
    const int S = d.ns <= 8 ? 8 : d.ns <= 16 ? 16 : d.ns <= 32 ? 32 : 64;
    const int lgS = S == 8 ? 3 : S == 16 ? 4 : S == 32 ? 5 : 6;
    const int npass = (S * S) >> 6;
    uint32_t c_lo = 0, c_hi = 0, o_lo = 0, o_hi = 0;
    int cov = 0;
    const int j = r & (S - 1);
    const int jl = min(j, d.ns - 1) << 2;
    // seed j of this lane (and its region), gathered once
    const int64_t j_rbeg = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)(sd.rbeg >> 32)) << 32 |
                                     (uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)sd.rbeg));
    const int j_qbeg = __builtin_amdgcn_ds_bpermute(jl, sd.qbeg), j_len = __builtin_amdgcn_ds_bpermute(jl, sd.len);
    const int j_cid = __builtin_amdgcn_ds_bpermute(jl, cid);
    const bool j_pad = __builtin_amdgcn_ds_bpermute(jl, sd.pad_) != 0;
    const bool j_done = __builtin_amdgcn_ds_bpermute(jl, computed ? 1 : 0) != 0;
    RegRec pj;
    pj.rb = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)(x.rb >> 32)) << 32 |
                      (uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)x.rb));
    pj.re = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)(x.re >> 32)) << 32 |
                      (uint32_t)__builtin_amdgcn_ds_bpermute(jl, (int)x.re));
    pj.qb = __builtin_amdgcn_ds_bpermute(jl, x.qb);
    pj.qe = __builtin_amdgcn_ds_bpermute(jl, x.qe);
    pj.w = __builtin_amdgcn_ds_bpermute(jl, x.w);
    pj.seedlen0 = j_len;
    for (int it = 0; it < npass; ++it) {
      const int k = (it << (6 - lgS)) + (r >> lgS);
      const int kl = min(k, d.ns - 1) << 2;
      bwagpu_seed_t sk;
      sk.rbeg = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)(sd.rbeg >> 32)) << 32 |
                          (uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)sd.rbeg));
      sk.qbeg = __builtin_amdgcn_ds_bpermute(kl, sd.qbeg);
      sk.len = __builtin_amdgcn_ds_bpermute(kl, sd.len);
      const int k_cid = __builtin_amdgcn_ds_bpermute(kl, cid);
      const bool valid = k < d.ns && j < d.ns;
      // C: the region of seed j holds seed k (bwamem.c:682-696)
      const bool inside = valid && j < k && j_done &&
                          !(sk.rbeg < pj.rb || sk.rbeg + sk.len > pj.re || sk.qbeg < pj.qb || sk.qbeg + sk.len > pj.qe) &&
                          !(sk.len - j_len >= rep_lim);
      uint64_t cm = __builtin_amdgcn_ballot_w64(inside);
      if (cm) cm = __builtin_amdgcn_ballot_w64(inside && seed_near(MG, sk, pj));
      // O: seed j of k's chain overlaps it (bwamem.c:701-704; t->len < s->len * .95 <=> t->len < ceil(...))
      const int len95 = (int)ceil(sk.len * .95);
      const bool a1 = sk.qbeg <= j_qbeg && sk.qbeg + sk.len - j_qbeg >= sk.len >> 2 &&
                      (int64_t)(j_qbeg - sk.qbeg) != j_rbeg - sk.rbeg;
      const bool b1 = j_qbeg <= sk.qbeg && j_qbeg + j_len - sk.qbeg >= sk.len >> 2 &&
                      (int64_t)(sk.qbeg - j_qbeg) != sk.rbeg - j_rbeg;
      const uint64_t om = __builtin_amdgcn_ballot_w64(valid && j < k && j_cid == k_cid && !j_pad && j_len >= len95 && (a1 || b1));
      c_lo = r == it ? (uint32_t)cm : c_lo;
      c_hi = r == it ? (uint32_t)(cm >> 32) : c_hi;
      o_lo = r == it ? (uint32_t)om : o_lo;
      o_hi = r == it ? (uint32_t)(om >> 32) : o_hi;
    }
    // ---- 2. the sequential decisions, on scalar masks
    // (emulate) unc: the seeds whose decisions the final pass may take
    // otherwise — the pending ones, every seed extended after one, and every
    // skip that is not certain; a seed skipped here but maybe not there gets
    // a round-B task too (spend), so the final pass never misses
    uint64_t ext = 0, skip = pad_m, pend = 0, spend = 0, unc = 0;
    int miss = -1;
    for (int k = 0; k < d.ns; ++k) {
      const uint64_t bit = 1ull << k;
      if (!(present_m & bit)) continue;
      const int it = (k << lgS) >> 6, sh = (k << lgS) & 63;
      const uint64_t fld = S == 64 ? ~0ull : ((1ull << S) - 1);
      const uint64_t cm = ((uint64_t)__builtin_amdgcn_readlane(c_hi, it) << 32 | (uint32_t)__builtin_amdgcn_readlane(c_lo, it)) >> sh & fld;
      if (cm & ext) {
        const uint64_t om = ((uint64_t)__builtin_amdgcn_readlane(o_hi, it) << 32 | (uint32_t)__builtin_amdgcn_readlane(o_lo, it)) >> sh & fld;
        if (!(om & ~skip)) {  // skipped: srt[k] = 0 (bwamem.c:709)
          skip |= bit;
          // certainly skipped in the final pass too iff a region of a seed
          // decided before any pending one holds it and no seed it overlaps
          // has an uncertain decision
          if (MODE == SEL_EMULATE && a.emu_strict && (!(cm & ext & ~unc) || (om & unc))) {
            unc |= bit;
            if (!(computed_m & bit)) spend |= bit;
          }
          continue;
        }
      }
      if (!(computed_m & bit)) {
        if (MODE == SEL_EMULATE) {
          pend |= bit;  // a round-B task; its region stays unknown in this pass
          unc |= bit;
          continue;
        }
        miss = k;
        break;
      }
      ext |= bit;
      if (MODE == SEL_EMULATE && pend) unc |= bit;  // a pending seed's region may hold it
    }
    // no round-B task: no a.ext[] of the read changes before the final pass,
    // which would load, decide and write what this pass does
    finished = MODE == SEL_EMULATE && a.emu_finish && !(pend | spend);
    // seedcov of an extended seed k's region over its chain's seeds
    // (bwamem.c:784-788), lane-parallel like the pair masks: the passes that
    // hold an extended seed, of a read this pass writes
    if (WRITE ? miss < 0 : finished) {
      const int kn = 1 << (6 - lgS);  // seeds per pass
      for (int it = 0; it < npass; ++it) {
        const uint64_t km = (kn == 64 ? ~0ull : (1ull << kn) - 1) << (it * kn);
        if (!(ext & km)) continue;
        const int k = it * kn + (r >> lgS);
        const int kl = min(k, d.ns - 1) << 2;
        const int k_cid = __builtin_amdgcn_ds_bpermute(kl, cid);
        const bool valid = k < d.ns && j < d.ns;
        const int64_t krb = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)(x.rb >> 32)) << 32 |
                                      (uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)x.rb));
        const int64_t kre = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)(x.re >> 32)) << 32 |
                                      (uint32_t)__builtin_amdgcn_ds_bpermute(kl, (int)x.re));
        const int kqb = __builtin_amdgcn_ds_bpermute(kl, x.qb), kqe = __builtin_amdgcn_ds_bpermute(kl, x.qe);
        int v = valid && j_cid == k_cid && j_qbeg >= kqb && j_qbeg + j_len <= kqe && j_rbeg >= krb &&
                        j_rbeg + j_len <= kre ? j_len : 0;
        for (int m = 1; m < S; m <<= 1) v += __shfl_xor(v, m, 64);
        // lane k takes the sum of its group (lane (k - first k of the pass) * S)
        const int src = (r - it * kn) << lgS;
        const int got = __builtin_amdgcn_ds_bpermute(min(max(src, 0), 63) << 2, v);
        cov = (r >= it * kn && r < (it + 1) * kn) ? got : cov;
      }
    }
    // ---- 3. outputs
    if constexpr (MODE == SEL_EMULATE) {
      const int list = kSpecBins + spec_bin(d.lq);
      const bool pnd = ((pend | spend) >> r) & 1;
      const int p = wave_append(&a.ctr[SPC_CNT + list], pnd);
      if (p >= 0) a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(d.s0 + r, d.c0 + cid);
      if (pend && r == 0) atomicOr(&a.rbits[rd >> 5], 1u << (rd & 31));  // the final pass takes it first
      if (a.emu_finish && r == 0) {
        if (finished) atomicOr(&a.fbits[rd >> 5], 1u << (rd & 31));
        else a.rlist[atomicAdd(&a.ctr[SPC_LIST_N], 1)] = rd;
      }
    } else {
      if (BWAGPU_LIGHT_INLINE && miss >= 0 && d.lq <= kSpecBinLen[0]) {  // extend seed `miss` here, then the read again
        const bwagpu_seed_t sm = uni_seed(a.prog[d.s0 + miss]);
        const int cm_id = uni(__shfl(cid, miss, 64));
        ChainWin cw = a.win[d.c0 + cm_id];
        cw.lo = uni64(cw.lo);
        cw.hi = uni64(cw.hi);
        const SeedExt e = extend_seed<3>(o, ref, sm, d.lq, b.seq + d.qoff, cw, tbl, tbr);
        store_ext(a.ext + d.s0 + miss, e);
        if (r == 0) atomicAdd(&a.ctr[SPC_MISS], 1);
        mem_fence_group();
        __builtin_amdgcn_wave_barrier();
        continue;
      }
      if (miss >= 0) {  // the redo pass (reads > 160 bp)
        // round C extends the miss and every later seed without a result: the
        // redo replay's next misses are among them (one region changes the
        // decisions after it), and the packed kernels take them all at once
        // instead of the redo wave one after another
        const int list = 2 * kSpecBins + spec_bin(d.lq);
        const int p = wave_append(&a.ctr[SPC_CNT + list], r >= miss && present && !computed);
        if (p >= 0) a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(d.s0 + r, d.c0 + cid);
        if (r == miss) a.redo[atomicAdd(&a.ctr[SPC_REDO_N], 1)] = rd;
        break;  // the redo pass writes this read
      }
    }
    if (WRITE || finished) {
      const bool mine = (ext >> r) & 1;
      if (mine) {  // the region of seed r, at its rank (bwamem.c:718-792 field by field; rest zero)
        const int slot = (int)__popcll(ext & lt_mask);
        uint2* dst = reinterpret_cast<uint2*>(a.out + d.s0 + slot);
        dst[0] = make_uint2((uint32_t)x.rb, (uint32_t)((uint64_t)x.rb >> 32));
        dst[1] = make_uint2((uint32_t)x.re, (uint32_t)((uint64_t)x.re >> 32));
        dst[2] = make_uint2((uint32_t)x.qb, (uint32_t)x.qe);
        dst[3] = make_uint2((uint32_t)rid, (uint32_t)x.score);
        dst[4] = make_uint2((uint32_t)x.truesc, 0u);
        dst[5] = make_uint2(0u, 0u);
        dst[6] = make_uint2(0u, (uint32_t)x.w);
        dst[7] = make_uint2((uint32_t)cov, 0u);
        dst[8] = make_uint2(0u, (uint32_t)sd.len);
        dst[9] = make_uint2(0u, __float_as_uint(frac));
        dst[10] = make_uint2(0u, 0u);
        tl.cells += x.cells;
        tl.rows += x.rows;
        tl.calls += x.calls - 1;
      }
      if (r == 0) a.out_n[rd] = (int)__popcll(ext);
    }
    trace_read(MODE, b.n_reads, rd, t_start, d.ns, (int)__popcll(ext), 1);
    break;
    }  // the read's attempts
  return finished;
}

// NARROW light reads (<= kPackW seeds and chains: nine in ten C2 reads), eight
// per wave: group g = lane >> 3 is the read, lane i = lane & 7 its seed i (in
// prog[] order) and its chain i.  The three steps of light_read, with every
// set an 8-bit one held alike by the group's lanes:
//   1. pairs: pass k gives seed k to its group; the group's byte of the two
//      ballots is C[k] / O[k], kept as byte k of a 64-bit word;
//   2. scan: light_read's statements in their order, as selects on the sets,
//      eight steps for the eight reads at once;
//   3. output: seedcov of every extended seed k, summed over the group into
//      lane k, and its record at its rank within the group.
// d, rd and nar (this lane's read is a narrow one of this wave) are the same
// in a group's lanes.  -> the lanes whose read the final pass missed a result
// for; nothing of such a read is written here, light_read takes it.  The
// emulate pass (SpecArgs::emu_finish) -> the lanes whose read it finished: no
// round-B task, its regions written here as the final pass would.
constexpr int kPackW = 8;
template <int MODE>
__device__ __forceinline__ uint64_t light_packed(const DevBatch& b, const SpecArgs& a, const int32_t* MG, int rd,
                                                 const ReadDesc& d, bool nar, Tally& tl) {
  const uint64_t t_start = g_trace ? __builtin_amdgcn_s_memrealtime() : 0;
  int r = (int)(threadIdx.x & 63);
  asm volatile("" : "+v"(r));  // per octet: what derives from it is not held in registers over light_read
  const int i = r & 7, g0 = r & ~7;
  const auto grp = [&](int v, int l) { return __builtin_amdgcn_ds_bpermute((g0 + l) << 2, v); };  // lane l of the group
  const auto grp64 = [&](int64_t v, int l) {
    return (int64_t)((uint64_t)(uint32_t)grp((int)(v >> 32), l) << 32 | (uint32_t)grp((int)v, l));
  };
  const auto byte_of = [&](uint64_t m) { return (uint32_t)(m >> g0) & 0xFFu; };  // the group's lanes of a ballot
  // everything of the eight reads, one round trip
  const bool has_c = nar && i < d.nch, has_s = nar && i < d.ns;
  int ce_l = 15, rid_l = 0;
  float fr_l = 0.f;
  bool ok_l = false;
  if (has_c) {
    ce_l = b.chain_seed_off[d.c0 + i + 1] - d.s0;
    const ChainWin cw = a.win[d.c0 + i];
    ok_l = cw.hi >= cw.lo;  // a chain with a flagged window is never processed
    rid_l = b.chain_rid[d.c0 + i];
    fr_l = b.chain_frac_rep[d.c0 + i];
  }
  bwagpu_seed_t sd{};
  SeedExt x{};
  if (has_s) {
    sd = a.prog[d.s0 + i];
    x = a.ext[d.s0 + i];
  }
  // seed i's chain: the chains' seed ranges follow each other from 0, so it is
  // the number of chains that end at or before i (ends as nibbles, or-ed over
  // the group; 15 for no chain)
  uint32_t ends = (uint32_t)ce_l << (4 * i);
  ends |= (uint32_t)dpp<0xB1>(0, (int)ends);   // quad_perm:[1,0,3,2]
  ends |= (uint32_t)dpp<0x4E>(0, (int)ends);   // quad_perm:[2,3,0,1]
  ends |= (uint32_t)dpp<0x141>(0, (int)ends);  // row_half_mirror
  int cid = 0;
#pragma unroll
  for (int c = 0; c < kPackW - 1; ++c) cid += (int)((ends >> (4 * c)) & 15u) <= i;
  const bool vchain = grp(ok_l ? 1 : 0, cid) != 0;
  const int rid = grp(rid_l, cid);
  const float frac = __int_as_float(grp(__float_as_int(fr_l), cid));
  const bool present = has_s && vchain;
  const bool computed = present && x.calls != 0;
  const bool j_pad = has_s && sd.pad_ != 0;
  const uint32_t present_m = byte_of(__builtin_amdgcn_ballot_w64(present));
  const uint32_t computed_m = byte_of(__builtin_amdgcn_ballot_w64(computed));
  const uint32_t pad_m = byte_of(__builtin_amdgcn_ballot_w64(j_pad));
  const int rep_lim = (int)floor(.1 * d.lq) + 1;  // s->len - p->seedlen0 > .1 * l_query, bwamem.c:685
  // ---- 1. pair masks: pass k, lane j = i; no pass depends on another
  RegRec pj;  // this lane's region
  pj.rb = x.rb;
  pj.re = x.re;
  pj.qb = x.qb;
  pj.qe = x.qe;
  pj.w = x.w;
  pj.seedlen0 = sd.len;
  uint64_t C = 0, O = 0;
  int cov = 0;
#pragma unroll 1  // (unrolled, the eight source lanes' addresses are held over the whole kernel)
  for (int k = 0; k < kPackW && __builtin_amdgcn_ballot_w64(nar && k < d.ns) != 0; ++k) {
    bwagpu_seed_t sk;
    sk.rbeg = grp64(sd.rbeg, k);
    sk.qbeg = grp(sd.qbeg, k);
    sk.len = grp(sd.len, k);
    const int k_cid = grp(cid, k);
    const bool valid = has_s && k < d.ns;
    // C: the region of seed j holds seed k (bwamem.c:682-696)
    const bool inside = valid && i < k && computed &&
                        !(sk.rbeg < pj.rb || sk.rbeg + sk.len > pj.re || sk.qbeg < pj.qb || sk.qbeg + sk.len > pj.qe) &&
                        !(sk.len - sd.len >= rep_lim);
    uint64_t cm = __builtin_amdgcn_ballot_w64(inside);
    if (cm) cm = __builtin_amdgcn_ballot_w64(inside && seed_near(MG, sk, pj));
    // O: seed j of k's chain overlaps it (bwamem.c:701-704; t->len < s->len * .95 <=> t->len < ceil(...))
    const int len95 = (int)ceil(sk.len * .95);
    const bool a1 = sk.qbeg <= sd.qbeg && sk.qbeg + sk.len - sd.qbeg >= sk.len >> 2 &&
                    (int64_t)(sd.qbeg - sk.qbeg) != sd.rbeg - sk.rbeg;
    const bool b1 = sd.qbeg <= sk.qbeg && sd.qbeg + sd.len - sk.qbeg >= sk.len >> 2 &&
                    (int64_t)(sk.qbeg - sd.qbeg) != sk.rbeg - sd.rbeg;
    const uint64_t om = __builtin_amdgcn_ballot_w64(valid && i < k && cid == k_cid && !j_pad && sd.len >= len95 && (a1 || b1));
    C |= (uint64_t)byte_of(cm) << (8 * k);
    O |= (uint64_t)byte_of(om) << (8 * k);
  }
  // ---- 2. the sequential decisions of the eight reads at once (light_read's, as selects)
  uint32_t ext = 0, skip = pad_m, pend = 0, spend = 0, unc = 0;
  bool missed = false;
#pragma unroll
  for (int k = 0; k < kPackW; ++k) {
    const uint32_t bit = 1u << k;
    const uint32_t cm = (uint32_t)(C >> (8 * k)) & 0xFFu, om = (uint32_t)(O >> (8 * k)) & 0xFFu;
    const bool act = (present_m & bit) != 0 && !missed;
    const bool done = (computed_m & bit) != 0;
    const bool skp = act && (cm & ext) != 0 && !(om & ~skip);  // skipped: srt[k] = 0 (bwamem.c:709)
    const bool sunc = skp && MODE == SEL_EMULATE && a.emu_strict && (!(cm & ext & ~unc) || (om & unc));
    const bool nores = act && !skp && !done;  // must be extended, no result
    const bool go = act && !skp && done;
    skip |= skp ? bit : 0u;
    spend |= sunc && !done ? bit : 0u;
    if (MODE == SEL_EMULATE) {
      unc |= sunc || nores || (go && pend) ? bit : 0u;  // (pend: of the steps before this one)
      pend |= nores ? bit : 0u;
    } else {
      missed = missed || nores;
    }
    ext |= go ? bit : 0u;
  }
  // ---- 3. outputs
  if constexpr (MODE == SEL_EMULATE) {
    const bool pnd = nar && (((pend | spend) >> i) & 1u) != 0;
    const int bin = spec_bin(d.lq);
    for (int k = 0; k < kSpecBins; ++k) {  // the reads of a wave differ in length
      const int list = kSpecBins + k;
      const int p = wave_append(&a.ctr[SPC_CNT + list], pnd && bin == k);
      if (p >= 0) a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(d.s0 + i, d.c0 + cid);
    }
    if (nar && pend && i == 0) atomicOr(&a.rbits[rd >> 5], 1u << (rd & 31));  // the final pass takes it first
  }
  // (emulate) no round-B task: no a.ext[] of the read changes before the final
  // pass, which would load, decide and write what this pass does
  const bool wr = nar && (MODE == SEL_EMULATE ? a.emu_finish && !(pend | spend) : !missed);
  // seedcov of an extended seed k's region over its chain's seeds (bwamem.c:784-788),
  // summed over the group into lane k: the k some read this pass writes extended
#pragma unroll 1
  for (int k = 0; k < kPackW; ++k) {
    if (__builtin_amdgcn_ballot_w64(wr && ((ext >> k) & 1u)) == 0) continue;
    const int k_cid = grp(cid, k);
    const int64_t krb = grp64(x.rb, k), kre = grp64(x.re, k);
    const int kqb = grp(x.qb, k), kqe = grp(x.qe, k);
    int v = has_s && k < d.ns && cid == k_cid && sd.qbeg >= kqb && sd.qbeg + sd.len <= kqe && sd.rbeg >= krb &&
                    sd.rbeg + sd.len <= kre ? sd.len : 0;
    v += dpp<0xB1>(0, v);
    v += dpp<0x4E>(0, v);
    v += dpp<0x141>(0, v);
    cov = i == k ? v : cov;
  }
  if (wr && ((ext >> i) & 1u)) {  // the region of seed i, at its rank (bwamem.c:718-792 field by field; rest zero)
    const int slot = (int)__popc(ext & ((1u << i) - 1u));
    uint2* dst = reinterpret_cast<uint2*>(a.out + d.s0 + slot);
    dst[0] = make_uint2((uint32_t)x.rb, (uint32_t)((uint64_t)x.rb >> 32));
    dst[1] = make_uint2((uint32_t)x.re, (uint32_t)((uint64_t)x.re >> 32));
    dst[2] = make_uint2((uint32_t)x.qb, (uint32_t)x.qe);
    dst[3] = make_uint2((uint32_t)rid, (uint32_t)x.score);
    dst[4] = make_uint2((uint32_t)x.truesc, 0u);
    dst[5] = make_uint2(0u, 0u);
    dst[6] = make_uint2(0u, (uint32_t)x.w);
    dst[7] = make_uint2((uint32_t)cov, 0u);
    dst[8] = make_uint2(0u, (uint32_t)sd.len);
    dst[9] = make_uint2(0u, __float_as_uint(frac));
    dst[10] = make_uint2(0u, 0u);
    tl.cells += x.cells;
    tl.rows += x.rows;
    tl.calls += x.calls - 1;
  }
  if (wr && i == 0) a.out_n[rd] = (int)__popc(ext);
  if (uint32_t* const tr = g_trace) {  // trace_read's record, a group's lanes one word each
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
    uint32_t v = 1u;  // shape: light
    v = i == 0 ? (uint32_t)t_start : v;
    v = i == 1 ? (uint32_t)(t_start >> 32) : v;
    v = i == 2 ? (uint32_t)t_end : v;
    v = i == 3 ? (uint32_t)(t_end >> 32) : v;
    v = i == 4 ? (uint32_t)d.ns : v;
    v = i == 5 ? (uint32_t)__popc(ext) : v;
    v = i == 6 ? __builtin_amdgcn_s_getreg((31 << 11) | 20) : v;
    if (nar && !missed) tr[((size_t)MODE * b.n_reads + rd) * 8 + i] = v;
  }
  return __builtin_amdgcn_ballot_w64(MODE == SEL_EMULATE ? wr : nar && missed);
}

// The light reads of a batch.  With SpecArgs::light_pack (bwagpu_ctx_light_pack,
// default) wave w takes the read-octets w, w + NW, ...: reads 8 * octet ...
// 8 * octet + 7.  An octet's narrow reads run packed (light_packed), then its
// wider ones and a narrow read the final pass missed a result for one after
// another (light_read).  Without it, and with risky_first, every light read
// of the wave's share goes through light_read.
// SpecArgs::emu_finish: the emulate pass writes the reads it
// leaves no round-B task (finished: a bit in fbits), and lists the others in
// rlist; the final pass's units are then `per` entries of that list each,
// group g < per of unit u the read rlist[per * u + g] — or, walking all reads
// (risky_first, no light_pack), it leaves the finished ones out.  per = the
// list's length over the grid's waves, rounded up, at most eight: the listed
// reads are the batch's hard ones (most of them wider than eight seeds, which a
// wave runs one after another), so a short list is spread one read per wave
// rather than eight to a wave with most waves idle.
template <int MODE>
__global__ void __launch_bounds__(kBlock) spec_select_light(DevOpt o, DevRef ref, DevBatch b, SpecArgs a,
                                                            int tb_bytes) {
  sel_prio();
  constexpr bool WRITE = MODE != SEL_EMULATE;
  __shared__ int32_t MG[kMglN];
  extern __shared__ __attribute__((aligned(16))) uint8_t lrows[];  // per wave: target rows of an inline extension
  uint8_t* const tbl = lrows + (threadIdx.x >> 6) * 2 * tb_bytes;
  uint8_t* const tbr = tbl + tb_bytes;
  constexpr int kLightList = 64;  // reads a wave lists for light_read before it runs them
  __shared__ int32_t WL[kBlock / 64][kLightList];
  int32_t* const wl = WL[threadIdx.x >> 6];
  for (int x = threadIdx.x; x < kMglN; x += kBlock) MG[x] = max_gap_len(o, x);
  __syncthreads();
  const int r = (int)(threadIdx.x & 63);
  Tally tl{0, 0, 0};
  // static deal: wave w takes the octets (pack), else the reads w, w + NW, ...
  // (light reads cost about the same; no queue atomics), the next descriptors
  // in flight meanwhile.
  // risky_first: the final pass first takes, in its static share, only the
  // reads the emulate pass left a round-B task in (rbits): only those can miss, and a
  // miss is extended inline (one wave, ~0.1 ms per extension, cascades of
  // several in a read) — so they start first, and every other read is claimed
  // afterwards in chunks of kLightChunk by whichever wave is free, instead of
  // waiting behind a wave's misses in its static share.
  const int NW = (int)gridDim.x * (kBlock / 64);
  const int w0 = (int)blockIdx.x * (kBlock / 64) + uni((int)(threadIdx.x >> 6));
  constexpr int kLightChunk = 16;
  int ph = 0, cb = 0, ce = 0, pbase = w0 - 64 * NW;
  uint64_t pm = 0;
  const auto risky = [&](int x) { return ((a.rbits[x >> 5] >> (x & 31)) & 1u) != 0; };
  const auto next_read = [&]() -> int {
    if (ph == 0) {  // this wave's static share, the reads with a round-B task, 64 at a time
      for (;;) {
        if (pm) {
          const int i = __builtin_ctzll(pm);
          pm &= pm - 1;
          return pbase + i * NW;
        }
        pbase += 64 * NW;
        if (pbase >= b.n_reads) break;
        const int x = pbase + r * NW;
        pm = __builtin_amdgcn_ballot_w64(x < b.n_reads && risky(x));
      }
      ph = 1;
    }
    for (;;) {  // the rest, claimed
      if (cb >= ce) {
        int c = 0;
        if (r == 0) c = atomicAdd(&a.ctr[SPC_LIGHT_CUR], kLightChunk);
        c = __builtin_amdgcn_readfirstlane(__shfl(c, 0, 64));
        if (c >= b.n_reads) return b.n_reads;
        cb = c;
        ce = min(c + kLightChunk, b.n_reads);
      }
      const int y = cb++;
      if (!risky(y)) return y;
    }
  };
  const bool dyn = MODE == SEL_FINAL && a.risky_first;
  const bool pack = a.light_pack && !dyn;
  const bool fin = a.emu_finish != 0;
  const bool listed = MODE == SEL_FINAL && fin && pack;  // the units are octets of rlist
  const int n_list =
      listed ? uni(__hip_atomic_load(&a.ctr[SPC_LIST_N], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : b.n_reads;
  // a unit: an octet of reads (pack: a group of eight lanes per read), else 64
  // reads of the wave's share at once (a lane per read), or the one next_read() gives
  const int per = listed ? min(max((n_list + NW - 1) / NW, 1), kPackW) : kPackW;  // a packed unit's reads
  const int n_units = pack ? (n_list + per - 1) / per : b.n_reads;
  const int unit_reads = pack ? kPackW : dyn ? 1 : 64;
  const uint64_t first_lanes = pack ? 0x0101010101010101ull : dyn ? 1ull : ~0ull;  // a read's first lane
  const auto lane_read = [&](int u) {
    const int x = pack ? per * u + (r >> 3) : dyn ? u : u + r * NW;
    if (MODE == SEL_FINAL && listed) return (r >> 3) < per && x < n_list ? a.rlist[x] : b.n_reads;
    return x;
  };
  int n_mine = 0, n_fin_nar = 0, n_fin_wide = 0;  // (emulate, fin) this wave's counts
  // A wave first goes through units — the narrow reads packed, the others
  // only listed (wl) — then through the list with light_read, and so on while
  // units are left: the units' per-lane descriptors are not held over
  // light_read, whose inline extension sets the kernel's register count.
  const uint64_t lt_mask = r ? (~0ull >> (64 - r)) : 0ull;  // lanes below r
  int un = dyn ? next_read() : w0;
  while (un < n_units) {
    int nw = 0;
    ReadDesc dn{};
    int rdn = lane_read(un);
    if (rdn < b.n_reads) dn = a.rdesc[rdn];
    while (un < n_units && nw + unit_reads <= kLightList) {
      const ReadDesc d = dn;
      const int rd = rdn;
      un = dyn ? next_read() : pack ? un + NW : un + 64 * NW;
      if (un < n_units) {
        rdn = lane_read(un);
        if (rdn < b.n_reads) dn = a.rdesc[rdn];
      }
      // not the heavy kernel's read, nor one flagged by spec_reads_kernel
      bool mine = rd < b.n_reads && !(d.ns > kSelLight || d.nch > kSelLight) && !(d.lq > a.lq_bound);
      // (walking all reads) nor one the emulate pass finished
      if (MODE == SEL_FINAL && fin && !listed && mine) mine = !((a.fbits[rd >> 5] >> (rd & 31)) & 1u);
      const bool nar = pack && mine && d.ns <= kPackW && d.nch <= kPackW;
      const bool empty = mine && !nar && d.ns == 0;
      if ((WRITE || fin) && empty) a.out_n[rd] = 0;
      uint64_t wide = __builtin_amdgcn_ballot_w64(mine && !nar && d.ns != 0);
      if constexpr (MODE == SEL_EMULATE) {
        uint64_t done = __builtin_amdgcn_ballot_w64(empty);
        if (pack) done |= light_packed<MODE>(b, a, MG, rd, d, nar, tl);
        if (fin) {  // the finished reads' bits and counts; the other narrow reads listed
          done &= first_lanes;
          const bool first = (first_lanes >> r) & 1, fin_here = (done >> r) & 1;
          const int p = wave_append(&a.ctr[SPC_LIST_N], first && nar && !fin_here);
          if (p >= 0) a.rlist[p] = rd;
          if (pack) {  // an octet's bits are one byte of a word: bit 8g of `done` to bit g
            const uint32_t byte = (uint32_t)((done * 0x0102040810204080ull) >> 56);
            const int rd0 = kPackW * (rd >> 3);  // (the octet's first read, in every lane)
            if (r == 0 && byte) atomicOr(&a.fbits[rd0 >> 5], byte << (rd0 & 31));
          } else if (fin_here) {
            atomicOr(&a.fbits[rd >> 5], 1u << (rd & 31));
          }
          const bool narrow = d.ns <= kPackW && d.nch <= kPackW;
          n_mine += (int)__popcll(__builtin_amdgcn_ballot_w64(mine) & first_lanes);
          n_fin_nar += (int)__popcll(__builtin_amdgcn_ballot_w64(fin_here && narrow));
          n_fin_wide += (int)__popcll(__builtin_amdgcn_ballot_w64(fin_here && !narrow));
        }
      } else {
        if (pack) wide |= light_packed<MODE>(b, a, MG, rd, d, nar, tl);
      }
      wide &= first_lanes;
      if ((wide >> r) & 1) wl[nw + (int)__popcll(wide & lt_mask)] = rd;
      nw += (int)__popcll(wide);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the listed reads one after another, the next one's descriptor in flight meanwhile
    ReadDesc wn{};
    if (nw) wn = a.rdesc[uni(wl[0])];
    for (int k = 0; k < nw; ++k) {
      const ReadDesc u = uniform_desc(wn);
      const int rd = uni(wl[k]);
      if (k + 1 < nw) wn = a.rdesc[uni(wl[k + 1])];
      const bool done = light_read<MODE>(o, ref, b, a, MG, tbl, tbr, rd, u, tl);
      if (MODE == SEL_EMULATE && done) ++(u.ns <= kPackW && u.nch <= kPackW ? n_fin_nar : n_fin_wide);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (WRITE || fin) block_stats<64>(tl, a.stats);
  if (MODE == SEL_EMULATE && fin && r == 0) {
    if (n_mine) atomicAdd(&a.ctr[SPC_LIGHT_N], n_mine);
    if (n_fin_nar) atomicAdd(&a.ctr[SPC_FIN_NAR], n_fin_nar);
    if (n_fin_wide) atomicAdd(&a.ctr[SPC_FIN_WIDE], n_fin_wide);
  }
}

// HEAVY reads with pair matrices (<= kSelMatMaxSeeds seeds).  The same
// decomposition as the light kernel, at a size where one wave cannot hold the
// read:
//   spec_pairs_kernel — one wave per column k (a seed) of a heavy read, over
//     every column of every such read at once: 64-bit words of C[k] (earlier
//     seeds whose region would hold k: bwamem.c:678-697) and O[k] (earlier
//     seeds of k's chain overlapping it: 698-707), and k's seedcov (784-788);
//   spec_scan_kernel  — one wave per read: the sequential decisions on bit
//     sets (lane w holds word w of the extended / skipped / pending sets), then
//     every extended seed's record lane-parallel at its rank.
template <int MODE>
__global__ void __launch_bounds__(kBlock) spec_pairs_kernel(DevOpt o, DevBatch b, SpecArgs a) {
  sel_prio();
  __shared__ int32_t MG[kMglN];
  for (int x = threadIdx.x; x < kMglN; x += kBlock) MG[x] = max_gap_len(o, x);
  __syncthreads();
  const int r = (int)(threadIdx.x & 63);
  const int ncol = uni(__hip_atomic_load(&a.ctr[SPC_HCOLS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const int nwv = (int)gridDim.x * (kBlock / 64);
  int x = (int)blockIdx.x * (kBlock / 64) + uni((int)(threadIdx.x >> 6));
  if (x >= ncol) return;
  // the next column's list entry is fetched under this column's words: two of
  // the four dependent loads in front of a column's first pair test
  int4 hi = a.hinfo[uni(a.colent[x])];
  for (; x < ncol; x += nwv) {
    const int tn = uni(a.colent[min(x + nwv, ncol - 1)]);
    const int rd = uni(hi.x), woff = uni(hi.y), col = uni(hi.z), ns = uni(hi.w);
    const int k = x - col, nw = (ns + 63) >> 6;
    const int nlow = (k + 63) >> 6;  // row k of C and O: the words of the seeds before k
    const ReadDesc d = uniform_desc(a.rdesc[rd]);
    const int rep_lim = (int)floor(.1 * d.lq) + 1;  // s->len - p->seedlen0 > .1 * l_query, bwamem.c:685
    const bwagpu_seed_t s = uni_seed(a.prog[d.s0 + k]);
    const int ck = uni(a.seedchain[d.s0 + k]);
    const int len95 = uni((int)ceil(s.len * .95));  // t->len < s->len * .95 <=> t->len < ceil(...)
    const SeedExt ek = a.ext[d.s0 + k];
    // seedcov depends on k's own region alone: once, in the first pass that
    // sees the region (the emulate pass marks the others with -1)
    const bool k_cov = uni(ek.calls) != 0 && (MODE == SEL_EMULATE || uni(a.cov[d.s0 + k]) < 0);
    const int64_t krb = uni64(ek.rb), kre = uni64(ek.re);
    const int kqb = uni(ek.qb), kqe = uni(ek.qe);
    const int4 hin = a.hinfo[tn];
    // what the scan's per-word sets need of seed k, in one word (the scan read
    // prog, seedchain -> win and ext per seed: two dependent gathers per word)
    const ChainWin wk = a.win[ck];
    if (r == 0)
      a.hflag[d.s0 + k] = (uni64(wk.hi) >= uni64(wk.lo) ? 1 : 0) | (uni(ek.calls) != 0 ? 2 : 0) | (s.pad_ != 0 ? 4 : 0);
    int cov = 0;
    // word w + 1's gathers are issued before word w's ballots
    bwagpu_seed_t sj{};
    int cj = 0;
    SeedExt ej{};
    if (nlow > 0) {
      const int jj = min(r, ns - 1);
      sj = a.prog[d.s0 + jj];
      cj = a.seedchain[d.s0 + jj];
      ej = a.ext[d.s0 + jj];
    }
    for (int w = 0; w < nlow; ++w) {
      const bwagpu_seed_t sc = sj;
      const int cc = cj;
      const SeedExt ec = ej;
      if (w + 1 < nlow) {
        const int jj = min(64 * (w + 1) + r, ns - 1);
        sj = a.prog[d.s0 + jj];
        cj = a.seedchain[d.s0 + jj];
        ej = a.ext[d.s0 + jj];
      }
      const int j = 64 * w + r;
      RegRec p;
      p.rb = ec.rb;
      p.re = ec.re;
      p.qb = ec.qb;
      p.qe = ec.qe;
      p.w = ec.w;
      p.seedlen0 = sc.len;
      const bool inside = j < k && ec.calls != 0 &&
                          !(s.rbeg < p.rb || s.rbeg + s.len > p.re || s.qbeg < p.qb || s.qbeg + s.len > p.qe) &&
                          !(s.len - sc.len >= rep_lim);
      uint64_t cm = __builtin_amdgcn_ballot_w64(inside);
      if (cm) cm = __builtin_amdgcn_ballot_w64(inside && seed_near(MG, s, p));
      if (r == 0) a.mat[woff + tri_off(k) + w] = cm;
      if (MODE == SEL_EMULATE) {  // O depends on no extension result: the final pass keeps it
        const bool a1 = s.qbeg <= sc.qbeg && s.qbeg + s.len - sc.qbeg >= s.len >> 2 &&
                        (int64_t)(sc.qbeg - s.qbeg) != sc.rbeg - s.rbeg;
        const bool b1 = sc.qbeg <= s.qbeg && sc.qbeg + sc.len - s.qbeg >= s.len >> 2 &&
                        (int64_t)(s.qbeg - sc.qbeg) != s.rbeg - sc.rbeg;
        const uint64_t om =
            __builtin_amdgcn_ballot_w64(j < k && cc == ck && sc.pad_ == 0 && sc.len >= len95 && (a1 || b1));
        if (r == 0) a.mat[woff + tri_off(ns) + tri_off(k) + w] = om;
      }
      if (k_cov)
        cov += (j < ns && cc == ck && sc.qbeg >= kqb && sc.qbeg + sc.len <= kqe && sc.rbeg >= krb &&
                sc.rbeg + sc.len <= kre) ? sc.len : 0;
    }
    if (k_cov) {  // the rest of the row, for seedcov alone
      for (int w = nlow; w < nw; ++w) {
        const int j = 64 * w + r, jj = min(j, ns - 1);
        const bwagpu_seed_t sc = a.prog[d.s0 + jj];
        const int cc = a.seedchain[d.s0 + jj];
        cov += (j < ns && cc == ck && sc.qbeg >= kqb && sc.qbeg + sc.len <= kqe && sc.rbeg >= krb &&
                sc.rbeg + sc.len <= kre) ? sc.len : 0;
      }
      cov = (int)grp_sum64(cov, 64);
      if (r == 0) a.cov[d.s0 + k] = cov;
    } else if (MODE == SEL_EMULATE) {
      if (r == 0) a.cov[d.s0 + k] = -1;
    }
    hi = hin;
  }
}

__device__ __forceinline__ uint64_t lane64(uint64_t v, int l) { return (uint64_t)readlane64((int64_t)v, l); }

constexpr int kScanLds = 64 * 1024;  // a read's C and O matrices staged in LDS when they fit

// The final pass over a heavy read computes a missing extension INLINE (the
// read's wave runs extend_seed, then sets the new region's containment bits in
// column k of C for every later seed, and k's seedcov) and carries on: a
// region only changes the decisions of the seeds after it, so the scan state
// up to k stays valid.  (Deferring such a read to round C + the serial redo
// pass cost 2.4-2.6 ms on one read of 1,167 seeds and 749 regions.)
__device__ __forceinline__ void heavy_fill_missing(const DevOpt& o, const DevRef& ref, const DevBatch& b,
                                                   const SpecArgs& a, const ReadDesc& d, int k, int ns,
                                                   uint64_t* C, uint8_t* tbl, uint8_t* tbr) {
  const int r = (int)(threadIdx.x & 63);
  const bwagpu_seed_t sk = uni_seed(a.prog[d.s0 + k]);
  const int ck = uni(a.seedchain[d.s0 + k]);
  ChainWin cw = a.win[ck];
  cw.lo = uni64(cw.lo);
  cw.hi = uni64(cw.hi);
  const SeedExt e = d.lq <= 192 ? extend_seed<3>(o, ref, sk, d.lq, b.seq + d.qoff, cw, tbl, tbr)
                                 : extend_seed<4>(o, ref, sk, d.lq, b.seq + d.qoff, cw, tbl, tbr);  // <= 256 bp
  store_ext(a.ext + d.s0 + k, e);
  if (r == 0) atomicAdd(&a.ctr[SPC_MISS], 1);
  // region k as the containment tests see it (bwamem.c:682-696)
  RegRec p;
  p.rb = e.rb;
  p.re = e.re;
  p.qb = e.qb;
  p.qe = e.qe;
  p.w = e.w;
  p.seedlen0 = sk.len;
  const int rep_lim = (int)floor(.1 * d.lq) + 1;  // s->len - p->seedlen0 > .1 * l_query, bwamem.c:685
  int cov = 0;
  for (int base = 0; base < ns; base += 64) {
    const int j = base + r, jj = min(j, ns - 1);
    const bwagpu_seed_t sj = a.prog[d.s0 + jj];
    // column k of C for the later seeds j > k (the pairs kernel's predicate)
    bool in = j > k && j < ns && !(sj.rbeg < p.rb || sj.rbeg + sj.len > p.re || sj.qbeg < p.qb || sj.qbeg + sj.len > p.qe) &&
              !(sj.len - sk.len >= rep_lim);
    if (in) {
      const int qd1 = sj.qbeg - p.qb;
      const int64_t rd1 = sj.rbeg - p.rb;
      const int g1 = max_gap_len(o, max(qd1 < rd1 ? qd1 : (int)rd1, 0));
      const int bw1 = g1 < p.w ? g1 : p.w;
      const int qd2 = p.qe - (sj.qbeg + sj.len);
      const int64_t rd2 = p.re - (sj.rbeg + sj.len);
      const int g2 = max_gap_len(o, max(qd2 < rd2 ? qd2 : (int)rd2, 0));
      const int bw2 = g2 < p.w ? g2 : p.w;
      in = (qd1 - rd1 < bw1 && rd1 - qd1 < bw1) || (qd2 - rd2 < bw2 && rd2 - qd2 < bw2);
    }
    if (in) C[tri_off(j) + (k >> 6)] |= 1ull << (k & 63);  // word k>>6 of row j: this lane's alone
    // seedcov of k (bwamem.c:784-788): its chain's seeds inside region k
    const int cj = a.seedchain[d.s0 + jj];
    cov += (j < ns && cj == ck && sj.qbeg >= p.qb && sj.qbeg + sj.len <= p.qe && sj.rbeg >= p.rb &&
            sj.rbeg + sj.len <= p.re) ? sj.len : 0;
  }
  cov = (int)grp_sum64(cov, 64);
  if (r == 0) a.cov[d.s0 + k] = cov;
  // the wave re-reads C (LDS or its own global writes) and ext/cov next
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// FOLD (kFuseHeavy; a template argument, so that the kernel
// without it is the one it was): the heavy reads without a matrix, the
// per-seed kernel's, run here as well, each by the wave whose stride meets it
// (select_heavy_read in this launch's LDS, in a loop ahead of the matrix
// reads'), and spec_select_kernel<MODE> is not launched.  That loop's LDS use
// ends with it.  (One wave's LDS operations are ordered by the hardware; the
// fence after the loop only keeps the compiler from moving the matrix loop's
// uint64 accesses across the differently typed ones of that layout.)
static_assert(kScanLds >= kSelHeavyLds, "spec_scan_kernel's LDS holds select_heavy_read's layout");
template <int MODE, bool FOLD>
__global__ void __launch_bounds__(64) spec_scan_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int tb_bytes) {
  sel_prio();
  constexpr bool WRITE = MODE != SEL_EMULATE;
  extern __shared__ __attribute__((aligned(16))) uint64_t M[];
  uint8_t* const tbl = reinterpret_cast<uint8_t*>(M) + kScanLds;
  uint8_t* const tbr = tbl + tb_bytes;
  const int r = (int)(threadIdx.x & 63);
  const uint64_t lt_mask = r ? (~0ull >> (64 - r)) : 0ull;
  const int nh = uni(__hip_atomic_load(&a.ctr[SPC_HEAVY_N], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  Tally tl{0, 0, 0};
  if constexpr (MODE != SEL_REDO) {
    if constexpr (FOLD) {  // a loop of its own, and first: these are the pass's longest reads, and nothing of it stays live below
      Tally ts{0, 0, 0};
      bool mg = true;  // the table survives from one such read to the next
      for (int t = (int)blockIdx.x; t < nh; t += (int)gridDim.x) {
        const int4 hi = a.hinfo[t];
        if (uni(hi.y) >= 0) continue;
        select_heavy_read<MODE>(o, ref, b, a, uni(hi.x), reinterpret_cast<uint8_t*>(M), tb_bytes, mg, ts);
        mg = false;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (r == 0) tl = ts;  // wave-uniform sums: once
    }
  }
  for (int t = (int)blockIdx.x; t < nh; t += (int)gridDim.x) {
    const int4 hi = a.hinfo[t];
    const int rd = uni(hi.x), woff = uni(hi.y), ns = uni(hi.w);
    if (woff < 0) continue;  // no matrix: the per-seed heavy kernel's read, or (fold) the loop above's
    const uint64_t t_start = g_trace ? __builtin_amdgcn_s_memrealtime() : 0;
    const int nw = (ns + 63) >> 6;
    const ReadDesc d = uniform_desc(a.rdesc[rd]);
    if (d.lq > a.lq_bound) continue;  // flagged by spec_reads_kernel
    const int64_t tw = tri_off(ns);
    const uint64_t* Cg = a.mat + woff;
    const bool staged = 2 * tw * 8 <= kScanLds;
    if (staged) {
      for (int i = r; i < 2 * tw; i += 64) M[i] = Cg[i];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    uint64_t* C = staged ? M : a.mat + woff;
    const uint64_t* O = C + tw;
    // per-word sets: lane w holds word w
    uint64_t present_w = 0, computed_w = 0, skip_w = 0;
    for (int w = 0; w < nw; ++w) {
      const int j = 64 * w + r;
      const int f = j < ns ? a.hflag[d.s0 + j] : 0;  // spec_pairs_kernel<MODE>, this pass
      const uint64_t pm = __builtin_amdgcn_ballot_w64(f & 1);  // seeds of a flagged chain are never processed
      const uint64_t cm = __builtin_amdgcn_ballot_w64((f & 3) == 3);
      const uint64_t km = __builtin_amdgcn_ballot_w64(f & 4);
      present_w = r == w ? pm : present_w;
      computed_w = r == w ? cm : computed_w;
      skip_w = r == w ? km : skip_w;
    }
    // Blocks of 64 seeds: the tests of seed k against the regions and skips of
    // the earlier blocks (final by then) run lane-parallel, lane r for seed
    // 64 * bw + r over its row's earlier words; only the in-block word is
    // decided seed by seed, on scalar masks.  (One seed per step cost ~256 ns:
    // a dependent row load, a ballot and a branch per seed.)
    // (emulate, BWAGPU_EMU_STRICT) as in spec_select_light: the seeds of
    // uncertain decision (unc_w: lane w's word) — pending, extended after the
    // first pending one (fp), or skipped without certainty — and a seed
    // skipped here that the final pass might extend gets a round-B task
    uint64_t ext_w = 0, pend_w = 0, unc_w = 0;
    const bool strict = MODE == SEL_EMULATE && a.emu_strict;
    int fp = ns;
    int miss = -1;
    for (int bw = 0; bw < nw && miss < 0; ++bw) {
      const int kb = 64 * bw, k = kb + r;
      const bool valid = k < ns;
      const int64_t row = tri_off(valid ? k : ns - 1);
      bool cb = false, cbc = false;
      for (int w = 0; w < bw; ++w) {
        const uint64_t x = C[row + w] & lane64(ext_w, w);
        cb |= x != 0;
        if (strict) cbc |= (x & ~lane64(unc_w, w)) != 0;  // held by a region decided before fp
      }
      uint64_t cin = valid && r > 0 ? C[row + bw] : 0;
      // O matters only where a region contains seed k
      bool need = valid && (cb || cin != 0), ob = false, ou = false;
      uint64_t oin = 0;
      if (__builtin_amdgcn_ballot_w64(need)) {
        if (need) {
          for (int w = 0; w < bw; ++w) {
            const uint64_t x = O[row + w];
            ob |= (x & ~lane64(skip_w, w)) != 0;
            if (strict) ou |= (x & lane64(unc_w, w)) != 0;  // overlaps a seed of uncertain decision
          }
          oin = r > 0 ? O[row + bw] : 0;
        }
      }
      const uint64_t pres = lane64(present_w, bw);
      uint64_t comp = lane64(computed_w, bw), skp = lane64(skip_w, bw), ext = 0, pend = 0, spend = 0;
      uint64_t uncb = 0;  // this block's seeds of uncertain decision
      const int nb = min(64, ns - kb);
      // The in-block word lane-parallel: seed kb + r's decision depends only on
      // the decisions of the lanes below r (cin and oin hold bits < r) and of
      // the earlier blocks, so every lane decides from the current masks and
      // the masks are exchanged by ballot until none changes.  After t rounds
      // the lanes below t are final: at most nb + 1 rounds, and the fixed point
      // is the serial loop's result.  (The serial loop cost ~230 ns per seed,
      // four lane reads and the branches: DESIGN.md §3 round 7.)  A block where
      // the final pass meets an extended seed without a result (`lack`) runs
      // the serial loop below from its start: it extends inline or defers.
      bool resolved = false;
      {
        const uint64_t skp0 = skp;
        const bool prs = (pres >> r) & 1, cmp = (comp >> r) & 1;
        const bool cb_k = valid && cb, ob_k = valid && ob, cbc_k = valid && cbc, ou_k = valid && ou;
        uint64_t e = 0, sk = skp0, pn = 0, sp = 0, un = 0, lack = 0;
        for (int it = 0; it <= nb + 1; ++it) {
          bool is_skip = false, is_ext = false, is_pend = false, is_spend = false, is_unc = false, is_lack = false;
          if (prs) {
            if ((cb_k || (cin & e)) && !ob_k && !(oin & ~sk)) {  // skipped: srt[k] = 0 (bwamem.c:709)
              is_skip = true;
              if (strict && (!(cbc_k || (cin & e & ~un)) || ou_k || (oin & un))) {
                is_unc = true;
                is_spend = !cmp;
              }
            } else if (!cmp) {
              if (MODE == SEL_EMULATE) is_pend = is_unc = true;  // a round-B task; its region stays unknown
              else is_lack = true;
            } else {
              is_ext = true;
              is_unc = strict && (fp < k || (pn & lt_mask));  // a pending seed's region may hold it
            }
          }
          const uint64_t e1 = __builtin_amdgcn_ballot_w64(is_ext), sk1 = skp0 | __builtin_amdgcn_ballot_w64(is_skip);
          uint64_t pn1 = 0, sp1 = 0, un1 = 0, lack1 = 0;
          if (MODE == SEL_EMULATE) {
            pn1 = __builtin_amdgcn_ballot_w64(is_pend);
            if (strict) {
              sp1 = __builtin_amdgcn_ballot_w64(is_spend);
              un1 = __builtin_amdgcn_ballot_w64(is_unc);
            }
          } else {
            lack1 = __builtin_amdgcn_ballot_w64(is_lack);
          }
          const bool same = e1 == e && sk1 == sk && pn1 == pn && sp1 == sp && un1 == un && lack1 == lack;
          e = e1, sk = sk1, pn = pn1, sp = sp1, un = un1, lack = lack1;
          if (same) {
            resolved = lack == 0;
            break;
          }
        }
        if (resolved) {
          ext = e, skp = sk, pend = pn, spend = sp;
          uncb = strict ? un : pn;
          if (pn) fp = min(fp, kb + (int)__builtin_ctzll(pn));
        }
      }
      const uint64_t cbm = resolved ? 0 : __builtin_amdgcn_ballot_w64(valid && cb);
      uint64_t obm = resolved ? 0 : __builtin_amdgcn_ballot_w64(valid && ob);
      const uint64_t cbcm = resolved ? 0 : __builtin_amdgcn_ballot_w64(valid && cbc);
      const uint64_t oum = resolved ? 0 : __builtin_amdgcn_ballot_w64(valid && ou);
      for (int i = 0; i < (resolved ? 0 : nb); ++i) {
        const uint64_t bit = 1ull << i;
        if (!(pres & bit)) continue;
        if ((cbm & bit) || (lane64(cin, i) & ext)) {
          if (!(obm & bit) && !(lane64(oin, i) & ~skp)) {  // skipped: srt[k] = 0 (bwamem.c:709)
            skp |= bit;
            if (strict && (!((cbcm & bit) || (lane64(cin, i) & ext & ~uncb)) || (oum & bit) || (lane64(oin, i) & uncb))) {
              uncb |= bit;
              if (!(comp & bit)) spend |= bit;
            }
            continue;
          }
        }
        if (!(comp & bit)) {
          if (MODE == SEL_EMULATE) {
            pend |= bit;  // a round-B task; its region stays unknown
            uncb |= bit;
            fp = min(fp, kb + i);
            continue;
          }
          if (d.lq > kSpecBinLen[1]) {  // longer reads: the redo pass
            miss = kb + i;
            break;
          }
          heavy_fill_missing(o, ref, b, a, d, kb + i, ns, C, tbl, tbr);
          comp |= bit;
          cin = valid && r > 0 ? C[row + bw] : 0;  // column kb + i of the later rows
          const bool fresh = valid && !need && cin != 0;
          if (__builtin_amdgcn_ballot_w64(fresh)) {
            if (fresh) {
              for (int w = 0; w < bw; ++w) ob |= (O[row + w] & ~lane64(skip_w, w)) != 0;
              oin = O[row + bw];
            }
            need = need || fresh;
            obm = __builtin_amdgcn_ballot_w64(valid && ob);
          }
        }
        ext |= bit;
        if (strict && fp < kb + i) uncb |= bit;  // a pending seed's region may hold it
      }
      ext_w = r == bw ? ext : ext_w;
      skip_w = r == bw ? skp : skip_w;
      pend_w = r == bw ? pend | spend : pend_w;
      unc_w = r == bw ? uncb : unc_w;
      computed_w = r == bw ? comp : computed_w;
    }
    int nreg = 0;
    if constexpr (MODE == SEL_EMULATE) {
      const int list = kSpecBins + spec_bin(d.lq);
      // the read's round-B tasks take one stretch of the list: one atomic per
      // read, not one dependent atomic per word
      const int tot = (int)grp_sum64(r < nw ? (int)__popcll(pend_w) : 0, 64);
      if (tot) {
        int off = 0;
        if (r == 0) off = atomicAdd(&a.ctr[SPC_CNT + list], tot);
        off = __builtin_amdgcn_readfirstlane(off);
        for (int w = 0; w < nw; ++w) {
          const uint64_t pw = lane64(pend_w, w);
          const int j = 64 * w + r;
          if ((pw >> r) & 1)
            a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + off + (int)__popcll(pw & lt_mask)] =
                make_int2(d.s0 + j, a.seedchain[d.s0 + j]);
          off += (int)__popcll(pw);
        }
      }
    } else {
      if (miss >= 0) {
        if (r == 0) {
          const int list = 2 * kSpecBins + spec_bin(d.lq);
          const int p = atomicAdd(&a.ctr[SPC_CNT + list], 1);
          a.tasks[spec_list_off(list, b.n_chains, b.n_seeds) + p] = make_int2(d.s0 + miss, a.seedchain[d.s0 + miss]);
          a.redo[atomicAdd(&a.ctr[SPC_REDO_N], 1)] = rd;
        }
        continue;  // the redo pass writes this read
      }
      for (int w = 0; w < nw; ++w) {
        const uint64_t ew = (uint64_t)__builtin_amdgcn_readlane((uint32_t)(ext_w >> 32), w) << 32 |
                            (uint32_t)__builtin_amdgcn_readlane((uint32_t)ext_w, w);
        const int j = 64 * w + r;
        if ((ew >> r) & 1) {  // the region of seed j at its rank (bwamem.c:718-792; rest zero)
          const int slot = nreg + (int)__popcll(ew & lt_mask);
          const SeedExt x = a.ext[d.s0 + j];
          const int c = a.seedchain[d.s0 + j];
          uint2* dst = reinterpret_cast<uint2*>(a.out + d.s0 + slot);
          dst[0] = make_uint2((uint32_t)x.rb, (uint32_t)((uint64_t)x.rb >> 32));
          dst[1] = make_uint2((uint32_t)x.re, (uint32_t)((uint64_t)x.re >> 32));
          dst[2] = make_uint2((uint32_t)x.qb, (uint32_t)x.qe);
          dst[3] = make_uint2((uint32_t)b.chain_rid[c], (uint32_t)x.score);
          dst[4] = make_uint2((uint32_t)x.truesc, 0u);
          dst[5] = make_uint2(0u, 0u);
          dst[6] = make_uint2(0u, (uint32_t)x.w);
          dst[7] = make_uint2((uint32_t)a.cov[d.s0 + j], 0u);
          dst[8] = make_uint2(0u, (uint32_t)a.prog[d.s0 + j].len);
          dst[9] = make_uint2(0u, __float_as_uint(b.chain_frac_rep[c]));
          dst[10] = make_uint2(0u, 0u);
          tl.cells += x.cells;
          tl.rows += x.rows;
          tl.calls += x.calls - 1;
        }
        nreg += (int)__popcll(ew);
      }
      if (r == 0) a.out_n[rd] = nreg;
    }
    trace_read(MODE, b.n_reads, rd, t_start, ns, nreg, 3);
  }
  if constexpr (WRITE) block_stats<64>(tl, a.stats);
}

// spec_scan_kernel's grid: one wave per workgroup, a static stride over the
// heavy reads (256-2048 measured within the noise)
constexpr int kScanGrid = 1024;

// The packed light path (bwagpu_ctx_light_pack):
// BWAGPU_LIGHT_PACK sets the process default (0: one read per wave).
#ifndef BWAGPU_LIGHT_PACK_DEFAULT
#define BWAGPU_LIGHT_PACK_DEFAULT 1
#endif
int light_pack_default() {
  static const int v = [] {
    const char* e = getenv("BWAGPU_LIGHT_PACK");
    return e && e[0] ? (atoi(e) != 0 ? 1 : 0) : BWAGPU_LIGHT_PACK_DEFAULT;
  }();
  return v;
}
// ... and its grid's workgroups per CU (BWAGPU_LIGHT_PACK_WGS, an A/B knob)
#ifndef BWAGPU_LIGHT_PACK_WGS_DEFAULT
#define BWAGPU_LIGHT_PACK_WGS_DEFAULT 2
#endif
static int light_pack_wgs() {
  static const int v = [] {
    const char* e = getenv("BWAGPU_LIGHT_PACK_WGS");
    return std::min(std::max(e && e[0] ? atoi(e) : BWAGPU_LIGHT_PACK_WGS_DEFAULT, 1), 64);
  }();
  return v;
}
// ... and the divisor of that grid for the final pass when it runs from the
// emulate pass's list of unfinished reads (BWAGPU_LIGHT_LIST_DIV, an A/B knob;
// DESIGN.md §25 has the sweep)
#ifndef BWAGPU_LIGHT_LIST_DIV_DEFAULT
#define BWAGPU_LIGHT_LIST_DIV_DEFAULT 4
#endif
static int light_list_div() {
  static const int v = [] {
    const char* e = getenv("BWAGPU_LIGHT_LIST_DIV");
    return std::min(std::max(e && e[0] ? atoi(e) : BWAGPU_LIGHT_LIST_DIV_DEFAULT, 1), 64);
  }();
  return v;
}
static int device_cus() {
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
    return 256;
  return ncu;
}

// The two selection shapes of one pass: heavy reads on `side` (when given)
// concurrently with the light reads on `st`; `st` continues once both are done.
template <int MODE>
static void launch_select(const DevOpt& o, const DevRef& ref, const DevBatch& b, const SpecArgs& a, int tb_bytes,
                          hipStream_t st, const SpecStreams& ss) {
  hipStream_t hs = st;
  const bool fold = MODE != SEL_REDO && (ss.fused & kFuseHeavy);
  if (MODE != SEL_REDO && ss.side) {
    (void)hipEventRecord(ss.fork, st);
    (void)hipStreamWaitEvent(ss.side, ss.fork, 0);
    hs = ss.side;
  }
  if (MODE != SEL_REDO) {  // target rows in LDS only for the final pass's inline extension
    const size_t lds = BWAGPU_LIGHT_INLINE && MODE == SEL_FINAL ? (size_t)(kBlock / 64) * 2 * tb_bytes : 0;
    int nb = resident_blocks(spec_select_light<MODE>, lds);
    // packed: the grid by the work (a C2 batch has 8.3 k octets), up to
    // light_pack_wgs() workgroups per CU, and never more than are resident
    if (a.light_pack && !(MODE == SEL_FINAL && a.risky_first)) {
      const int octets = (b.n_reads + kPackW - 1) / kPackW, per_wg = kBlock / 64;
      nb = std::min(nb, std::max(1, std::min((octets + per_wg - 1) / per_wg, light_pack_wgs() * device_cus())));
      // the final pass over the emulate pass's list: its length is known on the
      // device only, and the stride loop is right for any grid
      if (MODE == SEL_FINAL && a.emu_finish) nb = std::max(1, nb / light_list_div());
    }
    hipLaunchKernelGGL((spec_select_light<MODE>), dim3(nb), dim3(kBlock), lds, st, o, ref, b, a, tb_bytes);
  }
  if (MODE != SEL_REDO) {  // heavy reads with pair matrices: all pairs at once, then one scan per read
    const int nb = resident_blocks(spec_pairs_kernel<MODE>, 0);
    hipLaunchKernelGGL((spec_pairs_kernel<MODE>), dim3(nb), dim3(kBlock), 0, hs, o, b, a);
    if (fold)
      hipLaunchKernelGGL((spec_scan_kernel<MODE, true>), dim3(kScanGrid), dim3(64),
                         (size_t)kScanLds + 2 * (size_t)tb_bytes, hs, o, ref, b, a, tb_bytes);
    else
      hipLaunchKernelGGL((spec_scan_kernel<MODE, false>), dim3(kScanGrid), dim3(64),
                         (size_t)kScanLds + 2 * (size_t)tb_bytes, hs, o, ref, b, a, tb_bytes);
  }
  // the rest (no matrix, unless the scan's launch took them; the redo list): one wave per read, per seed
  if (!fold)
    hipLaunchKernelGGL((spec_select_kernel<MODE, true>), dim3(MODE == SEL_REDO ? 256 : 1024), dim3(64),
                       (size_t)kSelHeavyLds, hs, o, ref, b, a, tb_bytes);
  if (hs != st) {
    (void)hipEventRecord(ss.join, hs);
    (void)hipStreamWaitEvent(st, ss.join, 0);
  }
}

// The extension form (bwagpu_ctx_ext_form, per context; tests, A/B): which
// kernels a form runs is ext_plan's table (spec_plan.h).
static std::atomic<int> g_ext_form{0};
int ext_kernel_for(const DevOpt& o, int form, int tb_bytes) { return ext_plan(o, form, tb_bytes, 0).bin[0].code; }
int set_ext_form(int form) {  // the default of contexts made later; -> the previous one (form < 0: query only)
  const int prev = g_ext_form.load(std::memory_order_relaxed);
  if (form >= 0) g_ext_form.store(form > 2 ? 1 : form, std::memory_order_relaxed);
  return prev;
}

// The short-side threshold (bwagpu_ctx_ext_short): sides
// with a query of up to this many bases run sixteen per wave in the eight-
// per-wave phased kernel.  BWAGPU_EXT_SHORT_Q sets the process default (0: off).
#ifndef BWAGPU_EXT_SHORT_Q_DEFAULT
#define BWAGPU_EXT_SHORT_Q_DEFAULT 63
#endif
int ext_short_default() {
  static const int q = [] {
    const char* e = getenv("BWAGPU_EXT_SHORT_Q");
    const int v = e && e[0] ? atoi(e) : BWAGPU_EXT_SHORT_Q_DEFAULT;
    return std::min(std::max(v, 0), kShortQMax);
  }();
  return q;
}
// The short phase trades latency for throughput: a generation of sixteen
// calls of up to 63 columns takes about 1.5 times as long as one of eight (442
// against 296 VALU per row at the longest), and pays only while every wave
// has a next generation to run.  On C2, round A's short runs (36-40 k sides,
// 2.2-2.5 times the grid's 16 384 slots) gained 7-8 % per launch; round B's
// (10-12 k sides, 0.6-0.8 times) lost 9 %.  So a
// short run smaller than short_fill percent of the grid's sixteen-per-wave
// slots runs eight per wave as before.  BWAGPU_EXT_SHORT_FILL sets the process
// default.
#ifndef BWAGPU_EXT_SHORT_FILL_DEFAULT
#define BWAGPU_EXT_SHORT_FILL_DEFAULT 150
#endif
// The ungapped certificate (bwagpu_ctx_ungapped).
// BWAGPU_UNGAPPED=0 starts contexts with it off.
int ungapped_default() {
  static const int on = [] {
    const char* e = getenv("BWAGPU_UNGAPPED");
    return !(e && e[0] == '0');
  }();
  return on;
}
// Certified right sides behind a DP left side are settled after the left
// launch (bwagpu_ctx_ungapped_right).  BWAGPU_UNGAPPED_RIGHT=0
// starts contexts with that off.
int ungapped_right_default() {
  static const int on = [] {
    const char* e = getenv("BWAGPU_UNGAPPED_RIGHT");
    return !(e && e[0] == '0');
  }();
  return on;
}
// The emulate pass finishes the light reads it leaves no round-B task
// (bwagpu_ctx_emu_finish).  BWAGPU_EMU_FINISH=0 starts contexts with it off.
int emu_finish_default() {
  static const int on = [] {
    const char* e = getenv("BWAGPU_EMU_FINISH");
    return !(e && e[0] == '0');
  }();
  return on;
}
// The fused launches (bwagpu_ctx_fused_launches).
// BWAGPU_FUSED_LAUNCHES sets the mask contexts start with.
int fused_launches_default() {
  static const int m = [] {
    const char* e = getenv("BWAGPU_FUSED_LAUNCHES");
    return (e && e[0] ? atoi(e) : 5) & 7;  // bit 2 measured no gain: off
  }();
  return m;
}
int ext_short_fill_default() {
  static const int f = [] {
    const char* e = getenv("BWAGPU_EXT_SHORT_FILL");
    return std::min(std::max(e && e[0] ? atoi(e) : BWAGPU_EXT_SHORT_FILL_DEFAULT, 0), 100000);
  }();
  return f;
}


// a bin's list sorted as its kernel takes it, and its launch
static void launch_sort(const ExtBin& k, const ExtRound& r, int bin0, int nbins, int short_q, int short_fill) {
  if (k.phased) launch_side_sort(r, bin0, nbins, short_q, short_fill);
  else launch_task_sort(r, bin0, nbins);
}
static void launch_ext_bin(const ExtBin& k, const ExtRound& r, int list, const ExtPlan& p, int short_fill) {
  if (k.family == SIDE4) launch_side_bin(k, r, list, p, short_fill);
  else launch_task_bin(k, r, list, p.quad);
}

// One round's extension launches, as ext_plan (spec_plan.h) names them.
// Only the bins the batch's longest read reaches are launched: a persistent
// grid over an empty list still waits for CU slots that the other caller
// stream's extension kernel holds, and its stream waits with it.  Round C
// (mispredicted seeds of long reads: rare) runs on small grids for the same
// reason.
static void launch_ext_round(const DevOpt& o, const DevRef& ref, const DevBatch& b, const SpecArgs& a, int round,
                             int tb_bytes, int lq_max, hipStream_t st, const SpecStreams& ss) {
  const int l = round * kSpecBins;
  const bool bin1 = lq_max > kSpecBinLen[0], bin2 = lq_max > kSpecBinLen[1];
  const ExtPlan plan = ext_plan(o, ss.form, tb_bytes, ss.short_q);
  const ExtRound r{o, ref, b, a, round, tb_bytes, st, ss};
  if (!bin1 || plan.bin[0].phased == plan.bin[1].phased) {
    launch_sort(plan.bin[0], r, 0, bin1 ? 2 : 1, plan.short_q, ss.short_fill);
  } else {
    launch_sort(plan.bin[0], r, 0, 1, plan.short_q, ss.short_fill);
    launch_sort(plan.bin[1], r, 1, 1, 0, ss.short_fill);
  }
  const bool prof = ss.pool && *ss.pool_used + 2 <= ss.pool_n;
  if (prof) (void)hipEventRecord(ss.pool[*ss.pool_used], st);
  launch_ext_bin(plan.bin[0], r, l + 0, plan, ss.short_fill);
  if (prof) {
    (void)hipEventRecord(ss.pool[*ss.pool_used + 1], st);
    *ss.pool_used += 2;
  }
  if (!bin1) return;
  launch_ext_bin(plan.bin[1], r, l + 1, plan, ss.short_fill);
  if (bin2) launch_task_long(r, l + 2);
}

// prep -> round A -> emulate -> round B -> final -> [round C] -> redo, one
// stream.  The final pass sends a read over 160 bp that misses an extension,
// and a heavy read without a pair matrix, to the redo pass, and their
// missing seeds to the round-C lists (a light read: the miss and every later
// seed without a result).  Batches with reads over 160 bp run round C with
// the packed kernels first (C5: one read's chain of 12 misses took the redo
// wave 2.3 ms one extension at a time), so the redo pass mostly replays; on
// shorter batches (C2: no such miss) round C stays unlaunched — a launch
// waited ~0.18 ms per batch for CU slots the other caller stream's extension
// kernel held, even over an empty list — and the redo pass extends the rare
// misses inline.  With the strict emulation (BWAGPU_EMU_STRICT, default) the
// light and matrix-heavy reads have no miss left, so round C stays unlaunched
// on every batch; a heavy read without a matrix can still miss, and the redo
// pass extends that inline.
hipError_t launch_spec_chain2aln(const DevOpt& o, const DevRef& ref, const DevBatch& b, const SpecArgs& a,
                                 int tb_bytes, int lq_max, hipStream_t st, const SpecStreams& ss) {
  if (b.n_reads == 0) return hipSuccess;
  hipLaunchKernelGGL(spec_reads_kernel, dim3((b.n_reads + 255) / 256), dim3(256), 0, st, b, a);
  if (b.n_chains) {
    hipLaunchKernelGGL(spec_chain_kernel, dim3((b.n_chains + 255) / 256), dim3(256), 0, st, o, ref, b, a);
    hipLaunchKernelGGL(spec_order_kernel, dim3(kOrderBlocks), dim3(256), 0, st, o, ref, b, a);
  }
  if (b.n_chains) {
    launch_ext_round(o, ref, b, a, 0, tb_bytes, lq_max, st, ss);
    launch_select<SEL_EMULATE>(o, ref, b, a, tb_bytes, st, ss);
    launch_ext_round(o, ref, b, a, 1, tb_bytes, lq_max, st, ss);
  }
  // (no chains: no emulate pass ran, so nothing is finished or listed, and the final pass takes every read)
  SpecArgs af = a;
  if (!b.n_chains) af.emu_finish = 0;
  launch_select<SEL_FINAL>(o, ref, b, af, tb_bytes, st, ss);
  if (b.n_chains && lq_max > kSpecBinLen[0] && !a.emu_strict) launch_ext_round(o, ref, b, a, 2, tb_bytes, lq_max, st, ss);
  if (b.n_chains) launch_select<SEL_REDO>(o, ref, b, a, tb_bytes, st, ss);
  return hipGetLastError();
}

// a batch's zeroed state in one launch (blockIdx.y = which array)
__global__ void __launch_bounds__(256) spec_clear_kernel(SpecArgs a, int nr, int ns) {
  const int t0 = (int)(blockIdx.x * 256 + threadIdx.x), nt = (int)(gridDim.x * 256);
  switch (blockIdx.y) {
    case 0:
      for (int i = t0; i < 3 * ns; i += nt) reinterpret_cast<uint4*>(a.ext)[i] = make_uint4(0, 0, 0, 0);  // 48 B each
      break;
    case 1:
      for (int i = t0; i < nr; i += nt) a.out_n[i] = 0;
      break;
    case 2:
      for (int i = t0; i < nr / 32 + 1; i += nt) a.rbits[i] = a.fbits[i] = 0;
      break;
    case 3:
      for (int i = t0; i < kQHWords; i += nt) a.qh[i] = 0;
      break;
    case 4:
      for (int i = t0; i < kSortWords; i += nt) a.sorth[i] = 0;
      break;
    default:
      for (int i = t0; i < SPC_WORDS; i += nt) a.ctr[i] = 0;
  }
}
static_assert(sizeof(SeedExt) == 48, "spec_clear_kernel clears SeedExt as three uint4");

hipError_t launch_spec_clear(const SpecArgs& a, int n_reads, int n_seeds, hipStream_t st) {
  hipLaunchKernelGGL(spec_clear_kernel, dim3(256, 6), dim3(256), 0, st, a, n_reads, n_seeds);
  return hipGetLastError();
}

size_t spec_select_lds(int tb_bytes) { return (size_t)kSelHeavyLds + 0 * tb_bytes; }
int spec_redo_cap(int tb_bytes) { return sel_heavy_cap(SEL_REDO, tb_bytes); }

}  // namespace bwagpu
