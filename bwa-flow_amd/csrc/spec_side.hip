// spec_side.hip — the phased extension of the speculative mem_chain2aln
// (spec.hip has the design): its side lists' sort and spec_side4_kernel.
#include "side_sort.h"
#include "spec_dev.h"

namespace bwagpu {

// ---------------------------------------------- phased extension (round 6)
// The extension tasks of the first two length bins run as two launches per
// round: every task's LEFT call(s) (ksw_extend2 with the band retry,
// bwamem.c:717-751), then every task's RIGHT call(s) (752-792, h0 = the left
// score).  Each launch takes calls in the order of their own query length
// (longest first), so the eight calls of a wave have about the same length:
// with a task's left and right calls in one wave generation after another
// (spec_ext4_kernel), a wave ran until its longest call ended while shorter
// ones had ended (25 % of its call-slot cells) and set its columns by its
// longest query (10 %), tools_dev/occ_diag.py.  Lists: the tasks with a left
// side (FatTask, key = left query length) and those with a right side; a
// whole-read seed (neither side) is written by the scatter itself.  The key of
// a side is side_key (side_sort.h) of its query length.

// ------------------------------------- the ungapped certificate (§24, §26)
// A side whose diagonal loses less than the cheapest gap open needs no DP
// (ungapped.h).  spec_ungapped_kernel decides that once per side, ahead of the
// sort, and stores the decision with what the side leaves; the count and the
// scatter read the stored record, so both see the same lists.  The query bytes
// come from the read (a left side runs down from the seed), the target bases
// from the pac at the 2-strand coordinates that fill_side_run reads.
// keep_short > 0 (the first bin's lists with bwagpu_ctx_ext_short_fill at 0:
// every side up to the short threshold takes the short phase) leaves those
// sides to the lists.
//
// The unit of work is a pass, sixteen bases of a side, summarised as an UngSeg
// and folded per side in order (ungapped.h).  A block takes 128 tasks at a
// time, one thread per side: the thread runs the side's first pass itself,
// and a side that this pass leaves alive lists its later passes in LDS, where
// the block's threads take them densely, whichever side they belong to; the
// side's thread then folds the summaries.  (One thread per whole side ran a
// wave until its longest side was through: ten passes for an average of two.)
//
// count (kFuseSort): the block holds both sides' decisions of
// its tasks, so it also counts the sides that enter a list, as spec_sort2_count
// does from the stored records: an LDS histogram of side_key per side, added to
// the lists' global histograms and to SPC_LCNT / SPC_RCNT once at the end.
struct UngSide {
  const uint8_t* rd;  // the read; the side's query base j is rd[p0 + d j]
  int64_t x0;         // ... against the 2-strand coordinate x0 + d j
  int p0, d, qlen, lq;
};
// one pass: the side's bases [base, min(base + 15, qlen - 1)].  Sixteen bases
// are sixteen bytes of the read and at most five of the pac: one unaligned load
// of each (fast), from a window pushed back inside the read / the pac where the
// sixteen would leave it.  Strand, direction and the window's offsets are
// resolved once: the query bytes are brought into the pass's order, clamped to
// 4 and set to 5 past the side's end (a column of zeros in mat8), the target
// bases into one word at two bits each, complemented on the reverse strand;
// a base is then two constant bit-field extracts and the mat8 lookup.  P is
// the count times max_mat less the score sum; M and am are one running
// maximum of (c, earliest index).  A read under 16 bases, a pac under 8 bytes
// or a pass over both strands (a chain window never is) takes the bases one by
// one.  mat: o.mat's 25 scores; mat8[t * 8 + q]: the same for target bases 0-3.
__device__ __forceinline__ UngSeg ung_pass(const UngSide& s, const DevRef& ref, int base, const int8_t* mat,
                                           const int8_t* mat8, int max_mat) {
  const int last = min(base + 15, s.qlen - 1), cnt = last - base + 1;  // rows j < qlen <= tlen lie in the chain's window
  const int64_t two1 = (ref.l_pac << 1) - 1, pac_bytes = (ref.l_pac >> 2) + 1;  // bwa.c:281-282
  const int64_t xa = s.x0 + (int64_t)s.d * base, xb = s.x0 + (int64_t)s.d * last;
  const bool rev = xa >= ref.l_pac;
  const int64_t fa = rev ? two1 - xa : xa, fb = rev ? two1 - xb : xb;
  UngSeg g;
  if (s.lq >= 16 && pac_bytes >= 8 && (xb >= ref.l_pac) == rev) {
    const int qa = s.p0 + s.d * base;  // the read's byte of the pass's first base
    const int ws = min(max(min(qa, qa + 15 * s.d), 0), s.lq - 16);
    const int64_t b0 = min(min(fa, fb) >> 2, pac_bytes - 8);
    uint64_t q[2], tw;
    __builtin_memcpy(q, s.rd + ws, 16);
    __builtin_memcpy(&tw, ref.pac + b0, 8);
    // the query: byte m of (hi, lo) = base m
    uint64_t lo = q[0], hi = q[1];
    int sh = qa - ws;  // 0 .. 15
    if (s.d < 0) {
      lo = __builtin_bswap64(q[1]);
      hi = __builtin_bswap64(q[0]);
      sh = 15 - sh;
    }
    if (sh >= 8) {
      lo = hi;
      hi = 0;
    }
    const int sb = (sh & 7) * 8;
    if (sb) {
      lo = (lo >> sb) | (hi << (64 - sb));
      hi >>= sb;
    }
    constexpr uint64_t k7f = 0x7f7f7f7f7f7f7f7full, k80 = 0x8080808080808080ull, k04 = 0x0404040404040404ull,
                       k05 = 0x0505050505050505ull;
    uint64_t ge = ((((lo & k7f) + (k7f - k04)) | lo) & k80) >> 7;  // 1 in a byte of 5 or more
    lo = (lo & ~(ge * 255)) | (ge * 4);
    ge = ((((hi & k7f) + (k7f - k04)) | hi) & k80) >> 7;
    hi = (hi & ~(ge * 255)) | (ge * 4);
    if (cnt < 8) lo = (lo & ~(~0ull << (8 * cnt))) | (k05 << (8 * cnt));
    if (cnt <= 8) hi = k05;
    else if (cnt < 16) hi = (hi & ~(~0ull << (8 * (cnt - 8)))) | (k05 << (8 * (cnt - 8)));
    // the target: bits 2m + 1 : 2m of w = base m.  The pac holds base f of a byte at bits 7 - 2 (f & 3)
    // and up, so the eight bytes read as one big-endian number hold base f0 + k at bits 63 - 2 (f0 + k)
    const uint64_t T = __builtin_bswap64(tw);
    const int f0 = (int)(fa - (b0 << 2));  // 0 .. 31: the first base among the 32 loaded
    uint32_t w;
    if ((s.d > 0) != rev) {  // f rises along the pass
      w = __builtin_bitreverse32((uint32_t)((T << (2 * f0)) >> 32));
      w = ((w & 0x55555555u) << 1) | ((w >> 1) & 0x55555555u);
    } else {
      w = (uint32_t)(T >> (62 - 2 * f0));
    }
    if (rev) w = ~w;
    const uint32_t qw[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    int c = 0, key = 31;  // key = 32 c + 31 - am: the largest c, and of equal ones the first
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const uint32_t qv = (qw[m >> 2] >> ((m & 3) * 8)) & 255u, tv = (w >> (2 * m)) & 3u;
      c += mat8[(tv << 3) | qv];
      key = max(key, c * 32 + 30 - m);
    }
    g.n = cnt;
    g.c = c;
    g.P = cnt * max_mat - c;
    g.M = key >> 5;
    g.am = 31 - (key & 31);
  } else {
    for (int j = base; j <= last; ++j)
      g = ungseg_combine(g, ungseg_base(mat[pac_base2(ref.pac, ref.l_pac, s.x0 + (int64_t)s.d * j) * 5 +
                                            min((int)s.rd[s.p0 + s.d * j], 4)], max_mat));
  }
  return g;
}

// The decision record `u` of a task: which of its sides (query lengths qb, qr)
// are settled at sort time (cl, cr) and which enter a list.  A certified right
// side behind a left side that needs the DP has the left call's score for its
// h0, which the certificate does not depend on: with `ungt` (SpecArgs::ungt is
// there) it is a late right side, on no list and settled by
// spec_settle_right_kernel after the left launch; without, it stays on the
// right list.  The one copy of the rule: the certificate kernel's count, the
// count kernel, the scatter and the late kernel all decide by it.
struct SideLists {
  bool cl, cr, in_l, in_r, late;
};
__device__ __forceinline__ SideLists side_lists(const UngRec& u, bool ungt, int qb, int qr) {
  SideLists s;
  s.cl = qb > 0 && u.side[0].ok;
  s.in_l = qb > 0 && !s.cl;
  const bool okr = qr > 0 && u.side[1].ok;
  s.cr = okr && !s.in_l;
  s.late = okr && s.in_l && ungt;
  s.in_r = qr > 0 && !s.cr && !s.late;
  return s;
}
// ... from the stored record of the task at `slot` of its list (certificate off: every side enters its list)
__device__ __forceinline__ SideLists side_lists(const SpecArgs& a, size_t slot, int qb, int qr) {
  if (!a.ung) return SideLists{false, false, qb > 0, qr > 0, false};
  return side_lists(a.ung[slot], a.ungt != nullptr, qb, qr);
}

constexpr int kUngTasks = 128;      // tasks of one block pass: a thread per side
constexpr int kUngPassCap = 256 * 9;  // later passes listed per block pass (a side of 160 bases has nine); a side
                                      // whose passes do not fit runs them itself
struct UngSeg16 {  // a pass's summary in LDS (sixteen scores of an int8 each)
  int16_t c, P, M, am;
};

__global__ void __launch_bounds__(256) spec_ungapped_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int round,
                                                            int bin0, int keep_short, int count) {
  sel_prio();
  __shared__ int hist[2][kSideKeys];
  __shared__ int tot[2];
  __shared__ int8_t mat[25], mat8[32];  // the scores by (target, query) base: a lookup per base, kept out of global memory
  __shared__ UngSide sd[256];
  __shared__ uint32_t plist[kUngPassCap];  // side's thread << 8 | pass
  __shared__ UngSeg16 seg[kUngPassCap];
  __shared__ int wsum[4], listed;
  const int tid = (int)threadIdx.x;
  if (tid < 25) mat[tid] = o.mat[tid];
  if (tid < 32) mat8[tid] = (tid & 7) < 5 ? o.mat[(tid >> 3) * 5 + (tid & 7)] : 0;
  if (tid == 0) listed = 0;
  if (count) {  // (untouched without: the kernel then costs what it did before the count)
    for (int k = tid; k < 2 * kSideKeys; k += 256) hist[k >> 8][k & 255] = 0;
    if (tid < 2) tot[tid] = 0;
  }
  __syncthreads();
  const int bin = bin0 + (int)blockIdx.y;
  const int list = round * kSpecBins + bin;
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t off = spec_list_off(list, b.n_chains, b.n_seeds);
  const int2* tl = a.tasks + off;
  const int oe_min = ungapped_oe_min(o.o_del, o.e_del, o.o_ins, o.e_ins);
  const int keep = bin == 0 ? keep_short : 0;
  for (int t0 = (int)blockIdx.x * kUngTasks; t0 < n; t0 += (int)gridDim.x * kUngTasks) {
    const int i = t0 + (tid >> 1), right = tid & 1;
    UngSide s{};
    UngSeg g;
    bool ok = false;
    int extra = 0;  // the passes after the first, if that leaves the side alive
    int qside = 0;  // this side's query length
    if (i < n) {
      const FatTask f = fat_task(b, a, tl[i]);
      if (right && a.ungt) a.ungt[off + i] = UngTask{f.rbeg, f.pos, f.qls};
      const int qb = (int)(f.qls & 1023u), ln = (int)((f.qls >> 10) & 1023u), lq = (int)(f.qls >> 20);
      const int64_t xr = f.rbeg + ln;
      const int qlen = right ? lq - qb - ln : qb;
      const int tlen = right ? (int)(f.rbeg + f.dhi - xr) : f.dlo;
      qside = qlen;
      // a right side starts from the left score, which is at least the seed's (ln * a)
      ok = qlen > keep && ungapped_band_ok(o.w) &&
           ungapped_call_ok(qlen, tlen, ln * o.a, o.w, o.zdrop, o.max_mat, oe_min);
      if (ok) {
        s.rd = b.seq + f.qoff;
        s.p0 = right ? qb + ln : qb - 1;
        s.d = right ? 1 : -1;
        s.x0 = right ? xr : f.rbeg - 1;
        s.qlen = qlen;
        s.lq = lq;
        g = ung_pass(s, ref, 0, mat, mat8, o.max_mat);
        if (!g.dead(oe_min)) extra = (qlen - 1) >> 4;
      }
    }
    // the block's exclusive prefix sum of `extra`: the side's place in the pass list
    int inc = extra;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(inc, d, 64);
      if ((tid & 63) >= d) inc += y;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    int pos = inc - extra;
    for (int w = 0; w < (tid >> 6); ++w) pos += wsum[w];
    const bool fits = pos + extra <= kUngPassCap;  // (the sides that fit are a prefix of those with later passes)
    if (extra > 0 && fits) {
      sd[tid] = s;
      for (int k = 1; k <= extra; ++k) plist[pos + k - 1] = (uint32_t)tid << 8 | (uint32_t)k;  // k <= 63
      atomicMax(&listed, pos + extra);
    }
    __syncthreads();
    const int np = listed;
    for (int p = tid; p < np; p += 256) {
      const uint32_t e = plist[p];
      const UngSeg x = ung_pass(sd[e >> 8], ref, (int)(e & 255u) * 16, mat, mat8, o.max_mat);
      seg[p] = UngSeg16{(int16_t)x.c, (int16_t)x.P, (int16_t)x.M, (int16_t)x.am};
    }
    __syncthreads();
    UngRec::Side rec{0, {0, 0, 0}};
    if (ok) {
      for (int k = 1; k <= extra && !g.dead(oe_min); ++k) {
        UngSeg x;
        if (fits) {
          const UngSeg16 y = seg[pos + k - 1];
          x.n = min(16, s.qlen - 16 * k);
          x.c = y.c;
          x.P = y.P;
          x.M = y.M;
          x.am = y.am;
        } else {
          x = ung_pass(s, ref, 16 * k, mat, mat8, o.max_mat);
        }
        g = ungseg_combine(g, x);
      }
      if (!g.dead(oe_min)) rec = UngRec::Side{1, g.side()};
    }
    if (i < n) a.ung[off + i].side[right] = rec;
    // the task's other side is the neighbouring lane's: i = t0 + (tid >> 1) pairs the lanes 2k and 2k + 1, so a
    // task's two sides never straddle a wave (a change of that mapping has to change this shuffle with it)
    if (count) {
      const int ok2 = __shfl_xor(rec.ok, 1, 64), q2 = __shfl_xor(qside, 1, 64);
      if (i < n) {
        UngRec u{};
        u.side[0].ok = right ? ok2 : rec.ok;
        u.side[1].ok = right ? rec.ok : ok2;
        const SideLists sl = side_lists(u, a.ungt != nullptr, right ? q2 : qside, right ? qside : q2);
        if (right ? sl.in_r : sl.in_l) atomicAdd(&hist[right][side_key(qside)], 1);
      }
    }
    if (tid == 0) listed = 0;
    __syncthreads();
  }
  if (!count) return;
  int32_t* ghL = a.sorth + (round * 2 + bin) * kSortKeys;
  int32_t* ghR = ghL + kSortWordsR;
  for (int k = tid; k < 2 * kSideKeys; k += 256) {
    const int c = hist[k >> 8][k & 255];
    if (c) {
      atomicAdd((k >> 8) ? &ghR[k & 255] : &ghL[k & 255], c);
      atomicAdd(&tot[k >> 8], c);
    }
  }
  __syncthreads();
  if (tid < 2 && tot[tid]) atomicAdd(&a.ctr[(tid ? SPC_RCNT : SPC_LCNT) + list], tot[tid]);
}

// a certified right side's result on top of the slot `e` that the left side
// left (score, truesc) or that a task without a left side starts from, as
// side_advance<G, true> with tt = 0 and x = ungapped_result: bwamem.c:761-792
__device__ __forceinline__ void settle_right(const DevOpt& o, SeedExt& e, int64_t rbeg, int qb, int ln, int lq,
                                             const UngappedSide& u) {
  const int h0 = e.score;  // sc0 (bwamem.c:761)
  const UngappedOut x = ungapped_result(h0, lq - qb - ln, u);
  const bool local = x.gscore <= 0 || x.gscore <= x.score - o.pen_clip3;
  e.qe = local ? qb + ln + x.qle : lq;
  e.re = rbeg + ln + (local ? x.tle : x.gtle);
  e.score = x.score;
  e.truesc += (local ? x.score : x.gscore) - h0;
}

// The SeedExt of a task whose left side is absent or certified, as the side
// launches would leave it (side_start / side_advance with x = ungapped_result,
// one call per side, no rows, no cells, no band retry: max_off = 0).  right:
// the right side is certified too.  Final if the task has no right side or
// `right`; else the partial slot the right launch goes on from.
__device__ __forceinline__ SeedExt settle_sides(const DevOpt& o, const FatTask& f, const UngRec& u, bool right) {
  const int qb = (int)(f.qls & 1023u), ln = (int)((f.qls >> 10) & 1023u), lq = (int)(f.qls >> 20);
  const int qr = lq - qb - ln;
  SeedExt e;
  int calls = 0;
  e.rb = f.rbeg;
  e.qb = 0;
  e.score = e.truesc = ln * o.a;  // bwamem.c:753
  if (qb > 0) {
    const UngappedOut x = ungapped_result(ln * o.a, qb, u.side[0].s);
    const bool local = x.gscore <= 0 || x.gscore <= x.score - o.pen_clip5;
    e.rb = f.rbeg - (local ? x.tle : x.gtle);
    e.qb = local ? qb - x.qle : 0;
    e.score = x.score;
    e.truesc = local ? x.score : x.gscore;
    ++calls;
  }
  e.re = f.rbeg + ln;
  e.qe = lq;
  if (right) {
    settle_right(o, e, f.rbeg, qb, ln, lq, u.side[1].s);
    ++calls;
  } else if (qr > 0) {
    e.re = 0;
    e.qe = 0;
  }
  e.w = o.w;
  e.cells = e.rows = 0;
  e.calls = calls + (right || qr == 0 ? 1 : 0);  // + 1 on a final slot: a computed slot is never all-zero
  return e;
}

__global__ void __launch_bounds__(256) spec_sort2_count(DevBatch b, SpecArgs a, int round, int bin0) {
  sel_prio();
  __shared__ int hist[2][256];
  __shared__ int tot[2];
  const int bin = bin0 + (int)blockIdx.y;
  const int list = round * kSpecBins + bin;
  int32_t* ghL = a.sorth + (round * 2 + bin) * kSortKeys;
  int32_t* ghR = ghL + kSortWordsR;
  for (int k = threadIdx.x; k < 2 * 256; k += 256) hist[k >> 8][k & 255] = 0;
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t off = spec_list_off(list, b.n_chains, b.n_seeds);
  const int2* tl = a.tasks + off;
  const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) {
    const FatTask f = fat_task(b, a, tl[i]);
    const int qb = (int)(f.qls & 1023u), ln = (int)((f.qls >> 10) & 1023u), lq = (int)(f.qls >> 20);
    const int qr = lq - qb - ln;
    const SideLists sl = side_lists(a, off + i, qb, qr);
    if (sl.in_l) atomicAdd(&hist[0][side_key(qb)], 1);
    if (sl.in_r) atomicAdd(&hist[1][side_key(qr)], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * 256; k += 256) {
    const int c = hist[k >> 8][k & 255];
    if (c) {
      atomicAdd((k >> 8) ? &ghR[k & 255] : &ghL[k & 255], c);
      atomicAdd(&tot[k >> 8], c);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && tot[threadIdx.x])
    atomicAdd(&a.ctr[(threadIdx.x ? SPC_RCNT : SPC_LCNT) + list], tot[threadIdx.x]);
}

// exclusive scan of the 256 keys of each (side, bin) histogram: one block each
// (bins bin0 .. bin0 + nbins - 1).  short_q > 0: the first bin's lists get a
// short run, the sides with a query of up to short_q bases; its first position
// (= the sides with a longer query: the list is in descending length order)
// goes to the list's SPC_LLONG / SPC_RLONG word here, before the scatter turns
// the key positions into cursors.
__global__ void __launch_bounds__(256) spec_sort2_scan(SpecArgs a, int round, int bin0, int nbins, int short_q) {
  sel_prio();
  __shared__ int part[256];
  const int bin = bin0 + (int)blockIdx.x % nbins, side = (int)blockIdx.x / nbins;
  int32_t* gh = a.sorth + (round * 2 + bin) * kSortKeys + side * kSortWordsR;
  const int t = (int)threadIdx.x;
  const int v = gh[t];
  part[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int x = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  gh[t] = part[t] - v;  // the key's first position (a cursor from here on)
  if (short_q > 0 && bin == 0 && t == side_key(short_q))
    a.ctr[(side ? SPC_RLONG : SPC_LLONG) + round * kSpecBins + bin] = part[t] - v;
}

// The scatter.  scan = 0: spec_sort2_scan has turned the lists' histograms into
// cursors, and a pass's range for a key is what it claims there.  scan = 1
// (kFuseSort): the histograms stay as counted and read-only;
// every block computes their exclusive prefix itself at its start (a wave per
// side, side_sort.h), and a pass's range for a key is that first position plus
// what it claims from the key's cursor, a zeroed word kSortCursor further on.
// Block 0 of the first bin then writes the lists' SPC_LLONG / SPC_RLONG words
// (short_q > 0) as the scan kernel would: the side kernels read them after
// this kernel's end.
__global__ void __launch_bounds__(256) spec_sort2_scatter(DevOpt o, DevBatch b, SpecArgs a, int round, int bin0,
                                                          int short_q, int scan) {
  sel_prio();
  __shared__ int cnt[2][256];
  __shared__ int first[2][kSideKeys];  // scan: a key's first position
  __shared__ int ung[2];  // sides settled here, their query lengths
  const int bin = bin0 + (int)blockIdx.y;
  const int list = round * kSpecBins + bin;
  int32_t* ghL = a.sorth + (round * 2 + bin) * kSortKeys;
  int32_t* ghR = ghL + kSortWordsR;
  for (int k = threadIdx.x; k < 2 * 256; k += 256) cnt[k >> 8][k & 255] = 0;
  if (threadIdx.x < 2) ung[threadIdx.x] = 0;
  if (scan) {
    const int side = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (side < 2) {
      const int4 h4 = reinterpret_cast<const int4*>(side ? ghR : ghL)[lane];
      const int32_t h[kSideLaneKeys] = {h4.x, h4.y, h4.z, h4.w};
      const int32_t own = side_lane_total(h);
      int32_t inc = own;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) inc = side_scan_step(inc, __shfl_up(inc, d, 64), lane, d);
      int32_t f[kSideLaneKeys];
      side_lane_prefix(h, inc - own, f);
#pragma unroll
      for (int j = 0; j < kSideLaneKeys; ++j) first[side][kSideLaneKeys * lane + j] = f[j];
    }
    ghL += kSortCursor;
    ghR += kSortCursor;
  }  // (scan = 0 leaves first[] untouched and unread: the kernel then costs what it did before)
  __syncthreads();
  if (scan && short_q > 0 && bin == 0 && blockIdx.x == 0 && threadIdx.x < 2)
    a.ctr[(threadIdx.x ? SPC_RLONG : SPC_LLONG) + list] = side_short_first(first[threadIdx.x], short_q);
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t off = spec_list_off(list, b.n_chains, b.n_seeds);
  const int2* tl = a.tasks + off;
  FatTask* foL = a.ftask + off;
  FatTask* foR = a.ftaskR + off;
  const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int i0 = (int)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  constexpr int kPer = 8;  // entries per thread held across the barrier
  int kl[kPer], kr[kPer], rl[kPer], rr[kPer];
  FatTask ft[kPer];
  for (int base = i0; base < i1; base += 256 * kPer) {
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      const int i = base + m * 256 + (int)threadIdx.x;
      kl[m] = kr[m] = -1;
      if (i < i1) {
        ft[m] = fat_task(b, a, tl[i]);
        const int qb = (int)(ft[m].qls & 1023u), ln = (int)((ft[m].qls >> 10) & 1023u), lq = (int)(ft[m].qls >> 20);
        const int qr = lq - qb - ln;
        const SideLists sl = side_lists(a, off + i, qb, qr);
        if (sl.in_l) {
          kl[m] = side_key(qb);
          rl[m] = atomicAdd(&cnt[0][kl[m]], 1);
        }
        if (sl.in_r) {
          kr[m] = side_key(qr);
          rr[m] = atomicAdd(&cnt[1][kr[m]], 1);
        }
        if (!sl.in_l) {
          // no left call to run: a whole-read seed (bwamem.c:753, 781: no ksw_extend2 call), or sides the
          // certificate settles; with a right side on its list, the slot that launch goes on from
          if (qb > 0 || !sl.in_r)
            a.ext[ft[m].pos] = settle_sides(o, ft[m], sl.cl || sl.cr ? a.ung[off + i] : UngRec{}, sl.cr);
          if (sl.cl || sl.cr) {
            atomicAdd(&ung[0], (sl.cl ? 1 : 0) + (sl.cr ? 1 : 0));
            atomicAdd(&ung[1], (sl.cl ? qb : 0) + (sl.cr ? qr : 0));
          }
        }
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * 256; k += 256) {
      const int c = cnt[k >> 8][k & 255];
      cnt[k >> 8][k & 255] =
          c ? (scan ? first[k >> 8][k & 255] : 0) + atomicAdd((k >> 8) ? &ghR[k & 255] : &ghL[k & 255], c) : 0;  // this pass's range
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kPer; ++m) {
      if (kl[m] >= 0) foL[cnt[0][kl[m]] + rl[m]] = ft[m];
      if (kr[m] >= 0) foR[cnt[1][kr[m]] + rr[m]] = ft[m];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * 256; k += 256) cnt[k >> 8][k & 255] = 0;
    __syncthreads();
  }
  if (threadIdx.x < 2 && ung[threadIdx.x])
    atomicAdd(&a.ctr[(threadIdx.x ? SPC_UNG_Q : SPC_UNG_N) + round], ung[threadIdx.x]);
}

// The late right sides of a round's phased lists, after the
// lists' left launches: a thread per task of the list re-derives the class from
// the stored record, as side_lists does.  The seed's slot holds what its left
// side left (side_advance<G, false>'s partial slot), and the right call's
// result follows from the stored certificate with h0 = that score, as
// side_start / side_advance<G, true> would leave it after one call without a
// band retry (max_off = 0) that ran no row.  (A compact list of the class,
// written by the scatter, made that kernel longer than this pass over the
// records takes: DESIGN.md §26.)
__global__ void __launch_bounds__(256) spec_settle_right_kernel(DevOpt o, DevBatch b, SpecArgs a, int round, int bin0) {
  sel_prio();
  __shared__ int tot[2];              // sides, their query lengths
  __shared__ unsigned long long cel;  // the finished tasks' cells
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  if (threadIdx.x == 0) cel = 0;
  __syncthreads();
  const int list = round * kSpecBins + bin0 + (int)blockIdx.y;
  const int n = __hip_atomic_load(&a.ctr[SPC_CNT + list], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const size_t off = spec_list_off(list, b.n_chains, b.n_seeds);
  int sides = 0, bases = 0;
  unsigned long long cells = 0;
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < n; i += (int)gridDim.x * 256) {
    const UngTask t = a.ungt[off + i];
    const int qb = (int)(t.qls & 1023u), ln = (int)((t.qls >> 10) & 1023u), lq = (int)(t.qls >> 20);
    if (!side_lists(a, off + i, qb, lq - qb - ln).late) continue;
    SeedExt e = a.ext[t.pos];
    settle_right(o, e, t.rbeg, qb, ln, lq, a.ung[off + i].side[1].s);
    e.w = max(e.w, o.w);
    e.calls += 2;  // the right call, and + 1 on a final slot
    a.ext[t.pos] = e;
    ++sides;
    bases += lq - qb - ln;
    cells += (unsigned long long)e.cells;
  }
  if (sides) {
    atomicAdd(&tot[0], sides);
    atomicAdd(&tot[1], bases);
    atomicAdd(&cel, cells);
  }
  __syncthreads();
  if (threadIdx.x < 2 && tot[threadIdx.x])
    atomicAdd(&a.ctr[(threadIdx.x ? SPC_UNGR_Q : SPC_UNGR_N) + round], tot[threadIdx.x]);
  if (threadIdx.x == 0 && cel) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), cel);
}

// One side of a task in flight (LDS, per sub-slot, between its calls).
struct SideTask {
  int64_t rbeg, qoff, rb;
  int32_t pos, dlo, dhi, qbeg, len, lq;
  int32_t tt, score, h0, truesc, qb, aw0, cells, rows, calls, pad_;
};
static_assert(sizeof(SideTask) <= 96, "SideTask layout");
typedef __attribute__((address_space(3))) SideTask LdsS;
#define SIDE_FIELDS(X) X(rbeg) X(qoff) X(rb) X(pos) X(dlo) X(dhi) X(qbeg) X(len) X(lq) X(tt) X(score) X(h0) \
  X(truesc) X(qb) X(aw0) X(cells) X(rows) X(calls)
__device__ __forceinline__ void spark(LdsS* p, const SideTask& t) {
#define X(f) p->f = t.f;
  SIDE_FIELDS(X)
#undef X
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ SideTask sload(LdsS* p) {
  asm volatile("" ::: "memory");
  SideTask t;
#define X(f) t.f = p->f;
  SIDE_FIELDS(X)
#undef X
  return t;
}
#undef SIDE_FIELDS

// a sub-slot's start: the side's target rows into its LDS buffer, the state
// of the side's first call (a right side reads what the left launch left in
// the seed's SeedExt slot)
template <int G, bool RIGHT>
__device__ __forceinline__ void side_start(SideTask& t, const DevOpt& o, const DevRef& ref, const SpecArgs& a,
                                           const FatTask& f, uint8_t* tb) {
  t.rbeg = f.rbeg;
  t.qoff = f.qoff;
  t.pos = f.pos;
  t.dlo = f.dlo;
  t.dhi = f.dhi;
  t.qbeg = (int)(f.qls & 1023u);
  t.len = (int)((f.qls >> 10) & 1023u);
  t.lq = (int)(f.qls >> 20);
  t.tt = 0;
  const int64_t pac_bytes = (ref.l_pac >> 2) + 1;
  const int r = (int)(threadIdx.x & (G - 1));
  if constexpr (!RIGHT) {
    const int n = rows_needed(o, t.qbeg, t.dlo, o.w << 1, o.pen_clip5);
    const int R = (n + G - 1) / G;
    if (R <= 32) fill_side_run<G>(tb, t.rbeg - 1, -1, r * R, min(r * R + R, n), ref, pac_bytes);
    else fill_two_half<G>(tb, t.rbeg - 1, n, tb, 0, 0, ref);
    t.score = -1;  // bwamem.c:753 (a left side: the retry test compares with -1)
    t.h0 = t.len * o.a;
    t.truesc = -1;
    t.qb = 0;
    t.rb = t.rbeg;
    t.aw0 = o.w;
    t.cells = t.rows = t.calls = 0;
  } else {
    const int64_t x0 = t.rbeg + t.len;
    const int qr = t.lq - t.qbeg - t.len;
    const int n = rows_needed(o, qr, (int)(t.rbeg + t.dhi - x0), o.w << 1, o.pen_clip3);
    const int R = (n + G - 1) / G;
    if (R <= 32) fill_side_run<G>(tb, x0, 1, r * R, min(r * R + R, n), ref, pac_bytes);
    else fill_two_half<G>(tb, 0, 0, tb, x0, n, ref);
    if (t.qbeg > 0) {  // the left launch's result (the same wave wrote... another wave did: SeedExt slot)
      const SeedExt e = a.ext[t.pos];
      t.score = e.score;
      t.truesc = e.truesc;
      t.qb = e.qb;
      t.rb = e.rb;
      t.aw0 = e.w;
      t.cells = e.cells;
      t.rows = e.rows;
      t.calls = e.calls;
    } else {
      t.score = t.truesc = t.len * o.a;  // bwamem.c:753
      t.qb = 0;
      t.rb = t.rbeg;
      t.aw0 = o.w;
      t.cells = t.rows = t.calls = 0;
    }
    t.h0 = t.score;  // sc0 (bwamem.c:761)
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool RIGHT>
__device__ __forceinline__ QCall side_call(const SideTask& t, const DevOpt& o, const uint8_t* seq, const uint8_t* tb) {
  QCall q;
  if constexpr (!RIGHT) {
    q.qlen = t.qbeg;
    q.tlen = t.dlo;
    q.qa = t.qbeg - 1;
    q.qd = -1;
    q.eb = o.pen_clip5;
  } else {
    const int64_t x0 = t.rbeg + t.len;
    q.qlen = t.lq - t.qbeg - t.len;
    q.tlen = (int)(t.rbeg + t.dhi - x0);
    q.qa = t.qbeg + t.len;
    q.qd = 1;
    q.eb = o.pen_clip3;
  }
  q.h0 = t.h0;
  q.w = o.w << t.tt;
  q.zdrop = o.zdrop;
  q.q = seq + t.qoff;
  q.tb = tb;
  q.tlen = rows_needed(o, q.qlen, q.tlen, q.w, q.eb);  // as qtask_call
  return q;
}

// the call's result (bwamem.c:737-751 / 770-792); true = the side is done,
// its result written to the seed's SeedExt slot (partial after a left side
// with a right side to come, else final)
template <int G, bool RIGHT>
__device__ __forceinline__ bool side_advance(SideTask& t, const DevOpt& o, const SpecArgs& a, const ExtOut& x,
                                             const Tally32& tl, long long& spec_cells) {
  t.cells += tl.cells;
  t.rows += tl.rows;
  t.calls += tl.calls;
  const int prev = t.score;
  t.score = x.score;
  const int aw = o.w << t.tt;
  if (t.tt == 0 && !(x.score == prev || x.max_off < (aw >> 1) + (aw >> 2))) {  // the band retry (MAX_BAND_TRY)
    t.tt = 1;
    return false;
  }
  const int eb = RIGHT ? o.pen_clip3 : o.pen_clip5;
  const bool local = x.gscore <= 0 || x.gscore <= x.score - eb;
  SeedExt e;
  if constexpr (!RIGHT) {
    const int qr = t.lq - t.qbeg - t.len;
    e.rb = t.rbeg - (local ? x.tle : x.gtle);
    e.qb = local ? t.qbeg - x.qle : 0;
    e.score = t.score;
    e.truesc = local ? x.score : x.gscore;
    if (qr != 0) {  // partial: the right launch goes on from here
      e.re = 0;
      e.qe = 0;
      e.w = aw;
      e.cells = t.cells;
      e.rows = t.rows;
      e.calls = t.calls;
    } else {
      e.re = t.rbeg + t.len;
      e.qe = t.lq;
      e.w = max(aw, o.w);
      e.cells = t.cells;
      e.rows = t.rows;
      e.calls = t.calls + 1;  // + 1: a computed slot is never all-zero
      spec_cells += t.cells;
    }
  } else {
    e.rb = t.rb;
    e.qb = t.qb;
    e.qe = local ? t.qbeg + t.len + x.qle : t.lq;
    e.re = t.rbeg + t.len + (local ? x.tle : x.gtle);
    e.score = t.score;
    e.truesc = t.truesc + (local ? x.score : x.gscore) - t.h0;
    e.w = max(t.aw0, aw);
    e.cells = t.cells;
    e.rows = t.rows;
    e.calls = t.calls + 1;
    spec_cells += t.cells;
  }
  store_ext_half<G>(a.ext + t.pos, e);
  return true;
}

// a side's query bytes into LDS in column order (qd[j] = column j), so the DP
// has no global load (its prologue read them from HBM: a dependent round trip
// per generation)
template <int G, bool RIGHT>
__device__ __forceinline__ void side_query(const DevBatch& b, const FatTask& f, uint8_t* qd, int qb) {
  const int r = (int)(threadIdx.x & (G - 1));
  const int qbeg = (int)(f.qls & 1023u), len = (int)((f.qls >> 10) & 1023u), lq = (int)(f.qls >> 20);
  const int qlen = min(RIGHT ? lq - qbeg - len : qbeg, qb);
  const uint8_t* q = b.seq + f.qoff + (RIGHT ? qbeg + len : qbeg - 1);
  for (int j = r; j < qlen; j += G) qd[j] = q[RIGHT ? j : -j];
}

// The phased extension's loop over one run of a side list: 128 / G calls per
// wave (G = 16: eight, 32: four, 8: sixteen) in the
// packed 16-bit DP (extend_quad), claimed in the list's order (the side's
// query length, longest first) from the run's own sharded heads.  wlds = the
// wave's own LDS slice, cut per group: A's and B's target rows (tb_bytes
// each), their states, their query bytes.  Returns the sides it started.
template <int G, int PMAX, bool K8, bool RIGHT>
__device__ __forceinline__ int side_loop(const DevOpt& o, const DevRef& ref, const DevBatch& b, const SpecArgs& a,
                                         const FatTask* fl, int n, int32_t* heads, uint8_t* wlds, int tb_bytes,
                                         long long& spec_cells
#ifdef BWAGPU_OCC_DIAG
                                         , unsigned long long* tw, unsigned long long* occ
#endif
) {
  constexpr uint64_t kLead =
      G == 8 ? 0x0101010101010101ull : (G == 16 ? 0x0001000100010001ull : 0x0000000100000001ull);
  const uint64_t below = kLead & ((1ull << ((int)threadIdx.x & (64 - G))) - 1);
  constexpr int QB = PMAX * G;
  uint8_t* const ta_ = wlds + (size_t)((threadIdx.x & 63) / G) * (2 * (size_t)tb_bytes + 2 * kSideLds + 2 * QB);
  uint8_t* const tb_ = ta_ + tb_bytes;
  LdsS* const sa = (LdsS*)(tb_ + tb_bytes);
  LdsS* const sb = (LdsS*)(tb_ + tb_bytes + kSideLds);
  uint8_t* const qa_ = tb_ + tb_bytes + 2 * kSideLds;
  uint8_t* const qb_ = qa_ + QB;
  ShardQ qq;
  qq.init(heads, n);
  bool ha = false, hb = false, more = n > 0;
  int started = 0;
  for (;;) {
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
    if (more) {  // every sub-slot without a call takes the next entry: one claim for the wave
      const uint64_t na = __builtin_amdgcn_ballot_w64(!ha) & kLead, nb = __builtin_amdgcn_ballot_w64(!hb) & kLead;
      const int nn = __popcll(na) + __popcll(nb);
      if (nn > 0) {
        int m0, cap;
        if (qq.claim(nn, m0, cap)) {
          const int ia = m0 + __popcll(na & below) + __popcll(nb & below), ib = ia + (ha ? 0 : 1);
          if (!ha && ia < cap) {
            SideTask t;
            const FatTask f = fl[qq.shard + 8 * ia];
            side_query<G, RIGHT>(b, f, qa_, QB);
            side_start<G, RIGHT>(t, o, ref, a, f, ta_);
            spark(sa, t);
            ha = true;
            ++started;
          }
          if (!hb && ib < cap) {
            SideTask t;
            const FatTask f = fl[qq.shard + 8 * ib];
            side_query<G, RIGHT>(b, f, qb_, QB);
            side_start<G, RIGHT>(t, o, ref, a, f, tb_);
            spark(sb, t);
            hb = true;
            ++started;
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
      if (!more) break;
      continue;
    }
    QCall ca = quad_idle(qa_, ta_), cb = quad_idle(qb_, tb_);  // every query pointer in LDS
    if (ha) {
      ca = side_call<RIGHT>(sload(sa), o, b.seq, ta_);
      ca.q = qa_;
      ca.qa = 0;
      ca.qd = 1;
    }
    if (hb) {
      cb = side_call<RIGHT>(sload(sb), o, b.seq, tb_);
      cb.q = qb_;
      cb.qa = 0;
      cb.qd = 1;
    }
    ExtOut xa, xb;
    Tally32 tla{0, 0, 0}, tlb{0, 0, 0};
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c2 = __builtin_amdgcn_s_memtime();
    tw[1] += c2 - c1;
#endif
    extend_quad_dispatch<G, PMAX, K8>(o, ca, cb, xa, xb, tla, tlb);
#ifdef BWAGPU_OCC_DIAG
    const unsigned long long c3 = __builtin_amdgcn_s_memtime();
    tw[2] += c3 - c2;
    occ_diag<G>(occ, ca, cb, tla, tlb);
#endif
    if (ha) {
      SideTask t = sload(sa);
      if (side_advance<G, RIGHT>(t, o, a, xa, tla, spec_cells)) ha = false;
      else spark(sa, t);
    }
    if (hb) {
      SideTask t = sload(sb);
      if (side_advance<G, RIGHT>(t, o, a, xb, tlb, spec_cells)) hb = false;
      else spark(sb, t);
    }
#ifdef BWAGPU_OCC_DIAG
    tw[3] += __builtin_amdgcn_s_memtime() - c3;
#endif
  }
  return started;
}

// The phased extension's kernel: one side (RIGHT = false: left calls, true:
// right calls) of the tasks of one list.  The list is sorted by the side's
// query length, longest first: entries [0, n_long) have a query longer than
// short_q and run eight per wave (G = 16) or four (G = 32); the eight-per-wave
// form then runs the rest, [n_long, n), sixteen per wave in groups of eight
// lanes (short_q > 0; spec_sort2_scan left n_long in the list's counter word).
// A wave goes from the first run to the second on its own, when the first
// run's heads are dry: no launch and no barrier between them.  LDS is cut per
// wave (wave_lds bytes each, the larger of the two runs' needs), so a wave in
// the second run never touches a sibling's buffers of the first.
template <int G, int PMAX, bool K8, bool RIGHT>
__global__ void __launch_bounds__(kBlock) spec_side4_kernel(DevOpt o, DevRef ref, DevBatch b, SpecArgs a, int list,
                                                            int tb_bytes, int wave_lds, int short_q, int tb_short,
                                                            int short_fill) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* const wlds = lds + (size_t)(threadIdx.x >> 6) * (size_t)wave_lds;
  const int n = uni(__hip_atomic_load(&a.ctr[(RIGHT ? SPC_RCNT : SPC_LCNT) + list], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT));
  const FatTask* fl = (RIGHT ? a.ftaskR : a.ftask) + spec_list_off(list, b.n_chains, b.n_seeds);
  constexpr bool kShort = G == 16 && K8;  // the form with a short phase
  int n_long = n;
  if constexpr (kShort) {
    if (short_q > 0) {
      n_long = min(n, uni(__hip_atomic_load(&a.ctr[(RIGHT ? SPC_RLONG : SPC_LLONG) + list], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT)));
      // a short run that does not fill the grid's sixteen-per-wave slots
      // short_fill / 100 times over runs eight per wave as before (every wave
      // decides alike): see launch_side_pair
      const long long slots = (long long)gridDim.x * (kBlock / 64) * (128 / kShortG);
      if ((long long)(n - n_long) * 100 < slots * short_fill) n_long = n;
    }
  }
  const int hl = RIGHT ? kSpecRounds * kSpecBins + list : list;
  long long spec_cells = 0;
#ifdef BWAGPU_OCC_DIAG
  unsigned long long tw[6] = {0, 0, 0, 0, 0, 0}, occ[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  (void)side_loop<G, PMAX, K8, RIGHT>(o, ref, b, a, fl, n_long, a.qh + 8 * kQHStride * hl, wlds, tb_bytes, spec_cells,
                                      tw, occ);
#else
  (void)side_loop<G, PMAX, K8, RIGHT>(o, ref, b, a, fl, n_long, a.qh + 8 * kQHStride * hl, wlds, tb_bytes, spec_cells);
#endif
  if constexpr (kShort) {
    if (n_long < n) {
      int32_t* const hs = a.qh + kQHShort + 8 * kQHStride * hl;
      long long cells_s = 0;  // group-uniform over eight lanes, not sixteen: added on its own
#ifdef BWAGPU_OCC_DIAG
      const int ns = side_loop<kShortG, kShortPmax, true, RIGHT>(o, ref, b, a, fl + n_long, n - n_long, hs, wlds,
                                                                 tb_short, cells_s, tw, occ);
#else
      const int ns = side_loop<kShortG, kShortPmax, true, RIGHT>(o, ref, b, a, fl + n_long, n - n_long, hs, wlds,
                                                                 tb_short, cells_s);
#endif
      if ((threadIdx.x & (kShortG - 1)) == 0 && ns) {
        atomicAdd(&a.ctr[SPC_SHORT_N], ns);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), (unsigned long long)cells_s);
      }
    }
  }
#ifdef BWAGPU_OCC_DIAG
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 8; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + 32) + k, occ[k]);
    for (int k = 0; k < 4; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + 48) + k, tw[k]);
  }
#endif
  if ((threadIdx.x & (G - 1)) == 0 && spec_cells)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.ctr + SPC_SPEC64), (unsigned long long)spec_cells);
}


// kFuseSort: two launches, certificate + count and scan +
// scatter; a context without the certificate keeps the count kernel, three
void launch_side_sort(const ExtRound& r, int bin0, int nbins, int short_q, int short_fill) {
  const int fuse = (r.ss.fused & kFuseSort) ? 1 : 0;
  if (r.a.ung)
    hipLaunchKernelGGL(spec_ungapped_kernel, dim3(512, nbins), dim3(256), 0, r.st, r.o, r.ref, r.b, r.a, r.round, bin0,
                       short_fill == 0 ? short_q : 0, fuse);
  if (!(fuse && r.a.ung)) hipLaunchKernelGGL(spec_sort2_count, dim3(256, nbins), dim3(256), 0, r.st, r.b, r.a, r.round, bin0);
  if (!fuse)
    hipLaunchKernelGGL(spec_sort2_scan, dim3(2 * nbins), dim3(256), 0, r.st, r.a, r.round, bin0, nbins, short_q);
  hipLaunchKernelGGL(spec_sort2_scatter, dim3(256, nbins), dim3(256), 0, r.st, r.o, r.b, r.a, r.round, bin0, short_q,
                     fuse);
}

// the two side launches of the phased extension for one list: every left
// call, then every right call, G lanes per call.  The short phase's settings
// are the plan's (only the eight-per-wave form has one).
template <int G, int PMAX, bool K8>
static void launch_side_pair(const ExtRound& r, int list, const ExtPlan& p, int short_fill) {
  const size_t lds = (size_t)(kBlock / 64) * p.wave_lds;
  const int nb = resident_blocks(spec_side4_kernel<G, PMAX, K8, false>, lds);
  const int gr = r.round == 2 ? std::min(nb, 64) : std::min(nb, ext2_grid(1 << 30, true));
  if (!(G == 16 && K8)) short_fill = 0;
  hipLaunchKernelGGL((spec_side4_kernel<G, PMAX, K8, false>), dim3(gr), dim3(kBlock), lds, r.st, r.o, r.ref, r.b, r.a,
                     list, r.tb_bytes, (int)p.wave_lds, p.short_q, p.tb_short, short_fill);
  // the late right sides go on from the left launch's slots.  One launch per list, after that list's own left
  // launch, not one per round with grid.y = bins: ext_plan phases only the first bin today, and with two
  // phased bins a single launch would have to wait for the second list's left launch.
  // kFuseSettle: on the side stream, idle during an extension round, beside the right launch
  // and not ahead of it.  The two kernels never touch the same SeedExt slot: the right launch reads and
  // writes the slots of the tasks on the right list alone, this kernel those of the late tasks, and side_lists
  // puts a late task on no right list; both wait for the left launch, which wrote what either goes on from.
  // Both add their cells to SPC_SPEC64 atomically, the late kernel its own counters (SPC_UNGR_*) too.
  const bool beside = r.a.ungt && r.ss.side && (r.ss.fused & kFuseSettle);
  if (beside) {
    (void)hipEventRecord(r.ss.fork, r.st);
    (void)hipStreamWaitEvent(r.ss.side, r.ss.fork, 0);
    hipLaunchKernelGGL(spec_settle_right_kernel, dim3(256, 1), dim3(256), 0, r.ss.side, r.o, r.b, r.a, r.round,
                       list % kSpecBins);
    (void)hipEventRecord(r.ss.join, r.ss.side);
  } else if (r.a.ungt) {
    hipLaunchKernelGGL(spec_settle_right_kernel, dim3(256, 1), dim3(256), 0, r.st, r.o, r.b, r.a, r.round,
                       list % kSpecBins);
  }
  hipLaunchKernelGGL((spec_side4_kernel<G, PMAX, K8, true>), dim3(gr), dim3(kBlock), lds, r.st, r.o, r.ref, r.b, r.a,
                     list, r.tb_bytes, (int)p.wave_lds, p.short_q, p.tb_short, short_fill);
  if (beside) (void)hipStreamWaitEvent(r.st, r.ss.join, 0);
}

// the side kernels compiled are exactly these cases
void launch_side_bin(const ExtBin& k, const ExtRound& r, int list, const ExtPlan& p, int short_fill) {
  switch (ext_key(k.family, k.G, k.PMAX, k.K8)) {
    case ext_key(SIDE4, 16, 10, true): return launch_side_pair<16, 10, true>(r, list, p, short_fill);
    case ext_key(SIDE4, 32, 5, true): return launch_side_pair<32, 5, true>(r, list, p, short_fill);
    case ext_key(SIDE4, 32, 8, false): return launch_side_pair<32, 8, false>(r, list, p, short_fill);
    default: abort();  // ext_plan names no other side kernel (tests/cpp/ext_plan_asan.cpp)
  }
}

}  // namespace bwagpu
