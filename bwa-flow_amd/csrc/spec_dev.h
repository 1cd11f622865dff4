// spec_dev.h — what the two translation units of the speculative
// mem_chain2aln share (spec.hip: prep kernels, task kernels, selection passes
// and the round structure; spec_side.hip: the phased extension): device
// helpers that both inline, and the side launchers' declarations.  Internal.
#pragma once
#include "ksw_dev.h"

namespace bwagpu {

// The selection and bookkeeping kernels are latency-bound chains that share
// CUs with the other caller stream's persistent extension kernel; at wave
// priority 3 their instructions issue ahead of its (priority 0) waves.
__device__ __forceinline__ void sel_prio() { __builtin_amdgcn_s_setprio(3); }

// the heavy reads' pair matrices (spec_reads_kernel hands them out, the selection reads them):
// rows are triangular: row k holds words w < ceil(k / 64) (only seeds j < k
// count); tri_off(k) = sum over i < k of ceil(i / 64)
__host__ __device__ inline int64_t tri_off(int k) {
  if (k <= 1) return 0;
  const int64_t q = (k - 1) >> 6;
  return 32 * q * (q + 1) + (int64_t)(k - 1 - 64 * q) * (q + 1);
}

// ---------------------------------------------------------------- target rows
// Both target windows of the half's seed into its LDS rows (fill_two on 32
// lanes: 4 loads per side per lane in flight, 128 rows per side per pass).
template <int G = 32>
__device__ __forceinline__ void fill_two_half(uint8_t* tbl, int64_t x0l, int nl, uint8_t* tbr, int64_t x0r, int nr,
                                              const DevRef& ref) {
  const int r = (int)(threadIdx.x & (G - 1));
  const int64_t two1 = (ref.l_pac << 1) - 1;
  const int n = max(nl, nr);
  for (int base = 0; base < n; base += 4 * G) {
    uint32_t raw[8];
    int sh[8], kk[8];
    bool rev[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const bool left = m < 4;
      const int nn = left ? nl : nr;
      const int k = min(base + (m & 3) * G + r, max(nn - 1, 0));
      kk[m] = k;
      const int64_t x = left ? x0l - k : x0r + k;
      rev[m] = x >= ref.l_pac;
      int64_t f = rev[m] ? two1 - x : x;
      f = f < 0 ? 0 : (f >= ref.l_pac ? ref.l_pac - 1 : f);  // only for an empty side (nn == 0)
      raw[m] = ref.pac[f >> 2];
      sh[m] = (int)((~f & 3) << 1);
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int bse = (raw[m] >> sh[m]) & 3;
      const uint8_t v = (uint8_t)(rev[m] ? 3 - bse : bse);
      if (m < 4) {
        if (nl > 0) tbl[kk[m]] = v;
      } else {
        if (nr > 0) tbr[kk[m]] = v;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The same gather in ONE memory round trip (the packed kernels' task starts):
// lane r of the group takes rows [r R, r R + R) of each side, R = ceil(n / G)
// <= 32, i.e. a run of <= 32 consecutive bases of one strand, and loads the
// three aligned words of the pac that hold them (<= 9 bytes from a word
// boundary); each row's base is a 2-bit field of those words.  fill_two_half
// takes 4 rows per side per lane per pass, one dependent round trip per pass
// (5-6 for a 150 bp read's windows).  A run that leaves the pac's last 12
// bytes, or would straddle the two strands (a chain window never does), takes
// the per-row loads of fill_two_half's kind.
template <int G>
__device__ __forceinline__ void fill_side_run(uint8_t* tb, int64_t x0, int dir, int k0, int k1, const DevRef& ref,
                                              int64_t pac_bytes) {
  if (k1 <= k0) return;
  const int64_t two1 = (ref.l_pac << 1) - 1;
  const int64_t xa = x0 + (int64_t)dir * k0, xb = x0 + (int64_t)dir * (k1 - 1);
  const bool rev = xa >= ref.l_pac;
  const int64_t fa = rev ? two1 - xa : xa, fb = rev ? two1 - xb : xb;
  const int64_t fmin = fa < fb ? fa : fb;
  const int64_t w0 = (fmin >> 2) & ~(int64_t)3;  // first byte of the aligned words
  const bool fast = (xb >= ref.l_pac) == rev && fmin >= 0 && (fa > fb ? fa : fb) < ref.l_pac && w0 + 12 <= pac_bytes;
  const int df = (dir > 0) == !rev ? 1 : -1;  // f along the run
  if (fast) {
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(ref.pac + w0);
    const uint32_t d0 = pw[0], d1 = pw[1], d2 = pw[2];
    const int o0 = (int)(fa - (w0 << 2));  // the first row's base offset in the 48 loaded bases
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      if (k0 + j >= k1) break;
      const int o = o0 + df * j;
      const uint32_t w = o < 16 ? d0 : (o < 32 ? d1 : d2);
      const int bit = ((o >> 2) & 3) * 8 + 6 - 2 * (o & 3);
      const uint32_t bse = (w >> bit) & 3u;
      tb[k0 + j] = (uint8_t)(rev ? 3u - bse : bse);
    }
  } else {
    for (int k = k0; k < k1; ++k) {
      const int64_t x = x0 + (int64_t)dir * k;
      const bool rv = x >= ref.l_pac;
      int64_t f = rv ? two1 - x : x;
      f = f < 0 ? 0 : (f >= ref.l_pac ? ref.l_pac - 1 : f);
      const int bse = (ref.pac[f >> 2] >> ((~f & 3) << 1)) & 3;
      tb[k] = (uint8_t)(rv ? 3 - bse : bse);
    }
  }
}

template <int G>
__device__ __forceinline__ void fill_two_fast(uint8_t* tbl, int64_t x0l, int nl, uint8_t* tbr, int64_t x0r, int nr,
                                              const DevRef& ref) {
  const int n = max(nl, nr);
  const int R = (n + G - 1) / G;
  if (R > 32) {  // options with bands wider than the packed kernels' defaults
    fill_two_half<G>(tbl, x0l, nl, tbr, x0r, nr, ref);
    return;
  }
  const int r = (int)(threadIdx.x & (G - 1));
  const int64_t pac_bytes = (ref.l_pac >> 2) + 1;  // bwa.c:281-282
  const int k0 = r * R;
  fill_side_run<G>(tbl, x0l, -1, k0, min(k0 + R, nl), ref, pac_bytes);
  fill_side_run<G>(tbr, x0r, 1, k0, min(k0 + R, nr), ref, pac_bytes);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G = 32>
__device__ __forceinline__ void store_ext_half(SeedExt* dst, const SeedExt& e) {
  static_assert(G >= 12 || G == 8, "a SeedExt is 12 words");
  const int d = (int)(threadIdx.x & (G - 1));
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&e);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) v = d == k ? w[k] : v;
  if constexpr (G == 8) {  // eight lanes: words 0-7, then words 8-11 on the first four
    reinterpret_cast<uint32_t*>(dst)[d] = v;
    uint32_t u = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) u = d == k ? w[8 + k] : u;
    if (d < 4) reinterpret_cast<uint32_t*>(dst)[8 + d] = u;
  } else {
    if (d < 12) reinterpret_cast<uint32_t*>(dst)[d] = v;
  }
}

#ifdef BWAGPU_OCC_DIAG
// Occupancy of one extend_quad generation (a diagnostic build's counters,
// bwagpu_debug_occupancy): the wave runs rows until its longest call ends and
// CPL x G columns per call for its longest query; of those call-slot cells,
// the ones of calls that already ended, the ones beyond a live call's query,
// outside ksw's band, and the cells computed.  int64 counters at ctr words
// 32..47: generations, rows run, call-slot rows, live call rows, slot cells,
// live slot cells, query cells, computed cells.
template <int G>
__device__ __forceinline__ void occ_diag(unsigned long long* acc, const QCall& ca, const QCall& cb, const Tally32& ta,
                                         const Tally32& tb) {
  int qm = 0, rm = 0;
  long long lr = 0, lq = 0, cc = 0;
#pragma unroll
  for (int g = 0; g < 64; g += G) {
    const int qa = __builtin_amdgcn_readlane(ca.qlen, g), qb = __builtin_amdgcn_readlane(cb.qlen, g);
    const int ra = __builtin_amdgcn_readlane(ta.rows, g), rb = __builtin_amdgcn_readlane(tb.rows, g);
    qm = max(qm, max(qa, qb));
    rm = max(rm, max(ra, rb));
    lr += ra + rb;
    lq += (long long)ra * (qa + 1) + (long long)rb * (qb + 1);
    cc += __builtin_amdgcn_readlane(ta.cells, g) + __builtin_amdgcn_readlane(tb.cells, g);
  }
  const int cpl = (qm + G) / G;
  // summed per wave in registers, added to ctr words 32.. once at the kernel's end
  // (atomics here would put their round trips on the next generation start)
  acc[0] += 1ull;
  acc[1] += (unsigned long long)rm;
  acc[2] += (unsigned long long)rm * (2 * 64 / G);
  acc[3] += (unsigned long long)lr;
  acc[4] += (unsigned long long)rm * 128ull * cpl;
  acc[5] += (unsigned long long)lr * G * cpl;
  acc[6] += (unsigned long long)lq;
  acc[7] += (unsigned long long)cc;
}
#endif

// the task's FatTask record (engine.h): its seed, its chain's window, its read
__device__ __forceinline__ FatTask fat_task(const DevBatch& b, const SpecArgs& a, int2 tk) {
  const bwagpu_seed_t sd = a.prog[tk.x];
  const ChainWin cw = a.win[tk.y];
  const int rd = a.chain_read[tk.y];
  FatTask f;
  f.rbeg = sd.rbeg;
  f.qoff = b.seq_off[rd];
  f.pos = tk.x;
  f.dlo = (int32_t)(sd.rbeg - cw.lo);
  f.dhi = (int32_t)(cw.hi - sd.rbeg);
  const int lq = (int)(b.seq_off[rd + 1] - f.qoff);
  f.qls = (uint32_t)sd.qbeg | (uint32_t)sd.len << 10 | (uint32_t)lq << 20;
  return f;
}


// ---------------------------------------------------------------- launchers
// what the extension launches of one round share
struct ExtRound {
  const DevOpt& o;
  const DevRef& ref;
  const DevBatch& b;
  const SpecArgs& a;
  int round, tb_bytes;
  hipStream_t st;
  const SpecStreams& ss;
};
// the grid of an extension kernel on its persistent queue (spec.hip)
int ext2_grid(int nb, bool packed);
// the phased pair SIDE4 (spec_side.hip): a bin's lists, one per side in its
// query length order (spec_sort2_*), and its two launches as ext_plan
// (spec_plan.h) names the kernel `k`
void launch_side_sort(const ExtRound& r, int bin0, int nbins, int short_q, int short_fill);
void launch_side_bin(const ExtBin& k, const ExtRound& r, int list, const ExtPlan& p, int short_fill);
constexpr int ext_key(int family, int g, int pmax, bool k8) { return ((family * 64 + g) * 32 + pmax) * 2 + (k8 ? 1 : 0); }

}  // namespace bwagpu
