// samtext.hip — the SAM stage after bwagpu_pair_select_device.
//
//   xa_select_kernel: the selection of mem_gen_alt (bwa/bwamem_extra.c:98-118,
//   called at bwamem_pair.c:337-340 and bwamem.c:1026-1027): which regions of a
//   read become hits of an XA string and which record carries that string, and
//   from it the regions that need a CIGAR job.
//
// One wave per read, four reads per workgroup, three passes over the read's
// regions with lane i, i + 64, ... on region i.  Every loop is bounded by the
// read's count n, loaded once; every index into the read's span is below n.
// The two output arrays double as the passes' scratch, so the kernel needs no
// memory of its own and no bound on n:
//   1. job_select[i] = get_pri_idx(i)                        (reads regs only)
//   2. xa_of[i]      = that index if its string is within the caps and printed
//                      (reads job_select of the whole read, writes xa_of[i])
//   3. job_select[i] = 0 / -1                                (reads xa_of[i] only)
// A pass reads what other lanes (and, past 64 regions, the same lane) wrote in
// the pass before, so a workgroup barrier stands between them; it is reached by
// all four waves, which carry n = 0 when they have no read.
#include <hip/hip_runtime.h>

#include "pure.h"
#include "samtext.h"

namespace bwagpu {

namespace {
constexpr int kXaReadsPerBlock = 4;
}

__global__ void __launch_bounds__(64 * kXaReadsPerBlock) xa_select_kernel(XaSelArgs g) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t r64 = (int64_t)blockIdx.x * kXaReadsPerBlock + (threadIdx.x >> 6);
  const bool live = r64 < g.n_reads;
  const int r = live ? (int)r64 : 0;
  const int n = live ? g.n[r] : 0;
  const int64_t base = live ? g.reg_off[r] : 0;
  const bwagpu_alnreg_t* a = g.regs + base;
  const int32_t* mapq = g.out_mapq + base;
  int32_t* xa_of = g.xa_of + base;
  int32_t* job_select = g.job_select + base;
  bool done = false;
  int mate = -1;  // the no-pairing branch's mate record (bwamem_pair.c:375-384)
  if (live) {
    const bwagpu_pairsel_t& s = g.sel[r >> 1];
    done = s.status == BWAGPU_SEL_DONE;
    if (done && s.branch == BWAGPU_SEL_NO_PAIRING) mate = s.z[r & 1];
  }

  for (int i = lane; i < n; i += 64) job_select[i] = done ? xa_pri_idx(g.drop_ratio, a, n, i) : -1;
  __syncthreads();

  for (int i = lane; i < n; i += 64) {
    const int k = job_select[i];
    int x = -1;
    if (k >= 0) {  // k < n (xa_pri_idx)
      int cnt = 0;
      bool has_alt = false;
      for (int j = 0; j < n; ++j)
        if (job_select[j] == k) {
          ++cnt;
          has_alt |= (a[j].n_comp_is_alt >> 30) != 0;
        }
      // a string is printed only on an emitted record (h[i].XA, g[i].XA, q->XA)
      if (!xa_over_cap(cnt, has_alt, g.max_hits, g.max_hits_alt) && mapq[k] >= 0) x = k;
    }
    xa_of[i] = x;
  }
  __syncthreads();

  for (int i = lane; i < n; i += 64) job_select[i] = done && (mapq[i] >= 0 || xa_of[i] >= 0 || i == mate) ? 0 : -1;
}

hipError_t launch_xa_select(const XaSelArgs& a, hipStream_t st) {
  const unsigned nb = (unsigned)(((int64_t)a.n_reads + kXaReadsPerBlock - 1) / kXaReadsPerBlock);
  hipLaunchKernelGGL(xa_select_kernel, dim3(nb), dim3(64 * kXaReadsPerBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace bwagpu
