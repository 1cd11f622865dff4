// samtext.h — internal declarations of the kernels behind the SAM stage's last
// steps (samtext.hip) shared with the C ABI (capi_tasks.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"

namespace bwagpu {

// bwagpu_xa_select_device: mem_gen_alt's selection over regions in device memory
struct XaSelArgs {
  int32_t n_reads;
  int32_t max_hits, max_hits_alt;
  double drop_ratio;  // the float option widened, as get_pri_idx's parameter holds it
  const int64_t* reg_off;
  const bwagpu_alnreg_t* regs;
  const int32_t* n;
  const bwagpu_pairsel_t* sel;
  const int32_t* out_mapq;
  int32_t *xa_of, *job_select;
};
hipError_t launch_xa_select(const XaSelArgs& a, hipStream_t st);

// bwagpu_sam_text_device: the caller's struct and the call's scratch: the rg_id's
// bytes, per read the bytes of its lines, per 256 reads their sum
struct SamTextArgs {
  bwagpu_samtext_t t;
  int32_t n_reads, rg_len;
  const char* rg;
  int32_t* len;
  int64_t* sums;
};
struct SamRgBytes {
  char c[BWAGPU_SAM_MAX_RG + 1];
};
inline size_t sam_text_scratch_bytes(int32_t n_reads) {  // rg | sums | len
  return 256 + sizeof(int64_t) * (((size_t)n_reads + 255) / 256) + sizeof(int32_t) * (size_t)n_reads;
}
// the three steps on st: count, scan, write.  scratch: sam_text_scratch_bytes(n_reads), 8-aligned
hipError_t launch_sam_text(const bwagpu_samtext_t& t, int32_t n_reads, const SamRgBytes& rg, int32_t rg_len,
                           void* scratch, hipStream_t st);
// one step alone, for the timing tool: 0 count, 1 scan, 2 write
hipError_t launch_sam_text_step(int step, const bwagpu_samtext_t& t, int32_t n_reads, const SamRgBytes& rg,
                                int32_t rg_len, void* scratch, hipStream_t st);

}  // namespace bwagpu
