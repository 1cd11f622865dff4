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

}  // namespace bwagpu
