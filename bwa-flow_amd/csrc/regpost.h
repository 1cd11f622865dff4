// regpost.h — internal declarations of the region post-processing kernel
// (regpost.hip) shared with the C ABI (capi.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"
#include "engine.h"

namespace bwagpu {

// reference bases one patch DP holds in LDS: mem_patch_reg's window is
// b->re - a->rb, which mem_chain2aln's regions keep below ~3 x (read + band)
constexpr int kPostRefCap = 4096;
// set in stats[ST_ERR] when a patch candidate passed the gates but could not
// be evaluated (window over kPostRefCap, or qb/qe outside the read)
enum { ERR_POST = 8 };

struct RegPostArgs {
  int32_t n_reads, flags;
  int64_t id0;            // mem_mark_primary_se's id of read 0
  bwagpu_postopt_t po;
  int32_t opt_b;          // mem_opt_t.b (mem_mark_primary_se_core's tmp)
  const int64_t* seq_off;
  const uint8_t* seq;
  const int64_t* reg_off;         // read r's span starts at regs[reg_off[r]]; NULL: the slot layout
  const int32_t *rco, *cso;       // ... regs[cso[rco[r]]]
  bwagpu_alnreg_t* regs;
  int32_t* n;
  const uint8_t* alt;     // per-contig ALT flags, NULL = none
  int64_t* stats;         // ST_CALLS += patch DPs, ST_ERR |= ERR_POST; may be NULL
};

hipError_t launch_regpost(const DevOpt& o, const DevRef& ref, const RegPostArgs& a, hipStream_t st);

}  // namespace bwagpu
