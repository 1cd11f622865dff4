// pairsel.h — internal declarations of the primary-marking and pair-selection
// kernels (pairsel.hip) shared with the C ABI (capi.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"
#include "engine.h"

namespace bwagpu {

constexpr int kSelCap = BWAGPU_SEL_MAX_REGS;  // regions of a read / primary regions of a pair in LDS
constexpr int kSelMaxBlocks = 1024;           // grid bound of both kernels (one wave per block)

struct MarkArgs {
  int32_t n_reads;
  int32_t tmp;            // max(a + b, o_del + e_del, o_ins + e_ins)
  float mask_level;
  int64_t id0;
  const int64_t* reg_off;
  bwagpu_alnreg_t* regs;
  const int32_t* n;
  int32_t *n_pri, *status;
  bwagpu_alnreg_t* scratch;  // kSelCap records per block: the reordered read before it goes back
};
hipError_t launch_mark_primary(const MarkArgs& a, hipStream_t st);

struct PairSelArgs {
  int32_t n_pairs;
  int32_t a, b, tmp;      // mem_opt_t.a, .b, and tmp as above
  bwagpu_selopt_t so;
  int64_t pair_id0;
  bwagpu_pestat_t pes[4];
  const double* erfc_tab[4];  // per live orientation: .721 * log(2 erfc(|ns| / sqrt 2)) by dist - low
  const double* log_tab;      // log(k), k < log_n
  int32_t log_n;
  const int64_t* reg_off;
  bwagpu_alnreg_t* regs;
  const int32_t *n, *n_pri, *in_status;
  bwagpu_pairsel_t* sel;
  int32_t* out_mapq;
};
hipError_t launch_pair_select(const DevRef& ref, const PairSelArgs& a, hipStream_t st);

}  // namespace bwagpu
