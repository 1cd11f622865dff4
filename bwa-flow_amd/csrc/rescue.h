// rescue.h — internal declarations of the insert-size statistics and the mate
// rescue kernels (rescue.hip) shared with the C ABI (capi.hip).  Not part of
// the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"
#include "engine.h"

namespace bwagpu {

// rounds of plan -> align2 -> apply one call may run (bwagpu_pairopt_t.max_rounds)
constexpr int kRescueMaxRounds = 8;
// a slot (pair, side i, candidate k, orientation r) of the result table holds
// its task as round << kRescueIdxBits | index in that round's list, or:
constexpr int kRescueIdxBits = 26;
enum { RS_NONE = -1, RS_WANTED = -3 };  // not computed / asked for by the replay
// per-pair state between rounds
enum { RP_DONE = 0, RP_PENDING = 1 };
// counter words (int32): RC_PENDING zeroed per round, RC_USED per call
enum { RC_PENDING = 0, RC_USED = 1, RC_WORDS = 4 };

struct PestatArgs {
  int32_t n_pairs;        // n_reads >> 1
  int32_t cap;            // entries per orientation list: a power of two >= max(n_pairs, 1)
  bwagpu_pairopt_t po;
  const int64_t* reg_off;
  const bwagpu_alnreg_t* regs;
  const int32_t* n;
  uint64_t* isize;        // [4][cap]
  int32_t* cnt;           // [4], zeroed
  bwagpu_pestat_t* pes;   // [4]
};
hipError_t launch_pestat(const DevOpt& o, const DevRef& ref, const PestatArgs& a, hipStream_t st);

struct RescueArgs {
  int32_t n_pairs, round, drop;  // drop: the plan leaves every drop-th task of this round out (0 = none)
  bwagpu_pairopt_t po;
  const bwagpu_pestat_t* pes;
  const int64_t* seq_off;
  const uint8_t* seq;
  const int64_t* reg_off;
  const bwagpu_alnreg_t* regs;
  const int32_t* n;
  const int64_t* out_off;  // [n_reads + 1]
  bwagpu_alnreg_t* out_regs;
  int32_t *out_n, *status, *n_sw;
  // work arrays
  int32_t* pstate;         // per pair, RP_*
  int32_t* nb0;            // per pair: candidates of read 0, min(b[0].n, max_matesw)
  int32_t* nslot;          // per pair: 4 x candidates of both reads
  const int64_t* slot_off; // its scan
  int32_t* tab;            // per slot
  int32_t *ntask, *tbytes; // per pair, this round
  const int64_t *task_off, *tb_off;  // their scans
  uint8_t* qpool;          // the reads as given, then reverse-complemented at + rc_base
  int64_t rc_base;
  bwagpu_align2_task_t* tasks;  // this round's list
  uint8_t* tpool;
  const bwagpu_kswr_t* res[kRescueMaxRounds];
  int32_t* ctr;            // RC_* words
};
// both strands of every read into qpool
hipError_t launch_rescue_pool(const RescueArgs& a, hipStream_t st);
// candidates per pair -> nb0, nslot; pstate = RP_PENDING, status = 0
hipError_t launch_rescue_init(const DevOpt& o, const RescueArgs& a, hipStream_t st);
// emit = false: ntask / tbytes of this round; true: the tasks, their windows and the table
hipError_t launch_rescue_plan(const DevOpt& o, const DevRef& ref, const RescueArgs& a, bool emit, hipStream_t st);
hipError_t launch_rescue_apply(const DevOpt& o, const DevRef& ref, const RescueArgs& a, hipStream_t st);

}  // namespace bwagpu
