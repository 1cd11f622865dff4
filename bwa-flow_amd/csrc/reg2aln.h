// reg2aln.h — internal declarations of the batched mem_reg2aln CIGAR kernels
// (reg2aln.hip) shared with the C ABI (capi_tasks.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bwagpu.h"
#include "engine.h"

namespace bwagpu {

// (the buckets, kR2CD, r2_bucket_of and the matrix classes: pure.h)

struct R2AArgs {
  const bwagpu_reg2aln_task_t* tasks;
  const uint8_t* qpool;
  const int32_t* list;  // job ids of this bin, in processing order
  int n;                // jobs in list
  int max_ops, max_md;
  bwagpu_aln_t* out;
  uint32_t* cigar;
  char* md;
  uint8_t* zglob;   // NULL: direction matrix in LDS; else per-wave HBM slices of zstride bytes
  int64_t zstride;
  int qcap, rcap, ocap;  // per-wave LDS: query bytes, reference bytes, CIGAR-run words
  int lds_per_wave;      // qcap + rcap + 4 ocap (+ the LDS matrix), 16-aligned
  int64_t* stats;        // ST_* words, may be NULL
  const int32_t* dev_n;  // NULL, or the bin's job count in device memory: the kernel runs min(n, *dev_n) jobs
};

// wpb: waves per workgroup (1 for LDS-heavy bins: finer LDS packing per CU)
int r2_resident_waves(int cd, size_t lds_per_block, int wpb);
hipError_t launch_reg2aln(int cd, const DevOpt& o, const DevRef& ref, const R2AArgs& a, int n_blocks, int wpb,
                          hipStream_t st);


// bwagpu_reg2aln_device: the bin table reg2aln_classify_kernel fills, as int32 words
//   [4 b .. 4 b + 3]      bin b (= bucket * 3 + cls): jobs, longest query, longest window, largest matrix
//   [kR2TabClass + kR2CostClasses b + c] jobs of bin b in cost class c
//   [kR2TabJobs], [kR2TabRefused]  the call's job count (min(n_cap, *dev_n_tasks)), refused jobs
constexpr int kR2TabClass = 4 * kR2Bins, kR2TabJobs = kR2TabClass + kR2Bins * kR2CostClasses,
              kR2TabRefused = kR2TabJobs + 1, kR2TabWords = kR2TabJobs + 8;
struct R2Offsets {
  int32_t at[kR2Bins * kR2CostClasses];  // first list slot of every (bin, cost class)
};
// keys[k]: bin * kR2CostClasses + cost class, or -1 for a job that is refused or past the job count
hipError_t launch_reg2aln_classify(const DevOpt& o, int64_t l_pac, int64_t qpool_len, int n_cap,
                                   const int32_t* dev_n_tasks, const bwagpu_reg2aln_task_t* tasks, int32_t* keys,
                                   bwagpu_aln_t* out, int32_t* table, hipStream_t st);
// cursors: kR2Bins * kR2CostClasses zeroed words
hipError_t launch_reg2aln_scatter(int n_cap, const int32_t* keys, const R2Offsets& off, int32_t* cursors,
                                  int32_t* list, hipStream_t st);

// bwagpu_reg2aln_jobs_device: jobs of the selected regions in (read, k) order.
// block_sums: (n_reads + 255) / 256 words of scratch.
hipError_t launch_reg2aln_jobs(int n_reads, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                               const int32_t* select, const int64_t* seq_off, int job_cap,
                               bwagpu_reg2aln_task_t* tasks, int32_t* job_of, int32_t* n_jobs, int32_t* block_sums,
                               hipStream_t st);

}  // namespace bwagpu
