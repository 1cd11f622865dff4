/* bwagpu_debug.h — tuning, test and profiling entry points of libbwagpu.so.
 *
 * Not part of the drop-in stage's interface (include/bwagpu.h): bwa-flow's
 * ChainsToRegionsGPU never calls them.  The tests use them to force kernel
 * forms and inject failures, and bench.py uses them to time the dominant
 * extension kernel (HIP events) and read the speculative path's counters.
 * The reference has no counterpart: it logs per-phase stage wall times
 * (src/fpga/FPGAPipeline.cpp:557-578, src/util.h:34-40).  Every entry here
 * leaves results unchanged.
 */
#ifndef BWAGPU_DEBUG_H
#define BWAGPU_DEBUG_H
#include "bwagpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning / tests: bwagpu_collect_intv runs each read on one lane until it has
   made `budget` bwt_extend calls (default 1024, about the 90th percentile of a
   150 bp read on a chr21-sized index), then hands it to a second kernel that
   runs it on a whole wave (backward search lane-parallel).  0 sends every
   read to the wave kernel.  Results do not depend on it. */
int bwagpu_debug_seed_budget(bwagpu_ctx_t *ctx, int32_t budget);

/* Tests: the device occurrence layout keeps 32-bit counts relative to
   superblocks of 2^shift positions (default 32: only indexes past 2^32
   positions, e.g. GRCh38's 6.2 G, have more than one).  A smaller shift
   (7..32) for the NEXT bwagpu_set_bwt makes a small index cross superblock
   boundaries, so that the superblock table and the relative counts are
   exercised on the golden fixtures.  Results do not depend on it. */
int bwagpu_debug_sup_shift(bwagpu_ctx_t *ctx, int32_t shift);

/* diagnostics: while dev_ptr != NULL every chain2aln launch on this device
   writes 8 x uint32 per read index r at dev_ptr[8r..8r+7]: start and end
   s_memrealtime (100 MHz, lo/hi), DP rows, DP cells, HW_ID, XCC_ID (the
   per-read kernels); the speculative path writes its selection passes
   (emulate, final, redo) at dev_ptr[8 (pass n_reads + r) ..]: start / end,
   seeds, regions, XCC_ID, shape — so the buffer needs 24 x n_reads words.
   With bwagpu_ctx_emu_finish on, a light read the emulate pass finished has
   its record under pass 0 (emulate) only.
   Not part of the reference interface (the reference logs stage wall times
   with getUs(), src/util.h:34-40). */
int bwagpu_debug_set_trace(bwagpu_ctx_t *ctx, void *dev_ptr);
/* tests of the caller's recovery path: after `after_n_waits` more successful
   bwagpu_chain2aln_wait calls, the next one returns `code` (e.g.
   BWAGPU_E_HANG, as a watchdog expiry does) with its batch left in flight */
int bwagpu_debug_fail_wait(bwagpu_ctx_t *ctx, int after_n_waits, int code);
/* tests of the contexts' lifetime: the grow-only device and pinned host buffers
   that all contexts of this process hold at the moment (*n) and their
   capacities' sum (*bytes).  Every such buffer belongs to a context, so a
   bwagpu_destroy brings both back to what they were before its bwagpu_create
   — without reading the device's free memory, which other processes change.
   The resident reference (pac, contig table) is not counted. */
int bwagpu_debug_live_buffers(int64_t *n, int64_t *bytes);

/* kernel timing (bench.py's roofline): after bwagpu_prof_start(ctx, n) the
   next n launches of the dominant extension kernel (the first length bin's
   extension kernel, one per extension round of a chain2aln batch) are
   bracketed by HIP events on the stream they run on; bwagpu_prof_read waits
   for them and returns the summed kernel time and the number of launches
   timed; bwagpu_prof_intervals returns each launch's [start, end] in ms from
   the first event, so that launches of different streams that overlap can be
   counted once (their union).  bwagpu_prof_start(ctx, 0)
   turns timing off.  Diagnostics; the reference prints per-phase stage times
   instead (src/fpga/FPGAPipeline.cpp:557-578). */
int bwagpu_prof_start(bwagpu_ctx_t *ctx, int max_launches);
/* diagnostics: the speculative path's counters of the last device-entry batch
   on `stream` (waits for it): out[0..2] extension tasks of rounds A/B/C,
   out[3] DP cells of every computed task (used or not), out[4] extensions the
   redo pass computed inline, out[5] reads with > 64 seeds, out[6] reads left
   to the redo pass, out[7] seeds of heavy reads with pair matrices */
int bwagpu_debug_spec_counters(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* diagnostics of a library built with -DBWAGPU_OCC_DIAG (else
   BWAGPU_E_UNSUPPORTED): the packed extension kernels' occupancy over the last
   device-entry batch on `stream`, out[0..7] = generations (extend_quad calls
   of a wave), rows run, call-slot rows, live call rows, call-slot cells, live
   call-slot cells, cells inside the live calls' queries, computed cells;
   out[8..11] = the waves' shader-clock cycles in task starts + claims, call
   setup, the DP (extend_quad) and the result advance, out[12..13] = of the
   first, the claims' and the task records' own (out: 14 entries) */
int bwagpu_debug_occupancy(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* diagnostics: the per-seed extension records (48 B each: rb, re, qb, qe,
   score, truesc, w, cells, rows, calls + 1; calls == 0: not computed) of the
   last device-entry batch on `stream`, n = its seed count */
int bwagpu_debug_spec_ext(bwagpu_ctx_t *ctx, void *stream, void *host_out, int32_t n);
int bwagpu_prof_read(bwagpu_ctx_t *ctx, double *total_ms, int32_t *launches);
/* tests / A-B: the extension kernel of the first two read-length bins — 0
   (default) packed 16-bit DP where every score of the bin fits (else two per
   wave): eight seeds per wave in the first bin, four in the second; 1 two
   seeds per wave (32-bit DP); 2 four seeds per wave in both bins.  Results do
   not depend on it.  bwagpu_ctx_ext_form sets one context's form;
   bwagpu_debug_ext_form sets the form contexts created afterwards start with.
   Both return the previous form; form < 0 only queries. */
int bwagpu_debug_ext_form(int form);
int bwagpu_ctx_ext_form(bwagpu_ctx_t *ctx, int form);
/* the short-side threshold of the eight-per-wave phased extension (form 0,
   first length bin): a task side whose query has 1 .. q bases runs in groups
   of eight lanes, sixteen calls per wave, after the longer sides of its launch
   (the same kernel; no further launch).  q = 0: off, every side eight per
   wave; 1 .. 63 otherwise (a larger q counts as 63); q < 0 only queries.
   Returns the previous value.  A context starts with BWAGPU_EXT_SHORT_Q if
   set, else the compiled default.  A launch whose short buffers would not fit
   the workgroup's LDS runs with 0.  Results do not depend on it. */
int bwagpu_ctx_ext_short(bwagpu_ctx_t *ctx, int q);
/* ... and the smallest short run that takes the short phase, in percent of the
   launch's sixteen-per-wave call slots (16 x the grid's waves): a smaller run
   leaves fewer waves busy for longer generations than eight per wave would, so
   it runs eight per wave as before.  0: every short run takes the short phase
   (tests of small batches).  percent < 0 only queries; returns the previous
   value.  A context starts with BWAGPU_EXT_SHORT_FILL if set, else the compiled
   default. */
int bwagpu_ctx_ext_short_fill(bwagpu_ctx_t *ctx, int percent);
/* the packed light selection (default on): spec_select_light runs the reads
   with at most eight seeds and eight chains eight per wave, in groups of eight
   lanes; 0: every light read has a wave of its own.  on < 0 only queries;
   returns the previous setting.  A context starts with BWAGPU_LIGHT_PACK if
   set, else the compiled default.  Results do not depend on it. */
int bwagpu_ctx_light_pack(bwagpu_ctx_t *ctx, int on);
/* diagnostics of the last device-entry batch on `stream` (waits for it), out: 9
   entries.  out[0] = the task sides run in the short phase, all rounds
   (bwagpu_debug_spec_counters' eight words are a fixed layout its callers size
   their buffers by, so this counter has an entry of its own); out[1..4] = round
   A's first-bin side lists: left sides, of them longer than the threshold (0
   with the short phase off), right sides, of them longer; out[5..8] = round B's */
int bwagpu_debug_spec_short(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* the ungapped certificate (default on; BWAGPU_UNGAPPED=0 starts contexts
   with it off): a side of a phased extension task whose diagonal loses less
   than the cheapest gap open is settled when the side lists are sorted, from
   the diagonal's running sums alone, and never enters a list.
   Regions are identical either way and the ksw_extend2 calls are counted as
   before; a settled call counts no rows and no cells.  It acts only while the
   row bound (below) is on, the switch under which calls may end early.  With
   bwagpu_ctx_ext_short_fill at 0 (every short side takes the short phase) the
   sides up to the short threshold are left to that phase.  on < 0 only
   queries; returns the previous setting. */
int bwagpu_ctx_ungapped(bwagpu_ctx_t *ctx, int on);
/* diagnostics of the last device-entry batch on `stream` (waits for it), out:
   12 entries, four per round A, B, C: the sides the certificate settled, the
   sum of their query lengths, and the left and the right sides that stayed on
   the phased lists */
int bwagpu_debug_spec_ungapped(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* late-settled right sides (default on; BWAGPU_UNGAPPED_RIGHT=0 starts
   contexts with it off; acts only while the certificate does): a right side
   that holds the certificate behind a left side that needs the DP enters no
   list either; a small kernel after the list's left launch finishes its seed
   from the slot that launch wrote.  0: such a side runs the DP
   on the right list.  Regions and call counts are identical either way.
   on < 0 only queries; returns the previous setting. */
int bwagpu_ctx_ungapped_right(bwagpu_ctx_t *ctx, int on);
/* diagnostics of the last device-entry batch on `stream` (waits for it), out:
   6 entries, two per round A, B, C: the right sides settled after the left
   launch and the sum of their query lengths; all 0 with either switch off */
int bwagpu_debug_spec_ungapped_right(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* the emulate pass finishes decided light reads (default on;
   BWAGPU_EMU_FINISH=0 starts contexts with it off): a light read the emulate
   selection pass leaves no round-B task has every extension result the final
   pass would use, so that pass writes its regions itself and lists the other
   light reads; the final light pass then takes only the listed reads
   (DESIGN.md §25).  0: the final pass takes every light read.  Regions and the
   cell, row and call counters are identical either way.  on < 0 only queries;
   returns the previous setting. */
int bwagpu_ctx_emu_finish(bwagpu_ctx_t *ctx, int on);
/* diagnostics of the last device-entry batch on `stream` (waits for it), out:
   4 entries: the narrow light reads (at most eight seeds and eight chains) the
   emulate pass finished, the wider ones, the light reads it listed for the
   final pass, and the batch's light reads as that pass counts them; all 0 with
   the switch off or for a batch without chains */
int bwagpu_debug_spec_finish(bwagpu_ctx_t *ctx, void *stream, int64_t *out);
/* the packed extension kernels' row bound (default on): a ksw_extend2 call
   ends once no later target row can change its score, qle, tle, gtle, gscore
   or max_off (every later cell is bounded by a stored value plus max(mat) per
   query column still ahead of it).  Results are identical either way; with
   it off the cell and row counters (bwagpu_last_stats) count every row
   ksw_extend2 (ksw.c:380-479) evaluates.  Returns the previous setting;
   on < 0 only queries. */
int bwagpu_ctx_row_bound(bwagpu_ctx_t *ctx, int on);
/* the first length bin's extension kernel this context launches for reads of
   up to lq_max bases, as ext_plan (bwa-flow_amd/csrc/spec_plan.h, which holds
   the table) decides it: 18 / 14 / 15 = the phased pair
   spec_side4_kernel<G,PMAX,K8,{false,true}> (every left call, then every right
   call) eight per wave <16,10,true>, four per wave with the 8-bit row-max key
   <32,5,true>, four per wave <32,8,false>; 2 = two per wave, 32-bit
   (spec_ext2_kernel<5>) */
int bwagpu_debug_ext_kernel(bwagpu_ctx_t *ctx, int32_t lq_max);
/* 1 if work on the two streams (hipStream_t, on the current device) runs
   concurrently, 0 if they share a hardware queue (HIP maps the process's
   streams onto GPU_MAX_HW_QUEUES queues; streams on one queue run in
   submission order), < 0 on error.  Measured: a ~150 us spin on a, then an
   empty kernel on b.  Callers that drive several batches at once should give
   them concurrent streams (bench.py's caller_streams). */
int bwagpu_streams_concurrent(void *a, void *b);
/* tests: the first round's plan of every later bwagpu_mate_rescue* call leaves
   every k-th ksw_align2 task out of the result table (0 = off), the only way
   to reach the retry round and BWAGPU_RESCUE_UNFINISHED on demand.  Results do
   not depend on it while max_rounds >= 2. */
int bwagpu_debug_rescue_drop(bwagpu_ctx_t *ctx, int32_t k);
/* timing (tools_dev/rescue_bench.py): the last bwagpu_mate_rescue* call of this
   context by HIP events on its stream (waits for it), summed over its rounds:
   out[0] ms from a round's start to the end of its plan (the counting pass,
   the scans, the wait for the task count and the emitting pass), out[1] the
   batched ksw_align2, out[2] the replay, out[3] the rounds run */
int bwagpu_debug_rescue_times(bwagpu_ctx_t *ctx, double *out);
/* timing (tools_dev/reg2aln_device_bench.py).  The first use switches the timing
   of this context's later bwagpu_reg2aln_device calls on (two events and two
   clock readings per call; off by default) and returns zeros.  Afterwards: the
   last such call (waits for it): out[0] ms the host waited at the bin table's
   read-back, out[1] ms by HIP events on its stream from before the first bin
   launch to after the last one's end, out[2] ms the host spent in the call,
   out[3] the call's job count */
int bwagpu_debug_reg2aln_times(bwagpu_ctx_t *ctx, double *out);
/* timing (tools_dev/sam_text_bench.py): one step of bwagpu_sam_text_device alone,
   asynchronous on stream: 0 the count pass, 1 the scan, 2 the write pass.  The
   steps share the context's scratch, so they only make sense as 0, 1, 2 in order
   on one stream, each between the caller's events */
int bwagpu_debug_sam_text_step(bwagpu_ctx_t *ctx, const bwagpu_samtext_t *t, int32_t n_reads, int32_t step,
                               void *stream);
int bwagpu_prof_intervals(bwagpu_ctx_t *ctx, double *start_ms, double *end_ms, int32_t max, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* BWAGPU_DEBUG_H */
