/*
 * bwagpu.h — C ABI of the MI355X seed-extension engine.
 *
 * This is the drop-in boundary that takes the place of bwa-flow's FPGA
 * Smith-Waterman back end (the files under src/fpga/).  Everything crossing it is plain C:
 * POD structs, pointers and sizes, integer return codes, no exceptions.
 *
 * What each entry point replaces in the reference (file:line into
 * falcon-computing/bwa-flow):
 *
 *   bwagpu_create / bwagpu_create_resident
 *       BWAOCLEnv::BWAOCLEnv + initPAC (src/fpga/BWAOCLEnv.h:41-114): bring up
 *       one device, make the 2-bit reference resident on it.  The reference
 *       uploads a forward+revcomp pac with a blocking clEnqueueWriteBuffer per
 *       device (BWAOCLEnv.h:92, 293-312); here only bwa's forward pac
 *       (bwa.c:281-282 layout, bntseq.c:225 bit order) is resident and the
 *       reverse strand is computed in-kernel.  _resident takes a pac that is
 *       already in HBM (e.g. broadcast over xGMI with RCCL by the host).
 *   bwagpu_chain2aln_submit
 *       SWTask::start -> XCLAgent::writeInput + clEnqueueTask(sw_top)
 *       (src/fpga/SWTask.cpp:106-152, xlnx/XCLAgent.cpp:51,89-106): stage one
 *       packed read batch into a slot's buffers and launch asynchronously.
 *   bwagpu_chain2aln_wait
 *   bwagpu_chain2aln_stage / _results (zero-copy host path)
 *       SWTask::finish -> XCLAgent::readOutput + processOutput
 *       (SWTask.cpp:154-180, XCLAgent.cpp:64, FPGAPipeline.cpp:29-130): wait
 *       with a watchdog and return finished mem_alnreg_t records.
 *   bwagpu_chain2aln
 *       submit + wait; the per-batch body of ChainsToRegionsFPGA::compute
 *       (FPGAPipeline.cpp:367-579) with the semantics of the CPU stage
 *       ChainsToRegions::compute (src/Pipeline.cpp:503-544) ->
 *       mem_chain2aln (bwa/bwamem.c:641-795) for every chain of every read.
 *   bwagpu_chain2aln_device
 *       the same launch with every input/output already in device memory
 *       (benchmarks, multi-stream hosts).
 *   bwagpu_extend_batch
 *       a batch of independent ksw_extend2 calls (bwa/ksw.c:380-479); the
 *       task-level granularity of the FPGA kernel's seed_proc
 *       (src/fpga/kernel/smithwaterman.cpp:318-445) but with ksw_extend2's
 *       exact semantics (z-drop, band trimming, runtime scoring).
 *   bwagpu_align2_batch
 *       a batch of independent ksw_align2 calls (bwa/ksw.c:337-357: ksw_u8 /
 *       ksw_i16 local SW, 2nd-best score, start by the reverse pass) as made
 *       by mate rescue, mem_matesw (bwa/bwamem_pair.c:150-151), for every
 *       read pair of a batch (mem_sam_pe, bwamem_pair.c:290-300).  Results
 *       equal ksw_align2's kswr_t field for field, including the quirks of
 *       its striped first pass (see oracle/ksw_align.c).
 *   bwagpu_sw_stream
 *       the FPGA kernel's own job, sw_top over one packed task stream
 *       (clEnqueueTask, xlnx/XCLAgent.cpp:89-106): the input stream of
 *       packReadData (src/fpga/FPGAPipeline.cpp:252-336) in, the 5-int
 *       per-seed result records processOutput reads (FPGAPipeline.cpp:90-105)
 *       out, every seed extended as mem_chain2aln extends one seed
 *       (bwa/bwamem.c:717-792) in its chain's window rmax.
 *   bwagpu_set_bwt / bwagpu_collect_intv / bwagpu_bwt_sa
 *       seeding's interval search and SA lookups for a batch (bwa_idx_load's
 *       bwt_t, mem_collect_intv bwamem.c:120-167, bwt_sa bwt.c:86-96).
 *   bwagpu_seqs2chains
 *       SeqsToChains' per-read body (src/bwa_wrapper.cpp:118-131: mem_chain,
 *       mem_chain_flt, mem_flt_chained_seeds) for a whole batch.
 *   bwagpu_seqs2regions
 *       SeqsToChains + ChainsToRegions (src/Pipeline.cpp:110-121, 503-544) as
 *       one device call: reads in, mem_alnreg_v out.
 *   bwagpu_regs_post / bwagpu_regs_post_device / bwagpu_set_regs_post
 *       the per-read head of RegionsToSam::compute (src/Pipeline.cpp:560-575,
 *       612): mem_sort_dedup_patch with mem_patch_reg (bwa/bwamem.c:415-498),
 *       and the is_alt flag (Pipeline.cpp:570-574) for every read of a batch
 *       (mem_mark_primary_se, Pipeline.cpp:612, is bwagpu_mark_primary).
 *   bwagpu_pestat / bwagpu_mate_rescue (and their _device forms)
 *       what the reference does next with those regions: mem_pestat
 *       (bwa/bwamem_pair.c:49-112; src/Pipeline.cpp:288-289, 578-579) and the
 *       rescue loop at the top of mem_sam_pe (bwamem_pair.c:268-279) with
 *       mem_matesw (:114-183).
 *   bwagpu_mark_primary / bwagpu_pair_select (and their _device forms)
 *       what mem_sam_pe does after the rescue loop up to its first
 *       mem_reg2aln: mem_mark_primary_se on both reads (bwamem_pair.c:280-281),
 *       mem_pair (:185-246), the proper-pair / unpaired decision and the mapq
 *       arithmetic (:288-336, :374-390, mem_approx_mapq_se).
 *   bwagpu_xa_select_device
 *       the selection of mem_gen_alt (bwa/bwamem_extra.c:90-118): which regions
 *       are hits of which record's XA string, and so which regions need a
 *       CIGAR (bwagpu_reg2aln_jobs_device, bwagpu_reg2aln_device).
 *   bwagpu_sam_text_device
 *       the XA strings themselves (bwamem_extra.c:120-135) and mem_aln2sam
 *       (bwa/bwamem.c:837-961) for every record of a batch of pairs: the text
 *       of bseq1_t.sam, in device memory.
 *   bwagpu_last_error
 *       the what() of fpgaHangError / fpgaResultsError / std::runtime_error
 *       (src/util.h:16-32, OpenCLEnv.h:21-31).
 *   bwagpu_destroy
 *       BWAOCLEnv::~BWAOCLEnv (main.cpp:376-387).
 *
 * Results are bit-identical to the reference CPU path: every field that
 * mem_chain2aln writes (rb,re,qb,qe,rid,score,truesc,w,seedcov,seedlen0,
 * frac_rep), all other fields zero, regions in the same order.
 */
#ifndef BWAGPU_H
#define BWAGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BWAGPU_ABI_VERSION 1

/* return codes */
enum {
  BWAGPU_OK = 0,
  BWAGPU_E_INVAL = 1,       /* bad argument / malformed batch                       */
  BWAGPU_E_NOMEM = 2,       /* host or device allocation failed (FPGAPipeline.cpp:383-391) */
  BWAGPU_E_DEVICE = 3,      /* HIP runtime error (OpenCLEnv.h:21-31 analogue)       */
  BWAGPU_E_HANG = 4,        /* watchdog expired (fpgaHangError, SWTask.cpp:116-122)  */
  BWAGPU_E_RESULTS = 5,     /* device flagged an inconsistent input/result
                               (fpgaResultsError, FPGAPipeline.cpp:72; also the
                               reference's assert(c->rid == rid), bwamem.c:669)     */
  BWAGPU_E_UNSUPPORTED = 6, /* read longer than BWAGPU_MAX_READ_LEN                  */
  BWAGPU_E_NODEVICE = 7     /* no HIP device / not built for this device             */
};

/* longest read (bp) the device kernels accept; longer reads -> E_UNSUPPORTED */
#define BWAGPU_MAX_READ_LEN 1023
/* number of independent in-flight slots per context (ping-pong, FPGAPipeline.cpp:373-386) */
#define BWAGPU_NUM_SLOTS 4

/* The fields of mem_opt_t (bwa/bwamem.h:26-58) that mem_chain2aln/ksw_extend2 read. */
typedef struct {
  int32_t a, b;          /* match score, mismatch penalty (used by cal_max_gap)   */
  int32_t o_del, e_del;  /* deletion open/extend                                  */
  int32_t o_ins, e_ins;  /* insertion open/extend                                 */
  int32_t pen_clip5, pen_clip3;
  int32_t w;             /* band width                                            */
  int32_t zdrop;         /* z-dropoff                                             */
  int8_t mat[25];        /* 5x5 scoring matrix (bwa_fill_scmat, bwa/bwa.c:109-118) */
  int8_t pad_[3];
} bwagpu_opt_t;

/* == mem_seed_t (src/bwa_wrapper.h:62-66, bwa/bwamem.c:174-178), 24 bytes */
typedef struct {
  int64_t rbeg;
  int32_t qbeg, len;
  int32_t score;
  int32_t pad_;
} bwagpu_seed_t;

/* == mem_alnreg_t (bwa/bwamem.h:60-79), 88 bytes, same offsets */
typedef struct {
  int64_t rb, re;
  int32_t qb, qe;
  int32_t rid;
  int32_t score, truesc, sub, alt_sc, csub, sub_n;
  int32_t w, seedcov, secondary, secondary_all, seedlen0;
  uint32_t n_comp_is_alt; /* n_comp:30, is_alt:2 — always 0 from mem_chain2aln */
  float frac_rep;
  uint64_t hash;
} bwagpu_alnreg_t;

/* The parts of bntseq_t (bwa/bntseq.h:55-66) the path reads. */
typedef struct {
  int64_t l_pac;
  int32_t n_seqs;
  int32_t pad_;
  const int64_t *ann_offset; /* [n_seqs] bntann1_t.offset */
  const int32_t *ann_len;    /* [n_seqs] bntann1_t.len    */
} bwagpu_bns_t;

/*
 * One read batch (one ChainsRecord, src/Pipeline.h:46-57) in flattened form.
 * Read r has l_seq = seq_off[r+1]-seq_off[r] nt4 bases (0..4, already
 * converted in place as bwa_wrapper.cpp:124-125 does), chains
 * read_chain_off[r] .. read_chain_off[r+1]-1; chain c has seeds
 * chain_seed_off[c] .. chain_seed_off[c+1]-1 in mem_chain_t order, its
 * mem_chain_t.rid and .frac_rep.
 * Output: the regions of read r are written to
 *   out_regs[chain_seed_off[read_chain_off[r]] + k], k < out_n[r]
 * (a read never yields more regions than it has seeds), in the order
 * mem_chain2aln appends them to the read's mem_alnreg_v.
 */
typedef struct {
  int32_t n_reads, n_chains, n_seeds, pad_;
  int64_t seq_bytes;
  const int64_t *seq_off;        /* [n_reads+1]  */
  const uint8_t *seq;            /* [seq_bytes]  */
  const int32_t *read_chain_off; /* [n_reads+1]  */
  const int32_t *chain_seed_off; /* [n_chains+1] */
  const int32_t *chain_rid;      /* [n_chains]   */
  const float *chain_frac_rep;   /* [n_chains]   */
  const bwagpu_seed_t *seeds;    /* [n_seeds]    */
} bwagpu_batch_t;

/* One ksw_extend2 call: query = qpool[qoff..qoff+qlen), target = tpool[toff..toff+tlen).
   h0 is the caller's: a task with h0 <= 0 gets score -1 (the reference asserts h0 > 0), and
   bwagpu_extend_batch refuses a batch with BWAGPU_E_UNSUPPORTED when some task's
   h0 + qlen * max(mat) reaches 2^21 = 2097152 (no H of the call can pass that sum; the
   kernels keep a row's maximum and its last column in one int, H << 10 | j). */
typedef struct {
  int64_t qoff, toff;
  int32_t qlen, tlen;
  int32_t w, end_bonus, zdrop, h0;
} bwagpu_ext_task_t;

/* ksw_extend2 outputs: return value and *qle,*tle,*gtle,*gscore,*max_off */
typedef struct {
  int32_t score, qle, tle, gtle, gscore, max_off;
} bwagpu_ext_result_t;

/* ksw_align2 xtra flags (bwa/ksw.h:6-9); the low 16 bits carry minsc/endsc */
#define BWAGPU_KSW_XBYTE 0x10000
#define BWAGPU_KSW_XSTOP 0x20000
#define BWAGPU_KSW_XSUBO 0x40000
#define BWAGPU_KSW_XSTART 0x80000

/* One ksw_align2(qlen, query, tlen, target, 5, opt->mat, opt->o_del, opt->e_del,
   opt->o_ins, opt->e_ins, xtra, 0) call: query = qpool[qoff..qoff+qlen),
   target = tpool[toff..toff+tlen).  qlen <= BWAGPU_MAX_READ_LEN. */
typedef struct {
  int64_t qoff, toff;
  int32_t qlen, tlen;
  int32_t xtra, pad_;
} bwagpu_align2_task_t;

/* == kswr_t (bwa/ksw.h:17-21); unset fields are -1 */
typedef struct {
  int32_t score, te, qe, score2, te2, tb, qb;
} bwagpu_kswr_t;

/* One mem_reg2aln CIGAR job (bwa/bwamem.c:1104-1174, as called per output
   region from src/bwa_wrapper.cpp:611/728/736/774): the region's
   rb/re/qb/qe/truesc/w (mem_alnreg_t) and its read, l_seq nt4 bases at
   qpool[qoff..qoff+l_seq).  rb < 0 or re < 0 asks for the unmapped record. */
typedef struct {
  int64_t rb, re;
  int64_t qoff;
  int32_t l_seq, qb, qe;
  int32_t truesc, w;
  int32_t pad_;
} bwagpu_reg2aln_task_t;

#define BWAGPU_ALN_OK 0
#define BWAGPU_ALN_NO_CIGAR 1 /* bwa_gen_cigar2 returned no CIGAR (bwa.c:133/135): the
                                 reference's mem_reg2aln would dereference NULL here */
#define BWAGPU_ALN_OVERFLOW 2 /* more than max_ops CIGAR ops or max_md MD bytes */
#define BWAGPU_ALN_UNMAPPED 3 /* rb < 0 || re < 0: rid = -1, pos = -1 (bwamem.c:1112-1115) */
#define BWAGPU_ALN_REFUSED 4  /* bwagpu_reg2aln_device only: the job is outside what the kernel
                                 takes; rid = -1, pos = -1, n_cigar = 0, md_len = 0 */

/* The alignment fields mem_reg2aln fills in mem_aln_t (bwa/bwamem.h:81-92)
   besides mapq/flag/sub/alt_sc (which need the other regions): CIGAR with
   soft clips (ops at cigar[k * max_ops], BAM encoding len << 4 | op), the MD
   string after it in the reference layout (here at md[k * max_md],
   NUL-terminated, md_len = strlen), NM, strand, contig and 0-based position.
   score / w: the global score and band of the last bwa_gen_cigar2 call. */
typedef struct {
  int64_t pos;
  int32_t rid, is_rev;
  int32_t n_cigar, NM;
  int32_t md_len, score;
  int32_t w, status;
} bwagpu_aln_t;

/* ---- seeding: mem_collect_intv on the device ---- */

/* The FM-index of the reference as bwa holds it (bwt_t, bwa/bwt.h:46-57):
   primary, the cumulative counts L2[5], seq_len, and the bwt_size uint32
   words of the interleaved occurrence array (per 128 BWT positions: 4 uint64
   counts, then 8 words of 2-bit bases, first base in the highest bits). */
typedef struct {
  uint64_t primary;
  uint64_t L2[5];
  uint64_t seq_len;
  uint64_t bwt_size;
  const uint32_t *bwt;
  /* the sampled suffix array (bwt.h:55-57): sa[i] = SA[i * sa_intv], n_sa
     entries; sa may be NULL when bwagpu_bwt_sa is not used */
  int32_t sa_intv;
  int32_t pad_;
  uint64_t n_sa;
  const uint64_t *sa;
} bwagpu_bwt_t;

/* == bwtintv_t (bwa/bwt.h:60-62): x[0] / x[1] the SA intervals of the match
   and of its reverse complement, x[2] their size, info = start << 32 | end */
typedef struct {
  uint64_t x[3];
  uint64_t info;
} bwagpu_intv_t;

/* mem_opt_t's seeding fields (bwa/bwamem.h:34-46, defaults bwamem.c:62-72) */
typedef struct {
  int32_t min_seed_len; /* -k, 19 */
  int32_t split_width;  /* 10 */
  int32_t max_mem_intv; /* 20: the LAST-like third pass runs when > 0 */
  float split_factor;   /* -r, 1.5 */
} bwagpu_seedopt_t;

#define BWAGPU_MAX_SEED_READ 4096 /* longest read bwagpu_collect_intv takes */

/* mem_opt_t's chaining fields (bwa/bwamem.h:38-52, defaults bwamem.c:62-72);
   the band (w) and scoring (a, mat, gaps) come from the context's
   bwagpu_opt_t, min_seed_len from bwagpu_seedopt_t */
typedef struct {
  int32_t max_occ;          /* -c, 500: SA positions taken per interval  */
  int32_t max_chain_gap;    /* 10000                                     */
  int32_t min_chain_weight; /* 0                                         */
  int32_t max_chain_extend; /* 1<<30                                     */
  float mask_level;         /* 0.50                                      */
  float drop_ratio;         /* -D, 0.50                                  */
} bwagpu_chainopt_t;

/* one chain: mem_chain_t (bwa/bwamem.c:180-186) without its seed vector —
   the seeds follow in the batch layout (chain_seed_off / seeds) */
typedef struct {
  int64_t pos;      /* the first seed's rbeg: the kbtree key            */
  int32_t rid;      /* contig                                           */
  int32_t n;        /* seeds                                            */
  int32_t w;        /* mem_chain_weight (29-bit field)                  */
  int32_t kept;     /* mem_chain_flt: 1, 2 or 3 (0 chains are dropped)  */
  int32_t first;    /* mem_chain_flt's shadowed-chain index, -1 if none */
  int32_t is_alt;
  float frac_rep;
  int32_t pad_;
} bwagpu_chain_t;

/* per-launch statistics of the last finished launch on a slot */
typedef struct {
  double kernel_ms;      /* HIP-event time of the extension kernel(s)            */
  double total_ms;       /* H2D + kernel + D2H wall (submit..wait)               */
  int64_t cells;         /* evaluated DP cells: sum over executed rows of
                            (end-beg) as ksw.c:424 counts them.  Equal to the
                            reference's count only with the row bound off
                            (bwagpu_ctx_row_bound(ctx, 0), bwagpu_debug.h); with it on (the
                            default) the rows it skips are not counted, so
                            cells and rows fall below the reference's          */
  int64_t rows;          /* executed DP rows (the same caveat)                   */
  int64_t ext_calls;     /* ksw_extend2-equivalent calls                         */
  int64_t h2d_bytes, d2h_bytes;
} bwagpu_stats_t;

typedef struct bwagpu_ctx bwagpu_ctx_t;

int bwagpu_abi_version(void);
int bwagpu_device_count(int *n);

int bwagpu_create(int device, const bwagpu_opt_t *opt, const bwagpu_bns_t *bns,
                  const uint8_t *pac_host, bwagpu_ctx_t **ctx);
int bwagpu_create_resident(int device, const bwagpu_opt_t *opt, const bwagpu_bns_t *bns,
                           const void *pac_device, bwagpu_ctx_t **ctx);
int bwagpu_destroy(bwagpu_ctx_t *ctx);
const char *bwagpu_last_error(const bwagpu_ctx_t *ctx);

/* watchdog for _wait in milliseconds (default 10000, SWTask.cpp:116-122); 0 = none */
int bwagpu_set_watchdog_ms(bwagpu_ctx_t *ctx, int ms);

/* _wait returns BWAGPU_E_RESULTS when a chain's first seed lies outside its
   contig (where bwa asserts, bwamem.c:669); the outputs are still written:
   that chain is skipped, every other chain's regions are valid. */
int bwagpu_chain2aln_submit(bwagpu_ctx_t *ctx, int slot, const bwagpu_batch_t *batch);
int bwagpu_chain2aln_wait(bwagpu_ctx_t *ctx, int slot, bwagpu_alnreg_t *out_regs, int32_t *out_n);
int bwagpu_chain2aln(bwagpu_ctx_t *ctx, const bwagpu_batch_t *batch, bwagpu_alnreg_t *out_regs,
                     int32_t *out_n);

/* Zero-copy host path (packReadData writing straight into the device's DMA
   buffer instead of a staging copy, FPGAPipeline.cpp:252-336 / SWTask.cpp:
   writeInput).  _stage sizes the slot's pinned input buffer for a batch of
   these counts and fills *view with pointers into it (and the counts); the
   caller writes the batch there and passes *view to _submit, which then skips
   its copy.  The view stays valid until the slot's next _stage.  After a
   successful _wait(ctx, slot, NULL, NULL), _results points *regs / *n at the
   slot's pinned output (same layout as _wait's out_regs / out_n), valid until
   the slot's next _submit. */
int bwagpu_chain2aln_stage(bwagpu_ctx_t *ctx, int slot, int32_t n_reads, int32_t n_chains, int32_t n_seeds,
                           int64_t seq_bytes, bwagpu_batch_t *view);
int bwagpu_chain2aln_results(bwagpu_ctx_t *ctx, int slot, const bwagpu_alnreg_t **regs, const int32_t **n);
/* The same results as the device returns them: read r's n[r] regions at
   regs[off[r] .. off[r] + n[r]) (off[r] = n[0] + ... + n[r-1], off has n_reads
   + 1 entries), i.e. processOutput's order without the slot gaps
   (FPGAPipeline.cpp:29-130).  Only these bytes cross PCIe; _results and
   _wait's out_regs rebuild the slot layout from them on the host.  Valid until
   the slot's next _submit. */
int bwagpu_chain2aln_results_dense(bwagpu_ctx_t *ctx, int slot, const bwagpu_alnreg_t **regs, const int32_t **n,
                                   const int32_t **off);
/* all pointers in dev_batch / dev_out / dev_n are device pointers; stream is a
   hipStream_t (NULL = the context's slot-0 stream); asynchronous; dev_stats
   (device, 4 x int64: cells, rows, ext_calls, error flag) may be NULL.
   Up to BWAGPU_NUM_SLOTS distinct streams may be used on one context (each
   keeps its own scratch), so consecutive batches can overlap.  Two calls on
   the SAME stream are ordered by it; the device entry's scratch is separate
   from the submit/wait slots', so both entry points may be used concurrently
   on one context.  Options whose LDS need exceeds a launch are refused with
   BWAGPU_E_UNSUPPORTED before anything is enqueued. */
int bwagpu_chain2aln_device(bwagpu_ctx_t *ctx, const bwagpu_batch_t *dev_batch,
                            bwagpu_alnreg_t *dev_out, int32_t *dev_n, int64_t *dev_stats,
                            void *stream);
/* A bound on the read lengths of later _device batches (1..BWAGPU_MAX_READ_LEN,
   default BWAGPU_MAX_READ_LEN; the host entries take the exact maximum from
   seq_off).  The device sizes its LDS row buffers for it and launches only the
   length bins it reaches (a persistent grid over an empty bin still waits for
   the CU slots another stream's kernel holds).  A longer read sets
   dev_stats[3] bit 2 (as a read over BWAGPU_MAX_READ_LEN does) and gets no
   regions.  The per-read path (BWAGPU_C2A_PATH=fast) ignores it. */
int bwagpu_set_device_read_len(bwagpu_ctx_t *ctx, int32_t max_len);
/* Which steps of a _device batch's chain2aln share a launch, a
   bit mask; default 5 (bits 1 and 4; bit 2 measured no gain and starts off), or
   BWAGPU_FUSED_LAUNCHES when the context is made.
   1: the phased extension's side lists are sorted in two launches per round
      (the ungapped certificate's kernel counts the sides, the scatter scans
      the counts) instead of four;
   2: the late right sides (bwagpu_ctx_ungapped_right) are settled on the
      context's side stream beside a list's right launch, not ahead of it
      (acts only where the caller's stream leaves the context a side stream);
   4: heavy reads without a pair matrix are selected inside the matrix scan's
      launch in the emulate and the final pass, not by a launch of their own.
   0 is the launch sequence without any of them.  Regions, counters and list
   contents do not depend on the mask.  mask < 0 only queries; returns the
   previous mask. */
int bwagpu_ctx_fused_launches(bwagpu_ctx_t *ctx, int mask);

/* The blocking task-list entries below (host buffers) validate every task
   before anything is enqueued: a task outside its pools or a negative or
   NULL-with-length pool returns BWAGPU_E_INVAL, the first bad task in task
   order decides; bwagpu_extend_batch and bwagpu_align2_batch also refuse a
   pool base over 4 that way (bwagpu_sw_stream: BWAGPU_E_RESULTS, from the device).  bwagpu_last_stats(ctx, 0) after a good call:
   kernel_ms of the launches, the kernels' cells / rows / ext_calls, and the
   caller's arrays that moved:
     bwagpu_extend_batch   h2d_bytes = n_tasks * sizeof(bwagpu_ext_task_t) + qpool_len + tpool_len
                           d2h_bytes = n_tasks * sizeof(bwagpu_ext_result_t)
     bwagpu_align2_batch   h2d_bytes = n_tasks * sizeof(bwagpu_align2_task_t) + qpool_len + tpool_len
                           d2h_bytes = n_tasks * sizeof(bwagpu_kswr_t)
     bwagpu_reg2aln_batch  h2d_bytes = n_tasks * sizeof(bwagpu_reg2aln_task_t) + qpool_len
                           d2h_bytes = n_tasks * (sizeof(bwagpu_aln_t) + 4 * max_ops + max_md)
     bwagpu_sw_stream      h2d_bytes = 4 * i_words, d2h_bytes = 20 * *o_tasks (cells / rows /
                           ext_calls are 0) */
int bwagpu_extend_batch(bwagpu_ctx_t *ctx, int32_t n_tasks, const bwagpu_ext_task_t *tasks,
                        const uint8_t *qpool, int64_t qpool_len, const uint8_t *tpool,
                        int64_t tpool_len, bwagpu_ext_result_t *results);

/* ksw_align2 per task.  BWAGPU_E_UNSUPPORTED before anything is enqueued (the
   caller runs ksw_align2 on the CPU; bwagpu_last_error says which):
     - o_ins == 0, no positive match score, a gap penalty over 65535;
     - o_del + e_del or o_ins + e_ins over 65535: the reference keeps 16 bits
       of them (_mm_set1_epi16, ksw.c:252-255) -- for every batch;
     - a task with BWAGPU_KSW_XBYTE while e_del, e_ins, o_del + e_del or
       o_ins + e_ins is over 255: the reference's 8-bit pass keeps 8 bits of
       them (_mm_set1_epi8, ksw.c:132-135) -- a batch without such a task runs
       under the same options;
     - a task without BWAGPU_KSW_XBYTE whose qlen * max(mat) is over 32767 (the
       16-bit scores could saturate), or a qlen over BWAGPU_MAX_READ_LEN.
   The first such task in task order decides. */
int bwagpu_align2_batch(bwagpu_ctx_t *ctx, int32_t n_tasks, const bwagpu_align2_task_t *tasks,
                        const uint8_t *qpool, int64_t qpool_len, const uint8_t *tpool, int64_t tpool_len,
                        bwagpu_kswr_t *results);
/* the same with tasks/pools/results in device memory; asynchronous on stream
   (hipStream_t, NULL = slot-0 stream).  dev_scratch: 8 x (sum of tlen + n_tasks)
   bytes of device memory for the row-maxima lists (ksw.c:191-198).
   Options are refused as above (BWAGPU_E_UNSUPPORTED, nothing enqueued).  The
   host cannot see the tasks, so the per-task refusals are made on the device:
   a task with qlen outside 0..BWAGPU_MAX_READ_LEN or a negative tlen, a
   BWAGPU_KSW_XBYTE task under options over the 8-bit limit, and a task without
   it whose qlen * max(mat) is over 32767 are not computed.  Their records come
   back as seven -1 (score -1 is no value ksw_align2 returns), the other tasks
   of the batch are computed, and the call still returns BWAGPU_OK: a caller
   that can pass such tasks checks score < 0. */
int bwagpu_align2_device(bwagpu_ctx_t *ctx, int32_t n_tasks, const bwagpu_align2_task_t *dev_tasks,
                         const uint8_t *dev_qpool, const uint8_t *dev_tpool, bwagpu_kswr_t *dev_results,
                         void *dev_scratch, void *stream);

/* mem_reg2aln's CIGAR/NM/MD/position for n regions (host buffers; blocking).
   cigar: n * max_ops uint32, md: n * max_md bytes. */
int bwagpu_reg2aln_batch(bwagpu_ctx_t *ctx, int32_t n_tasks, const bwagpu_reg2aln_task_t *tasks,
                         const uint8_t *qpool, int64_t qpool_len, int32_t max_ops, int32_t max_md,
                         bwagpu_aln_t *out, uint32_t *cigar, char *md);
/* The same records, CIGAR slots (k * max_ops) and MD slots (k * max_md) with
   jobs, pool and outputs in device memory, on stream (hipStream_t, NULL = the
   context's slot-0 stream).  The job count is n_cap, or min(n_cap,
   *dev_n_tasks) when dev_n_tasks is not NULL (a producer's count that stayed
   on the device: bwagpu_reg2aln_jobs_device's dev_n_jobs fits).  Records and
   slots at or beyond the job count are not touched.
   Before any launch: NULLs with n_cap > 0, n_cap < 0, max_ops < 1, max_md < 1
   and qpool_len < 0 return BWAGPU_E_INVAL.  Nothing else is validated on the
   host.  On the device a job is judged alone and never fails the call: it gets
   status BWAGPU_ALN_REFUSED (rid = -1, pos = -1, n_cigar = 0, md_len = 0, its
   CIGAR and MD slots untouched) when bwagpu_reg2aln_batch would have refused
   the batch for it (read outside the pool; on an otherwise valid window qb /
   qe outside the read, qe - qb > BWAGPU_MAX_READ_LEN, re - rb > 8192, more
   LDS than a workgroup has), or when its truesc is outside [-2^24, 2^24] or
   its w outside [0, 2^24] (no real score reaches these; inside them no 32-bit
   expression of the band inference wraps).  BWAGPU_ALN_UNMAPPED and
   BWAGPU_ALN_NO_CIGAR are decided as in the batch form.
   The call waits for the stream once: the device bins the jobs, and the bin
   table (under 1 KB) comes to the host, which sizes the launches from its
   counts and maxima.  The bin kernels are then left running: they are
   enqueued on the context's side streams and stream is ordered after them.
   Calls on different streams are ordered among themselves by an event (they
   share the context's scratch).  bwagpu_last_stats(ctx, 0) after the call is
   all zeros but ext_calls = the job count, as bwagpu_mate_rescue_device
   leaves it: h2d_bytes = d2h_bytes = 0, and kernel_ms = 0 because no _device
   entry takes a kernel time (the kernels are still running when it returns;
   bwagpu_mark_primary_device does not write the stats at all).  Refused jobs
   are counted from their status.  n_cap may be any int32 >= 0. */
int bwagpu_reg2aln_device(bwagpu_ctx_t *ctx, int32_t n_cap, const int32_t *dev_n_tasks,
                          const bwagpu_reg2aln_task_t *dev_tasks, const uint8_t *dev_qpool, int64_t qpool_len,
                          int32_t max_ops, int32_t max_md, bwagpu_aln_t *dev_out, uint32_t *dev_cigar,
                          char *dev_md, void *stream);
/* The jobs of a selection over regions in device memory, asynchronous on
   stream (no host wait).  Read r's region k is dev_regs[dev_reg_off[r] + k],
   k < dev_n[r]; it gets a job iff dev_select[dev_reg_off[r] + k] >= 0
   (bwagpu_pair_select_device's out_mapq fits).  Jobs come in (read, k) order:
   rb, re, qb, qe, truesc, w from the region, qoff = dev_seq_off[r], l_seq =
   dev_seq_off[r + 1] - dev_seq_off[r].  dev_job_of is parallel to the regions
   (only the entries of the reads' regions are written): the job's index, or
   -1 for a region without a job or whose job is past job_cap.  dev_n_jobs[0] =
   jobs written (<= job_cap), dev_n_jobs[1] = jobs needed.  Negative n_reads or
   job_cap and NULLs return BWAGPU_E_INVAL before any launch. */
int bwagpu_reg2aln_jobs_device(bwagpu_ctx_t *ctx, int32_t n_reads, const int64_t *dev_reg_off,
                               const bwagpu_alnreg_t *dev_regs, const int32_t *dev_n, const int32_t *dev_select,
                               const int64_t *dev_seq_off, int32_t job_cap, bwagpu_reg2aln_task_t *dev_tasks,
                               int32_t *dev_job_of, int32_t *dev_n_jobs, void *stream);

/* The FPGA wire format.  i_buf/i_words: one or more
   read records exactly as packReadData writes them (FPGAPipeline.cpp:252-336),
   back to back from word 0 (each record's first word is the word index of its
   end, relative to i_buf):
     end, l_seq, ceil(l_seq/8) words of 4-bit bases (first base in the high
     nibble), n_chains, then per chain: rmax[0], rmax[1] (int64, the window of
     getChainRef, FPGAPipeline.cpp:143-192), n_tasks, then per task: task index,
     rbeg (int64), qbeg, len.
   Every task is one seed extended left and right in its chain's window
   (bwamem.c:717-792: band retry, z-drop, local vs to-end); the record of task
   t is o_buf[10 t .. 10 t + 9] (int16): t & 0xffff, t >> 16, qb, qe - (qbeg +
   len), rb - rbeg, re - (rbeg + len), score, truesc, w, 0 — the fields
   processOutput applies (FPGAPipeline.cpp:91-105).  Task indices must be
   0..n-1, each once; *o_tasks = n.  o_cap_tasks bounds n.  A malformed
   stream returns BWAGPU_E_INVAL before any launch, or BWAGPU_E_RESULTS when
   the device finds it (a record that does not end at its end word, a task
   index out of range or repeated, a seed outside its window).  Reads up to
   BWAGPU_MAX_READ_LEN bp. */
int bwagpu_sw_stream(bwagpu_ctx_t *ctx, const int32_t *i_buf, int64_t i_words, int16_t *o_buf,
                     int32_t o_cap_tasks, int32_t *o_tasks);

int bwagpu_last_stats(const bwagpu_ctx_t *ctx, int slot, bwagpu_stats_t *stats);

/* Makes bwt the context's resident FM-index (copied to the device; a later
   call replaces it).  Replaces bwa's in-memory bwt_t for the seeding stage
   (bwa_idx_load_bwt, bwa/bwa.c:244-260; bwa-flow's SeqsToChains reads it through
   aux->idx->bwt, src/Pipeline.cpp:110-121). */
int bwagpu_set_bwt(bwagpu_ctx_t *ctx, const bwagpu_bwt_t *bwt);

/* mem_collect_intv (bwa/bwamem.c:120-167) for every read of a batch: the
   SMEMs (bwt_smem1, bwt.c:289-356), the re-seeding inside long SMEMs, the
   LAST-like pass (bwt_seed_strategy1, bwt.c:358-378), sorted by info as
   ks_introsort leaves them (bwamem.c:90-91, 166).  Reads: nt4 bases (0..4) at
   seq[seq_off[r]..seq_off[r+1]), host buffers, at most BWAGPU_MAX_SEED_READ
   bases.  out_n[r] = read r's interval count; the intervals of all reads go
   to out back to back in read order (read r's at sum(out_n[0..r))), at most
   out_cap of them.  max_per_read bounds one read's list on the device: a read
   with more gets out_n[r] = -(its count) and the call returns
   BWAGPU_E_UNSUPPORTED (out_n is still written); so does a batch whose total
   exceeds out_cap.  Blocking. */
int bwagpu_collect_intv(bwagpu_ctx_t *ctx, const bwagpu_seedopt_t *opt, int32_t n_reads, const int64_t *seq_off,
                        const uint8_t *seq, int32_t max_per_read, bwagpu_intv_t *out, int64_t out_cap,
                        int32_t *out_n);

/* bwt_sa (bwa/bwt.c:86-96) for n BWT positions k[i] in [0, seq_len]: out[i]
   = the forward-reverse coordinate mem_chain takes as a seed's rbeg
   (bwamem.c:288).  Needs the suffix array in bwagpu_set_bwt.  Blocking. */
int bwagpu_bwt_sa(bwagpu_ctx_t *ctx, int64_t n, const uint64_t *k, uint64_t *out);

/* ---- seeding's chaining: SeqsToChains on the device ---- */

/* a batch's chains in the bwagpu_batch_t layout: read r's chains are
   read_chain_off[r] .. read_chain_off[r+1]-1 (in the order bwa-flow's
   SeqsToChains leaves them), chain c's seeds chain_seed_off[c] ..
   chain_seed_off[c+1]-1 (mem_chain_t.seeds, in order) */
typedef struct {
  int32_t n_reads, n_chains;
  int64_t n_seeds;
  const int32_t *read_chain_off;  /* [n_reads+1]  */
  const int32_t *chain_seed_off;  /* [n_chains+1] */
  const bwagpu_chain_t *chains;   /* [n_chains]   */
  const bwagpu_seed_t *seeds;     /* [n_seeds]    */
} bwagpu_chains_t;

/* per-contig ALT flags (bntann1_t.is_alt, bwa/bntseq.h:41) that mem_chain
   copies into its chains and mem_chain_flt reads (bwamem.c:305, 359); n_seqs
   bytes, NULL = none (the default) */
int bwagpu_set_alt(bwagpu_ctx_t *ctx, const uint8_t *is_alt);

/* bwa-flow's SeqsToChains (src/bwa_wrapper.cpp:105-115) for every read of a
   batch: mem_collect_intv, then mem_chain's body (bwamem.c:260-330: bwt_sa of
   each interval's positions stepped to max_occ, bns_intv2rid, the kbtree of
   chains with test_and_merge), mem_chain_flt (336-396) and
   mem_flt_chained_seeds (607-624, mem_seed_sw through ksw_align2).  raw = 1
   stops after mem_chain (chains in kbtree order; w = kept = 0, first = -1).
   Reads as for bwagpu_collect_intv (host buffers, nt4, <= BWAGPU_MAX_SEED_READ
   bases); needs the suffix array in bwagpu_set_bwt.  *out points into
   context-owned pinned memory, valid until the next call on the context.
   Blocking. */
int bwagpu_seqs2chains(bwagpu_ctx_t *ctx, const bwagpu_seedopt_t *sopt, const bwagpu_chainopt_t *copt,
                       int32_t n_reads, const int64_t *seq_off, const uint8_t *seq, int32_t raw,
                       bwagpu_chains_t *out);

/* SeqsToChains and ChainsToRegions (src/Pipeline.cpp:110-121, 503-544) fused
   on the device: the chains never leave it.  out_n[r] = read r's regions
   (mem_chain2aln of each of its chains in order, as bwagpu_chain2aln returns
   them); *regs = every read's regions back to back in read order, *n_regs in
   all (context-owned pinned memory, valid until the next call).  Reads <=
   BWAGPU_MAX_READ_LEN.  BWAGPU_E_RESULTS as for bwagpu_chain2aln_wait.
   Blocking. */
int bwagpu_seqs2regions(bwagpu_ctx_t *ctx, const bwagpu_seedopt_t *sopt, const bwagpu_chainopt_t *copt,
                        int32_t n_reads, const int64_t *seq_off, const uint8_t *seq, int32_t *out_n,
                        const bwagpu_alnreg_t **regs, int64_t *n_regs);

/* ---- region post-processing: the head of RegionsToSam::compute on the device ---- */

#define BWAGPU_POST_DEDUP_PATCH 1 /* mem_sort_dedup_patch (bwamem.c:446-498)                    */
#define BWAGPU_POST_MARK_ALT    2 /* is_alt (Pipeline.cpp:570-574); needs bwagpu_set_alt; NULL
                                     table = no ALT                                            */
#define BWAGPU_POST_PRIMARY     4 /* mem_mark_primary_se (bwamem.c:530-567), id = id0 + read index:
                                     reserved, every entry refuses it with BWAGPU_E_UNSUPPORTED */

/* mem_opt_t's fields the pass reads besides the context's bwagpu_opt_t
   (bwa/bwamem.h:38-52; defaults 10000, 0.95f, 0.50f, bwamem.c:62-72) */
typedef struct {
  int32_t max_chain_gap;
  float mask_level_redun;
  float mask_level;
  int32_t pad_;
} bwagpu_postopt_t;

/* RegionsToSam::compute's loop over a batch (src/Pipeline.cpp:560-575): read r's n[r] regions at regs[reg_off[r] ..) are
   replaced by the surviving ones at the front of that span, in the reference's
   order and with every byte of every record as the reference leaves it
   (n_comp and is_alt included); n[r] is updated.  id0 belongs to the reserved
   BWAGPU_POST_PRIMARY and is not read.  Reads: nt4 bases at seq[seq_off[r] ..
   seq_off[r+1]), at most BWAGPU_MAX_READ_LEN (a longer read returns
   BWAGPU_E_UNSUPPORTED before any launch).  Negative counts, spans that
   overlap and a region whose qb/qe lie outside its read return
   BWAGPU_E_INVAL, also before any launch.  A pair that passes
   mem_patch_reg's gates (bwamem.c:421-432) with b->re - a->rb over 4096 is
   not evaluated: BWAGPU_E_UNSUPPORTED after the pass (mem_chain2aln's regions
   stay far below).  Host buffers; blocking.  bwagpu_last_stats(ctx, 0):
   kernel_ms of the pass, ext_calls = the patch DPs (bwa_gen_cigar2 calls that
   reached ksw_global2). */
int bwagpu_regs_post(bwagpu_ctx_t *ctx, const bwagpu_postopt_t *popt, int32_t flags, int64_t id0, int32_t n_reads,
                     const int64_t *seq_off, const uint8_t *seq, const int64_t *reg_off, bwagpu_alnreg_t *regs,
                     int32_t *n);
/* The same on device memory, asynchronous on stream (hipStream_t, NULL = the
   context's slot-0 stream): directly on what bwagpu_chain2aln_device wrote, on
   the same stream.  dev_batch: host struct of device pointers (n_reads,
   seq_off, seq; with dev_reg_off == NULL also read_chain_off and
   chain_seed_off: read r's span then starts at
   chain_seed_off[read_chain_off[r]], the slot layout).  dev_reg_off: int64 per
   read.  Nothing is validated on the device path except what keeps the kernel
   inside its buffers: a patch candidate outside its read (or over the 4096
   window) is skipped. */
int bwagpu_regs_post_device(bwagpu_ctx_t *ctx, const bwagpu_postopt_t *popt, int32_t flags, int64_t id0,
                            const bwagpu_batch_t *dev_batch, const int64_t *dev_reg_off, bwagpu_alnreg_t *dev_regs,
                            int32_t *dev_n, void *stream);
/* The switch: with flags != 0, bwagpu_chain2aln_submit/_wait (and so
   bwagpu_chain2aln, _results, _results_dense) and bwagpu_seqs2regions run the
   pass on the device before the results leave it; the dense output is
   compacted after the pass, so only surviving regions cross PCIe.  The next
   batch takes id0_of_next_batch as its id0, every later one the previous id0
   plus the previous batch's n_reads (RegionsToSam's start_idx).  flags == 0
   (the default; popt may be NULL then) restores the plain results. */
int bwagpu_set_regs_post(bwagpu_ctx_t *ctx, const bwagpu_postopt_t *popt, int32_t flags, int64_t id0_of_next_batch);

/* ---- paired ends: mem_pestat and the mate rescue loop on the device ---- */

/* mem_opt_t's fields the two passes read besides the context's bwagpu_opt_t
   (defaults 10000, 50, 17, 19, 10000, 0.95f, 0.50f: bwamem.c:48-84), and the
   number of plan / align / replay rounds one bwagpu_mate_rescue call may run
   (1..8; 3 is plenty: a second round happens only when a dedup removed the
   region that had made a call unnecessary) */
typedef struct {
  int32_t max_ins;
  int32_t max_matesw;
  int32_t pen_unpaired;
  int32_t min_seed_len;
  int32_t max_chain_gap;
  float mask_level_redun;
  float mask_level;
  int32_t max_rounds;
} bwagpu_pairopt_t;

/* == mem_pestat_t (bwa/bwamem.h:82-86) */
typedef struct {
  int32_t low, high;
  int32_t failed, pad_;
  double avg, std;
} bwagpu_pestat_t;

/* mem_pestat over a batch (bwamem_pair.c:49-112): reads 2i and 2i+1 are pair
   i (a trailing odd read is ignored, as n >> 1 does), read r's n[r] regions at
   regs[reg_off[r] ..) as bwagpu_regs_post leaves them.  pes[4] equals the
   reference's bit for bit, the doubles included.  Host buffers; blocking.
   Negative counts return BWAGPU_E_INVAL before any launch.
   bwagpu_last_stats(ctx, 0): kernel_ms of the pass; h2d_bytes counts the
   caller's arrays that were moved, as for the other host-buffer entries (the
   regions from the first to the last span, reg_off and n of the reads in
   pairs); d2h_bytes is 0, the four fixed-size records are not counted. */
int bwagpu_pestat(bwagpu_ctx_t *ctx, const bwagpu_pairopt_t *popt, int32_t n_reads, const int64_t *reg_off,
                  const bwagpu_alnreg_t *regs, const int32_t *n, bwagpu_pestat_t *pes);
/* The same on device memory, asynchronous on stream (hipStream_t, NULL = the
   context's slot-0 stream); dev_pes: 4 records in device memory. */
int bwagpu_pestat_device(bwagpu_ctx_t *ctx, const bwagpu_pairopt_t *popt, int32_t n_reads, const int64_t *dev_reg_off,
                         const bwagpu_alnreg_t *dev_regs, const int32_t *dev_n, bwagpu_pestat_t *dev_pes,
                         void *stream);

#define BWAGPU_RESCUE_DONE        0 /* both reads' regions are the reference's a[0] / a[1] after
                                       bwamem_pair.c:268-279, byte for byte and in order         */
#define BWAGPU_RESCUE_UNFINISHED  1 /* max_rounds reached                                        */
#define BWAGPU_RESCUE_OVERFLOW    2 /* a push did not fit the read's output span                 */
#define BWAGPU_RESCUE_UNSUPPORTED 3 /* a read of the pair is longer than BWAGPU_MAX_READ_LEN (or
                                       ksw_align2's 16-bit scores could saturate on it)          */

/* The rescue loop of mem_sam_pe (bwamem_pair.c:268-279) for every pair of a
   batch.  The input regions (regs, reg_off, n) are not modified.  Read r's
   result goes to out_regs[out_off[r] ..) and may hold up to out_off[r+1] -
   out_off[r] regions (at least n[r]; every region a call pushes needs room
   before the dedup that follows may remove one); out_n[r] is its count.
   status[n_reads/2] is BWAGPU_RESCUE_* per pair; with a non-zero status the
   pair's output is a copy of its input, n_sw is -1 and the caller keeps the
   CPU path for that pair.  n_sw[n_reads/2]: the sum of mem_matesw's return
   values (ksw_align2 calls the reference makes for the pair).
   Before any launch: odd n_reads, negative counts, a qb/qe outside its read,
   a base over 4 or an output span smaller than its input return
   BWAGPU_E_INVAL; options bwagpu_align2_batch refuses and a live orientation
   with high - low over 2^20 return BWAGPU_E_UNSUPPORTED.  Host buffers;
   blocking.  bwagpu_last_stats(ctx, 0): kernel_ms of the passes, ext_calls =
   ksw_align2 tasks computed (0: no align2 launch), cells = tasks the replay
   used, rows = rounds run. */
int bwagpu_mate_rescue(bwagpu_ctx_t *ctx, const bwagpu_pairopt_t *popt, const bwagpu_pestat_t *pes, int32_t n_reads,
                       const int64_t *seq_off, const uint8_t *seq, const int64_t *reg_off,
                       const bwagpu_alnreg_t *regs, const int32_t *n, const int64_t *out_off,
                       bwagpu_alnreg_t *out_regs, int32_t *out_n, int32_t *status, int32_t *n_sw);
/* The same on device memory, on stream (hipStream_t, NULL = the context's
   slot-0 stream): directly after bwagpu_regs_post_device / bwagpu_pestat_device
   on the same stream.  dev_batch: host struct of device pointers (n_reads,
   seq_bytes, seq_off, seq with seq_off[n_reads] <= seq_bytes).  The task
   counts of every round come to the host (the call waits for the stream
   there, as bwagpu_seqs2regions does); the last round's replay is left
   running on the stream.  Nothing is validated on the device path except what
   keeps the kernels inside their buffers: an output span smaller than its
   input gives the pair BWAGPU_RESCUE_OVERFLOW with out_n = 0. */
int bwagpu_mate_rescue_device(bwagpu_ctx_t *ctx, const bwagpu_pairopt_t *popt, const bwagpu_pestat_t *dev_pes,
                              const bwagpu_batch_t *dev_batch, const int64_t *dev_reg_off,
                              const bwagpu_alnreg_t *dev_regs, const int32_t *dev_n, const int64_t *dev_out_off,
                              bwagpu_alnreg_t *dev_out_regs, int32_t *dev_out_n, int32_t *dev_status,
                              int32_t *dev_n_sw, void *stream);

/* ---- paired ends: primary marking, mem_pair and the mapq arithmetic on the device ---- */

/* mem_opt_t's fields the two passes read besides the context's bwagpu_opt_t
   (bwa/bwamem.h:26-58; defaults 30, 17, 19, 50.f, 3, 0.50f, 0.50f: bwamem.c:48-84).
   flags are mem_opt_t.flag's bits: BWAGPU_MEM_F_NOPAIRING is honoured, the
   four refused ones below return BWAGPU_E_UNSUPPORTED, every other bit is
   ignored (none of them is read between bwamem_pair.c:280 and the first
   mem_reg2aln).  drop_ratio is carried for mem_reg2sam's third test
   (bwamem.c:1035), which only MEM_F_ALL can reach. */
typedef struct {
  int32_t T;
  int32_t pen_unpaired;
  int32_t min_seed_len;
  float mapQ_coef_len;
  int32_t mapQ_coef_fac;
  float mask_level;
  float drop_ratio;
  int32_t flags;
} bwagpu_selopt_t;

#define BWAGPU_MEM_F_NOPAIRING      0x4
#define BWAGPU_MEM_F_ALL            0x8    /* refused */
#define BWAGPU_MEM_F_NO_MULTI       0x10   /* refused */
#define BWAGPU_MEM_F_PRIMARY5       0x800  /* refused */
#define BWAGPU_MEM_F_KEEP_SUPP_MAPQ 0x1000 /* refused */

/* regions of one read (bwagpu_mark_primary), primary regions of one pair
   (bwagpu_pair_select) the kernels hold in LDS */
#define BWAGPU_SEL_MAX_REGS 512

#define BWAGPU_SEL_DONE     0 /* the read / pair is as the reference leaves it                     */
#define BWAGPU_SEL_TOO_MANY 1 /* over BWAGPU_SEL_MAX_REGS, or (pair_select) an argument of the
                                 mapq arithmetic's log outside the context's table [1, 65536)    */
#define BWAGPU_SEL_SKIPPED  2 /* pair_select: in_status was non-zero for the pair                  */

/* mem_mark_primary_se (bwamem.c:502-567) for every read of a batch, in place:
   read r's n[r] regions at regs[reg_off[r] ..) with id = id0 + r (mem_sam_pe's
   id<<1|r is id0 = 2 * the first pair's id; the contract BWAGPU_POST_PRIMARY
   reserves).  The regions are reordered and sub, sub_n, alt_sc, secondary,
   secondary_all and hash are written as the reference leaves them; n_pri[r] is
   the function's return value.  status[r] is BWAGPU_SEL_DONE, or
   BWAGPU_SEL_TOO_MANY for a read over BWAGPU_SEL_MAX_REGS regions, which is left
   untouched (n_pri[r] = 0): the caller keeps the CPU path for it.  Of sopt only
   mask_level is read.  Negative counts, overlapping spans and NULLs return
   BWAGPU_E_INVAL before any launch.  Host buffers; blocking.
   bwagpu_last_stats(ctx, 0): kernel_ms of the pass. */
int bwagpu_mark_primary(bwagpu_ctx_t *ctx, const bwagpu_selopt_t *sopt, int64_t id0, int32_t n_reads,
                        const int64_t *reg_off, bwagpu_alnreg_t *regs, const int32_t *n, int32_t *n_pri,
                        int32_t *status);
/* The same on device memory, asynchronous on stream (hipStream_t, NULL = the
   context's slot-0 stream): directly on what bwagpu_mate_rescue_device wrote
   (dev_out_off, dev_out_regs, dev_out_n).  Nothing is validated on the device
   path except what keeps the kernel inside its buffers. */
int bwagpu_mark_primary_device(bwagpu_ctx_t *ctx, const bwagpu_selopt_t *sopt, int64_t id0, int32_t n_reads,
                               const int64_t *dev_reg_off, bwagpu_alnreg_t *dev_regs, const int32_t *dev_n,
                               int32_t *dev_n_pri, int32_t *dev_status, void *stream);

#define BWAGPU_SEL_NO_PAIRING 0 /* bwamem_pair.c:374-392: each read goes through mem_reg2sam      */
#define BWAGPU_SEL_PAIRED     1 /* bwamem_pair.c:298-362: h[i] (and g[i]) are the pair's records   */

/* What mem_sam_pe decides for one pair between bwamem_pair.c:286 and its first
   mem_reg2aln; 64 bytes.
   BWAGPU_SEL_PAIRED: z[i] is the region emitted as h[i] with mapq[i] (q_se as
   mem_aln_t.mapq's 8 bits hold it) and flag 0x40<<i | extra_flag; alt[i] is the index of g[i] (n_pri[i]) or -1.
   BWAGPU_SEL_NO_PAIRING: z[i] is the `which` of :375-384 (the mate record h[i]
   the other read's lines refer to) or -1, mapq[i] that record's mapq, alt[i]
   -1; the read's own records are the regions with out_mapq >= 0 in order
   (mem_reg2sam, bwamem.c:1030-1047: the first one primary, later ones
   supplementary), each with extra_flag | 0x41 / 0x81.
   o, subo, n_sub: mem_pair's return value and outputs as it leaves them
   (before :301), 0 where it was not called. */
typedef struct {
  int32_t status;     /* BWAGPU_SEL_* */
  int32_t branch;
  int32_t n_pri[2];
  int32_t z[2];
  int32_t mapq[2];
  int32_t alt[2];
  int32_t extra_flag;
  int32_t o, subo, n_sub;
  int32_t pad_[2];
} bwagpu_pairsel_t;

/* mem_sam_pe from bwamem_pair.c:286 to its first mem_reg2aln for every pair of
   a batch: mem_pair (:185-246), the proper-pair / unpaired decision and the
   mapq arithmetic (:288-336, :374-390, mem_approx_mapq_se).  Reads 2i and 2i+1
   are pair i with id pair_id0 + i; read r's n[r] regions at regs[reg_off[r] ..)
   as bwagpu_mark_primary leaves them (which was given id0 = 2 * pair_id0) with
   its n_pri[r]; pes[4] as bwagpu_pestat returns it.
   sel[n_reads/2] receives the decision.  out_mapq is parallel to regs:
   out_mapq[reg_off[r] + k] is -1 for a region that gets no SAM record,
   otherwise the record's mapq.  The regions are modified in place exactly as
   the reference modifies them (sub and secondary = -2 of :312-313, the
   secondary_all switch of :327-336).  in_status may be NULL; a pair with
   in_status[i] != 0 (bwagpu_mate_rescue's status array fits) gets
   BWAGPU_SEL_SKIPPED.  A pair with a non-zero status keeps its regions
   untouched, its out_mapq entries are -1 and the caller keeps the CPU path for
   it.  mem_gen_alt's selection is bwagpu_xa_select_device, the CIGARs are
   bwagpu_reg2aln_jobs_device and bwagpu_reg2aln_device; the XA strings and the
   SAM text are bwagpu_sam_text_device.
   Before any launch: odd n_reads, negative counts, n_pri outside [0, n], a rid
   outside the reference, overlapping spans and NULLs return BWAGPU_E_INVAL;
   the refused flags and a live orientation with high - low over 2^20 return
   BWAGPU_E_UNSUPPORTED.  Host buffers; blocking.  bwagpu_last_stats(ctx, 0):
   kernel_ms of the pass; h2d_bytes / d2h_bytes count the caller's arrays that
   were moved, so the n_reads/2 words of in_status only when it is not NULL. */
int bwagpu_pair_select(bwagpu_ctx_t *ctx, const bwagpu_selopt_t *sopt, const bwagpu_pestat_t *pes, int64_t pair_id0,
                       int32_t n_reads, const int64_t *reg_off, bwagpu_alnreg_t *regs, const int32_t *n,
                       const int32_t *n_pri, const int32_t *in_status, bwagpu_pairsel_t *sel, int32_t *out_mapq);
/* The same on device memory, on stream (hipStream_t, NULL = the context's
   slot-0 stream), directly after bwagpu_mark_primary_device on that stream.
   The 128 bytes of dev_pes come to the host for the pairing tables (the call
   waits for the stream there, as bwagpu_mate_rescue_device does); the kernel
   is left running on the stream. */
int bwagpu_pair_select_device(bwagpu_ctx_t *ctx, const bwagpu_selopt_t *sopt, const bwagpu_pestat_t *dev_pes,
                              int64_t pair_id0, int32_t n_reads, const int64_t *dev_reg_off,
                              bwagpu_alnreg_t *dev_regs, const int32_t *dev_n, const int32_t *dev_n_pri,
                              const int32_t *dev_in_status, bwagpu_pairsel_t *dev_sel, int32_t *dev_out_mapq,
                              void *stream);

/* ---- paired ends: the selection of mem_gen_alt (XA) on the device ---- */

/* mem_opt_t's fields the SAM stage reads after the pair selection: so far those
   of mem_gen_alt's selection (bwa/bwamem.h:50, 56; defaults 0.80f, 5, 200:
   bwamem.c:71-76).  flags are mem_opt_t.flag's bits:
   the four bwagpu_selopt_t refuses return BWAGPU_E_UNSUPPORTED (with MEM_F_ALL
   the reference does not call mem_gen_alt at all), every other bit is ignored. */
typedef struct {
  int32_t flags;
  float XA_drop_ratio;
  int32_t max_XA_hits, max_XA_hits_alt;
} bwagpu_samopt_t;

/* The selection of mem_gen_alt (bwa/bwamem_extra.c:90-118, as called at
   bwamem_pair.c:337-340 and bwamem.c:1026-1027) for every read of a batch, on
   device memory, asynchronous on stream (hipStream_t, NULL = the context's
   slot-0 stream; no host wait): directly after bwagpu_pair_select_device on
   that stream, on the regions, dev_sel and dev_out_mapq it leaves.
   dev_xa_of and dev_job_select are parallel to the regions; only the entries of
   the reads' regions are written.  For a pair with sel.status ==
   BWAGPU_SEL_DONE, with i and r indices into one read's regions:
   dev_xa_of[reg_off + i] = r when region i is a hit of the XA string that the
   record of region r prints, else -1.  That is: get_pri_idx(i) == r (in
   double, as the reference computes it), the string's hit count cnt[r] within
   max_XA_hits, or within max_XA_hits_alt when one of its hits is an ALT hit,
   and out_mapq[reg_off + r] >= 0 (a string is only ever printed on an emitted
   record; the counts and caps run over all regions).  The hits of r's string
   are the regions with xa_of == r in index order.
   dev_job_select[reg_off + i] = 0 when region i needs a CIGAR: it has a record
   (out_mapq >= 0), or it is an XA hit (xa_of >= 0), or it is sel.z of a
   BWAGPU_SEL_NO_PAIRING pair (the mate record the other read's lines refer
   to, which may have no record of its own); else -1.  It is what
   bwagpu_reg2aln_jobs_device takes as dev_select in the place of out_mapq.
   A pair with another status gets -1 in both arrays.
   Before any launch: NULLs, negative or odd n_reads return BWAGPU_E_INVAL, the
   refused flags BWAGPU_E_UNSUPPORTED.  Nothing is validated on the device
   except what keeps the kernel inside the reads' spans: a secondary_all
   outside its read joins no string. */
int bwagpu_xa_select_device(bwagpu_ctx_t *ctx, const bwagpu_samopt_t *xopt, int32_t n_reads,
                            const int64_t *dev_reg_off, const bwagpu_alnreg_t *dev_regs, const int32_t *dev_n,
                            const bwagpu_pairsel_t *dev_sel, const int32_t *dev_out_mapq, int32_t *dev_xa_of,
                            int32_t *dev_job_select, void *stream);

/* ---- paired ends: the XA strings and mem_aln2sam on the device ---- */

#define BWAGPU_MEM_F_REF_HDR  0x100  /* refused by bwagpu_sam_text_device (XR:Z needs bntann1_t.anno) */
#define BWAGPU_MEM_F_SOFTCLIP 0x200
#define BWAGPU_MEM_F_XB       0x2000

/* bwagpu_sam_text_device's per-pair status */
#define BWAGPU_SAM_DONE       0
#define BWAGPU_SAM_SKIPPED    1 /* sel.status was not BWAGPU_SEL_DONE                                */
#define BWAGPU_SAM_NEEDS_HOST 2 /* a needed region has no job (job_of == -1, or outside job_cap), a
                                   needed record is not BWAGPU_ALN_OK or does not fit its slots, a
                                   rid is outside [0, n_contigs), or an index of sel is outside its
                                   read                                                             */
#define BWAGPU_SAM_NO_ROOM    3 /* the pair's text would pass text_cap                               */

#define BWAGPU_SAM_MAX_RG 255 /* longest bwa_rg_id taken */

/* The arguments of bwagpu_sam_text_device.  Device memory unless said otherwise.
   The regions, dev_sel, dev_out_mapq and dev_xa_of as bwagpu_pair_select_device and
   bwagpu_xa_select_device leave them; dev_job_of as bwagpu_reg2aln_jobs_device and
   dev_aln, dev_cigar (max_ops words per job), dev_md (max_md bytes per job) as
   bwagpu_reg2aln_device leave them, job_cap their capacity in jobs.
   Read r: nt4 bases dev_seq[dev_seq_off[r] .. dev_seq_off[r+1]) (the CIGAR stage's
   pool), its qualities at the same offsets of dev_qual (NULL: "*"), its name
   dev_names[dev_name_off[r] .. dev_name_off[r+1]) (each read of a pair carries its
   own; they are not compared), its comment likewise (dev_comment_off NULL, or an
   empty span: none).  Contig c's name is dev_contig_names[dev_contig_off[c] ..
   dev_contig_off[c+1]), c < n_contigs.  rg_id is a host string, bwa_rg_id (NULL or
   empty: no RG:Z), at most BWAGPU_SAM_MAX_RG bytes; it is read before the call
   returns.  flags are mem_opt_t.flag's bits. */
typedef struct {
  const int64_t *dev_reg_off;
  const bwagpu_alnreg_t *dev_regs;
  const int32_t *dev_n;
  const bwagpu_pairsel_t *dev_sel;
  const int32_t *dev_out_mapq;
  const int32_t *dev_xa_of;
  const int32_t *dev_job_of;
  const bwagpu_aln_t *dev_aln;
  const uint32_t *dev_cigar;
  const char *dev_md;
  const int64_t *dev_seq_off;
  const uint8_t *dev_seq;
  const char *dev_qual;
  const int64_t *dev_name_off;
  const char *dev_names;
  const int64_t *dev_comment_off;
  const char *dev_comments;
  const int64_t *dev_contig_off;
  const char *dev_contig_names;
  const char *rg_id; /* host */
  int32_t flags;
  int32_t n_contigs;
  int32_t job_cap;
  int32_t max_ops, max_md;
  int32_t pad_;
  int64_t text_cap;
  char *dev_text;        /* [text_cap]                                   */
  int64_t *dev_text_off; /* [n_reads + 1]                                */
  int32_t *dev_status;   /* [n_reads / 2] BWAGPU_SAM_*                   */
  int64_t *dev_text_n;   /* [2]: bytes written, bytes needed             */
} bwagpu_samtext_t;

/* The last step of mem_sam_pe for every pair of a batch, on device memory,
   asynchronous on stream (hipStream_t, NULL = the context's slot-0 stream; no
   host wait), directly after bwagpu_reg2aln_device on that stream: mem_gen_alt's
   strings (bwa/bwamem_extra.c:120-135) and mem_aln2sam (bwa/bwamem.c:837-961) for
   every record of bwamem_pair.c:342-362 and of mem_reg2sam (bwamem.c:1030-1058).
   Read r's SAM lines are dev_text[dev_text_off[r] .. dev_text_off[r+1]), byte for
   byte what the reference leaves in bseq1_t.sam without its NUL: the spans follow
   one another without a gap, a non-empty one ends in '\n'.
   For a pair with sel.status == BWAGPU_SEL_DONE the record lists are those of
   bwagpu_pairsel_t's comment.  A record takes rid, pos, is_rev, n_cigar, NM, the
   CIGAR and MD from the job of its region, score, sub = max(sub, csub), is_alt and
   alt_sc from the region (bwamem.c:1170-1171; bwagpu_aln_t.score is not AS), its
   mapq from sel.mapq (h[i]) or dev_out_mapq, printed as eight bits hold it.  A
   record's XA (MEM_F_XB: XB) string is the regions with xa_of == its region, in
   index order.  MEM_F_SOFTCLIP and MEM_F_XB are honoured.  The 0x100 branches of
   mem_aln2sam ("*\t*" for SEQ and QUAL, records left out of SA:Z) are not built:
   only MEM_F_ALL and MEM_F_NO_MULTI give a record that flag, and both are refused.
   dev_status[i] is BWAGPU_SAM_DONE or the reason why both reads of pair i have
   empty spans and the caller keeps the CPU path for it.  dev_text_n[1] is the
   text of all BWAGPU_SAM_DONE and BWAGPU_SAM_NO_ROOM pairs; while it is over
   text_cap, the pairs from the first one that would pass text_cap on are
   BWAGPU_SAM_NO_ROOM and dev_text_n[0] < dev_text_n[1] is what was written
   (text_cap = dev_text_n[1] of an earlier call always fits).
   Before any launch: NULLs (dev_qual, dev_comment_off with dev_comments and rg_id
   may be), negative or odd n_reads, negative text_cap, n_contigs or job_cap,
   max_ops < 1, max_md < 1 and an rg_id over BWAGPU_SAM_MAX_RG bytes return
   BWAGPU_E_INVAL; MEM_F_REF_HDR and the four flags bwagpu_selopt_t refuses return
   BWAGPU_E_UNSUPPORTED; every other bit is ignored.  Nothing is validated on the
   device except what keeps the kernels inside the arrays. */
int bwagpu_sam_text_device(bwagpu_ctx_t *ctx, const bwagpu_samtext_t *t, int32_t n_reads, void *stream);

/* Tuning, test and profiling entry points (bwagpu_debug_*, bwagpu_prof_*,
   bwagpu_ctx_ext_form / _row_bound, bwagpu_streams_concurrent) are declared
   in bwagpu_debug.h: none of them is part of the stage's interface, and the
   reference has no counterpart (it logs per-phase wall times instead,
   src/fpga/FPGAPipeline.cpp:557-578). */

#ifdef __cplusplus
}
#endif
#endif /* BWAGPU_H */
