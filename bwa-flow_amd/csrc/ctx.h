// ctx.h — what the translation units of the C ABI share (capi.hip,
// capi_seed.hip, capi_stages.hip, capi_tasks.hip): the context and its slots,
// grow-only buffers, the error path, the chain2aln and post-processing passes
// that more than one of them enqueues, and the scaffold of a blocking
// host-buffer entry.
// Internal: nothing here is part of include/bwagpu.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "bwagpu.h"
#include "chain.h"
#include "engine.h"
#include "rescue.h"
#include "seed.h"
#include "stage_host.h"
#include "task_host.h"

namespace bwagpu {

// live GrowBuf allocations of the process and their bytes (bwagpu_debug_live_buffers)
inline std::atomic<int64_t> g_live_bufs{0}, g_live_bytes{0};

// Grow-only device buffer, or pinned host buffer.  It owns its memory: whoever holds one
// (the context, a Slot, Staging) frees it by going away, so nothing lists buffers to free.
template <bool kPinned>
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(n + n / 4, 4096);
    const hipError_t e = kPinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = want;
    g_live_bufs.fetch_add(1, std::memory_order_relaxed);
    g_live_bytes.fetch_add((int64_t)want, std::memory_order_relaxed);
    return e;
  }
  // room for n elements of T, at least one so that a kernel always gets a pointer -> out (null on failure)
  template <class T>
  hipError_t get(T*& out, size_t n) {
    const hipError_t e = ensure(sizeof(T) * std::max<size_t>(n, 1));
    out = e == hipSuccess ? (T*)p : nullptr;
    return e;
  }
  void release() {
    if (p) {
      (void)(kPinned ? hipHostFree(p) : hipFree(p));
      g_live_bufs.fetch_sub(1, std::memory_order_relaxed);
      g_live_bytes.fetch_sub((int64_t)cap, std::memory_order_relaxed);
    }
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};
using DevBuf = GrowBuf<false>;
using HostBuf = GrowBuf<true>;
static_assert(!std::is_copy_constructible<DevBuf>::value, "a copy would free the buffer twice");

struct Slot {
  // created on first use (lazy_stream): the device entry runs on the caller's
  // streams, and every stream a context creates takes a place on one of the
  // process's hardware queues (GPU_MAX_HW_QUEUES) the caller's streams and
  // the selection side streams share
  hipStream_t stream = nullptr;
  std::once_flag stream_once;
  hipError_t stream_err = hipSuccess;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  DevBuf d_in, d_win, d_srt, d_prog, d_desc, d_out, d_n, d_stats, d_lists, d_counts;
  DevBuf d_cread, d_ext, d_tasks, d_ctr, d_regpos, d_skipf, d_heavy, d_redo, d_rbits, d_rlist;  // speculative path
  DevBuf d_schain, d_hinfo, d_mat, d_cov, d_hflag, d_colent, d_qh, d_longc, d_sorth, d_stasks, d_ftask, d_ftaskR, d_ung, d_ungt;
  SpecStreams spec;  // created on first use (choose_side)
  bool side_chosen = false;
  HostBuf h_in, h_out, h_n, h_stats;
  // the submit/wait path's results: regions written densely (read r's at
  // h_dense[h_off[r] ..]) by dense_copy_kernel straight into pinned memory;
  // h_out (the slot layout) is filled from them only when asked for
  HostBuf h_dense, h_off;
  DevBuf d_off;
  size_t in_rco = 0, in_cso = 0;  // where the batch's offsets sit in h_in
  bool slot_view = false;         // h_out holds the last batch's slot layout
  bool busy = false;
  // the last submitted batch finished and its results are in h_dense / h_n /
  // h_off (set by _wait; cleared by the next _submit, and never set when a
  // submit fails)
  bool has_results = false;
  // the finished batch's offsets, copied out of h_in by a _stage of the next
  // batch (which overwrites h_in) so that a later _results can still build
  // the slot layout
  bool kept = false;
  std::vector<int32_t> keep_rco, keep_cso;
  int32_t n_reads = 0, n_chains = 0, n_seeds = 0;
  std::chrono::steady_clock::time_point t_submit;
  bwagpu_stats_t last{};
  int64_t h2d = 0, d2h = 0;
  // what the slot itself created, drained first; its buffers free themselves afterwards
  ~Slot() {
    for (hipStream_t x : {stream, spec.side})
      if (x) {
        (void)hipStreamSynchronize(x);
        (void)hipStreamDestroy(x);
      }
    for (hipEvent_t e : {ev0, ev1, ev2, ev3, spec.fork, spec.join})
      if (e) (void)hipEventDestroy(e);
  }
};

inline hipError_t lazy_stream(Slot& s, hipStream_t* st) {
  std::call_once(s.stream_once, [&s] { s.stream_err = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking); });
  *st = s.stream;
  return s.stream_err;
}

// The host-buffer entries' copies of their arguments (HostCall below), one set
// for all of bwagpu_regs_post, bwagpu_pestat, bwagpu_mate_rescue,
// bwagpu_mark_primary and bwagpu_pair_select.  Sharing is safe because those
// entries are blocking (each returns after a synchronise of its stream), all
// run on slot[0]'s stream (so two calls on one context are ordered even when
// issued back to back), and a call reads nothing from a staging buffer that
// the same call did not write first — by an upload, or by the kernels whose
// output it is.  Nothing is live across calls.
struct Staging {
  DevBuf regs, out_regs;             // input (or in-place) spans, output spans
  DevBuf seq;                        // bases
  DevBuf seq_off, reg_off, out_off;  // offsets, relative to what is copied
  DevBuf n, out_n, n_pri, status, n_sw, mapq, sel;  // per read, per pair or per region
  DevBuf pes;                        // the four bwagpu_pestat_t
};

}  // namespace bwagpu

struct bwagpu_ctx {
  using DevBuf = bwagpu::DevBuf;
  using HostBuf = bwagpu::HostBuf;
  using Slot = bwagpu::Slot;
  int device = 0;
  // caller streams seen by the spec path, and side streams retired after a
  // later caller turned out to share their hardware queue (choose_side)
  std::mutex side_mu;
  std::vector<hipStream_t> callers, side_graveyard;
  bwagpu::DevOpt opt{};
  bwagpu::DevRef ref{};
  bool own_pac = false;
  void* d_pac = nullptr;
  int64_t* d_ann_off = nullptr;
  int32_t* d_ann_len = nullptr;
  int watchdog_ms = 10000;
  int ext_form = 0;  // bwagpu_ctx_ext_form (the process default when made)
  int ext_short = 0; // bwagpu_ctx_ext_short (BWAGPU_EXT_SHORT_Q or the compiled default when made)
  int light_pack = 0;  // bwagpu_ctx_light_pack (BWAGPU_LIGHT_PACK or the compiled default when made)
  int ext_short_fill = 0;  // bwagpu_ctx_ext_short_fill (BWAGPU_EXT_SHORT_FILL or the compiled default when made)
  int ungapped = 1;  // bwagpu_ctx_ungapped (BWAGPU_UNGAPPED or on when made); acts only while opt.row_bound is on
  int ungapped_right = 1;  // bwagpu_ctx_ungapped_right (BWAGPU_UNGAPPED_RIGHT or on when made); acts only while ungapped does
  int emu_finish = 1;  // bwagpu_ctx_emu_finish (BWAGPU_EMU_FINISH or on when made)
  int fused_launches = 5;  // bwagpu_ctx_fused_launches (BWAGPU_FUSED_LAUNCHES or 5 when made)
  Slot slot[BWAGPU_NUM_SLOTS];
  // bwagpu_chain2aln_device: the caller's streams, one per slot's scratch (a
  // stream always reuses the same scratch, so its launches never race)
  hipStream_t dev_stream[BWAGPU_NUM_SLOTS] = {};
  // ... and its own scratch (only the Dev buffers of these are used): the
  // submit/wait path's slots never share scratch with the device entry, so the
  // two entry points may run concurrently on one context
  Slot dev_scratch[BWAGPU_NUM_SLOTS];
  // bare ksw_extend2 task lists (bwagpu_extend_batch): grow-only, reused across calls
  DevBuf ex_tasks, ex_list, ex_q, ex_t, ex_res, ex_stats;
  // ksw_align2 batches (bwagpu_align2_*): grow-only, reused across calls
  DevBuf a2_tasks, a2_q, a2_t, a2_out, a2_scratch, a2_lists, a2_counts, a2_boff;
  // mem_reg2aln batches (bwagpu_reg2aln_batch)
  DevBuf r2_tasks, r2_q, r2_out, r2_cig, r2_md, r2_lists, r2_z, r2_stats;
  // bwagpu_reg2aln_device / bwagpu_reg2aln_jobs_device: their own scratch (keys, the one list, the
  // bin table and the scatter cursors, the HBM matrix slices, the job builder's block sums) and the
  // table's pinned copy.  r2d_done is recorded at the end of each of those calls and the next one's
  // stream waits for it before it touches the scratch.  Only once bwagpu_debug_reg2aln_times has
  // been used (r2d_timing): r2d_ev around the bin launches of the last call, the host's wait at the
  // read-back and its whole call.
  DevBuf r2d_keys, r2d_lists, r2d_tab, r2d_z, r2d_sums;
  HostBuf r2d_htab;
  // bwagpu_sam_text_device: the rg_id's bytes, the reads' text lengths and their block sums; ordered
  // by r2d_done like the scratch above
  DevBuf sam_scratch;
  hipEvent_t r2d_done = nullptr, r2d_ev[2] = {};
  bool r2d_pending = false, r2d_timing = false, r2d_timed = false;
  double r2d_wait_ms = 0, r2d_call_ms = 0;
  int32_t r2d_jobs = 0;
  // bins run concurrently on these (fork/join with events from the caller's stream)
  static constexpr int kA2Streams = 4;
  hipStream_t a2_st[kA2Streams] = {};
  hipEvent_t a2_fork = nullptr, a2_join[kA2Streams] = {};
  // seeding (capi_seed.hip: bwagpu_set_bwt / bwagpu_collect_intv): the resident
  // FM-index and the batch buffers
  DevBuf bwt_words, sa_d, sa_in, sa_out, occ_d, sup_d, sa_full;
  bwagpu::DevBwt bwt{};
  bool has_bwt = false;
  DevBuf sd_off, sd_seq, sd_out, sd_n, sd_scratch, sd_poff, sd_pack, sd_heavy, sd_dbg;
  // seeding's chaining (bwagpu_seqs2chains / bwagpu_seqs2regions): per read,
  // per SA position, the kbtree arenas, mem_seed_sw tasks, the packed chains
  DevBuf ch_npos, ch_posoff, ch_frac, ch_nout, ch_noseed, ch_nsw, ch_need, ch_swtab, ch_alt;
  DevBuf ch_kpos, ch_rbeg, ch_qinfo, ch_label, ch_score, ch_slist, ch_ord, ch_chains, ch_nodes;
  DevBuf ch_ochains, ch_oslist, ch_bins, ch_dbg;
  DevBuf ch_swoff, ch_swtasks, ch_swt, ch_swskip, ch_swres, ch_swscr;
  DevBuf ch_ocoff, ch_osoff, ch_rco, ch_cso, ch_rid, ch_cfrac, ch_out, ch_seeds;
  DevBuf ch_regoff, ch_regc;
  HostBuf chh_tot, chh_rco, chh_cso, chh_chains, chh_seeds, chh_regs, chh_n;
  HostBuf sdh_in;  // the reads of a seeding call, staged for the H2D
  hipEvent_t sdh_done = nullptr;  // recorded after the H2D out of sdh_in
  Slot ch_slot;  // chain2aln scratch of bwagpu_seqs2regions
  bwagpu::ChainStreams ch_cs{};  // created on first use
  bool has_alt = false;
  // the stages after mem_chain2aln (capi_stages.hip): the host-buffer entries' staging
  bwagpu::Staging stg;
  // region post-processing (bwagpu_regs_post*, bwagpu_set_regs_post): mem_opt_t.b,
  // the switch's options / flags / next batch's id0, the host entry's stats words
  int opt_b = 0;
  bwagpu_postopt_t post_opt{};
  int32_t post_flags = 0;
  int64_t post_id0 = 0;
  DevBuf rp_stats;
  // paired ends (bwagpu_pestat*, bwagpu_mate_rescue*): the lists and counters of
  // mem_pestat; mate rescue's per-pair work arrays, query pool, per-round task
  // lists / window pools / results
  DevBuf pe_isize, pe_cnt;
  DevBuf rs_pair, rs_soff, rs_tab, rs_toff, rs_boff, rs_qpool, rs_ctr, rs_scr;
  DevBuf rs_tasks[bwagpu::kRescueMaxRounds], rs_tpool[bwagpu::kRescueMaxRounds], rs_res[bwagpu::kRescueMaxRounds];
  int32_t rescue_drop = 0;  // bwagpu_debug_rescue_drop
  // bwagpu_debug_rescue_times: per round of the last call, events before the plan,
  // after it, after align2 and after the replay
  hipEvent_t rs_ev[4 * bwagpu::kRescueMaxRounds] = {};
  int rs_ev_rounds = 0;
  hipStream_t rs_ev_stream = nullptr;
  // primary marking and pair selection (bwagpu_mark_primary*, bwagpu_pair_select*):
  // the marking kernel's per-block scratch, the log table (filled once), the
  // pairing tables of the last call
  DevBuf ps_scratch, ps_log, ps_erfc;
  bool ps_log_ready = false;
  // the FPGA wire format (bwagpu_sw_stream)
  DevBuf st_buf, st_start, st_q, st_tasks, st_lists, st_seen, st_ctr, st_out;
  // bwt_extend calls tier 1 spends on a read before tier 2 (one wave per read)
  // takes it: ~p90 of the C2 batch's per-read counts (mean 666, p90 975)
  int seed_budget = 1024;
  int sup_shift = 32;  // bwagpu_debug_sup_shift: superblock size of the next set_bwt
  int dev_read_len = BWAGPU_MAX_READ_LEN;  // bwagpu_set_device_read_len
  // bwagpu_debug_fail_wait: after fail_after more successful waits, _wait
  // returns fail_code once (tests of the stage's recovery path)
  int fail_after = -1, fail_code = 0;
  // bwagpu_prof_*: event pairs around the dominant extension launches
  std::vector<hipEvent_t> prof_ev;
  int prof_used = 0;
  std::string err;
};

namespace bwagpu {

inline int fail(bwagpu_ctx_t* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

inline int hip_fail(bwagpu_ctx_t* c, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return fail(c, BWAGPU_E_NOMEM, m);
  return fail(c, BWAGPU_E_DEVICE, m);
}

#define HIPC(call, what)                             \
  do {                                               \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, what); \
  } while (0)
#define TRY(call)                     \
  do {                                \
    if (int rc_ = (call)) return rc_; \
  } while (0)

// a plan's refusal (stage_host.h, task_host.h): a bad argument has no text
inline int refuse(bwagpu_ctx_t* c, int code, const char* why) { return why && *why ? fail(c, code, why) : code; }

// the stream of a _device entry: the caller's, or slot[0]'s when it passes none
inline int entry_stream(bwagpu_ctx_t* ctx, void* stream, hipStream_t* st) {
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  *st = (hipStream_t)stream;
  if (!*st) HIPC(lazy_stream(ctx->slot[0], st), "hipStreamCreate");
  return BWAGPU_OK;
}

// The context's side streams (a2_st): the launches of one call run concurrently on up to kA2Streams
// of them.  side_fork makes `used` = min(kA2Streams, n_launches) of them wait for what `st` holds
// so far, launch k then goes to a2_st[k % used], and side_join makes `st` wait for them all.
inline int side_fork(bwagpu_ctx_t* ctx, hipStream_t st, size_t n_launches, int* used) {
  for (int i = 0; i < bwagpu_ctx::kA2Streams; ++i) {  // created on first use
    if (!ctx->a2_st[i]) HIPC(hipStreamCreateWithFlags(&ctx->a2_st[i], hipStreamNonBlocking), "stream");
    if (!ctx->a2_join[i]) HIPC(hipEventCreateWithFlags(&ctx->a2_join[i], hipEventDisableTiming), "event");
  }
  if (!ctx->a2_fork) HIPC(hipEventCreateWithFlags(&ctx->a2_fork, hipEventDisableTiming), "event");
  *used = (int)std::min<size_t>(bwagpu_ctx::kA2Streams, n_launches);
  HIPC(hipEventRecord(ctx->a2_fork, st), "event");
  for (int i = 0; i < *used; ++i) HIPC(hipStreamWaitEvent(ctx->a2_st[i], ctx->a2_fork, 0), "stream wait");
  return BWAGPU_OK;
}
inline int side_join(bwagpu_ctx_t* ctx, hipStream_t st, int used) {
  for (int i = 0; i < used; ++i) {
    HIPC(hipEventRecord(ctx->a2_join[i], ctx->a2_st[i]), "event");
    HIPC(hipStreamWaitEvent(st, ctx->a2_join[i], 0), "stream wait");
  }
  return BWAGPU_OK;
}

// The two events around a call's timed section; destroyed on every way out.
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  hipError_t start(hipStream_t st) {  // creates both, records the first
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    return e == hipSuccess ? hipEventRecord(e0, st) : e;
  }
  hipError_t stop(hipStream_t st) { return hipEventRecord(e1, st); }
  float ms() const {  // after the stream was synchronised
    float t = 0;
    (void)hipEventElapsedTime(&t, e0, e1);
    return t;
  }
};

// the post-processing pass over read spans in device memory (regpost.hip)
int enqueue_regpost(bwagpu_ctx_t* ctx, const bwagpu_postopt_t& po, int32_t flags, int64_t id0, int32_t n_reads,
                    const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off, const int32_t* rco,
                    const int32_t* cso, bwagpu_alnreg_t* regs, int32_t* n, int64_t* stats, hipStream_t st);

// mem_chain2aln over a batch in device memory (capi.hip): check_lds refuses options whose LDS row
// buffers do not fit, before anything is enqueued; enqueue_chain2aln then fills d_out / d_n on st
int check_lds(bwagpu_ctx_t* ctx, int lq_max);
int enqueue_chain2aln(bwagpu_ctx_t* ctx, Slot& s, const DevBatch& db, int lq_max, bwagpu_alnreg_t* d_out,
                      int32_t* d_n, int64_t* d_stats, hipStream_t st);

// One blocking host-buffer entry of a stage, on slot[0]'s stream:
//   begin();  up(...) / up_spans(...) / reserve(...);  uploaded();
//   start();  enqueue_*(..., st);  stop();
//   down(...);  finish();  then the entry adds its own ext_calls / rows / cells.
// up and down count the caller's arrays they move (h2d_bytes / d2h_bytes); a
// copy of fixed-size bookkeeping (stats words, counters, pes records, tables)
// is a plain hipMemcpyAsync on st between these calls and is not counted.
// kernel_ms spans start() .. stop().  Every method returns a BWAGPU_* code.
struct HostCall {
  bwagpu_ctx_t* ctx;
  Staging& g;
  hipStream_t st = nullptr;
  EventPair ev;
  int64_t h2d = 0, d2h = 0, hs[ST_N] = {};
  std::vector<int64_t> roff, soff, ooff;  // rebased offsets: pageable, alive until uploaded()
  bool open = false;                      // between begin() and finish()

  explicit HostCall(bwagpu_ctx_t* c) : ctx(c), g(c->stg) {}
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  // an entry that gives up half way: no copy may still read the offsets above or
  // the caller's arrays, or write the entry's locals, once it has returned
  ~HostCall() {
    if (open) (void)hipStreamSynchronize(st);
  }
  int begin() {
    if (int rc = entry_stream(ctx, nullptr, &st)) return rc;
    open = true;
    return BWAGPU_OK;
  }
  int done(hipError_t e, const char* what) { return e == hipSuccess ? BWAGPU_OK : hip_fail(ctx, e, what); }
  // at least one element, so that the kernels get a pointer
  int reserve(DevBuf& b, size_t bytes) { return done(b.ensure(std::max<size_t>(bytes, 1)), "hipMalloc"); }
  template <class T>
  int reserve(DevBuf& b, T*& out, size_t n) { return done(b.get(out, n), "hipMalloc"); }  // n elements of T -> out
  int up(DevBuf& b, const void* src, size_t bytes, size_t slack = 0) {  // slack: bytes a kernel may read past the end
    if (int rc = reserve(b, bytes + slack)) return rc;
    if (bytes) HIPC(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st), "H2D");
    h2d += (int64_t)bytes;
    return BWAGPU_OK;
  }
  int down(void* dst, const DevBuf& b, size_t bytes) {
    if (bytes) HIPC(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, st), "D2H");
    d2h += (int64_t)bytes;
    return BWAGPU_OK;
  }
  // regs[plan.lo, plan.hi), n and the reads' offsets into what is copied -> g.regs, g.n, g.reg_off
  int up_spans(const StagePlan& plan, size_t nr, const int64_t* reg_off, const bwagpu_alnreg_t* regs,
               const int32_t* n) {
    roff.resize(nr);
    for (size_t r = 0; r < nr; ++r) roff[r] = n[r] ? reg_off[r] - plan.lo : 0;
    if (int rc = up(g.regs, regs + plan.lo, sizeof(bwagpu_alnreg_t) * (size_t)(plan.hi - plan.lo))) return rc;
    if (int rc = up(g.reg_off, roff.data(), sizeof(int64_t) * nr)) return rc;
    return up(g.n, n, sizeof(int32_t) * nr);
  }
  // seq[plan.seq_lo, plan.seq_hi) and the reads' offsets into it -> g.seq, g.seq_off
  int up_seq(const StagePlan& plan, size_t nr, const int64_t* seq_off, const uint8_t* seq) {
    soff.resize(nr + 1);
    for (size_t r = 0; r <= nr; ++r) soff[r] = seq_off[r] - plan.seq_lo;
    if (int rc = up(g.seq, seq + plan.seq_lo, (size_t)(plan.seq_hi - plan.seq_lo), 1)) return rc;
    return up(g.seq_off, soff.data(), sizeof(int64_t) * (nr + 1));
  }
  // the output spans' offsets into out_regs[plan.out_lo, plan.out_hi) -> g.out_off; g.out_regs is reserved
  int up_out_off(const StagePlan& plan, size_t nr, const int64_t* out_off) {
    ooff.resize(nr + 1);
    for (size_t r = 0; r <= nr; ++r) ooff[r] = out_off[r] - plan.out_lo;
    if (int rc = reserve(g.out_regs, sizeof(bwagpu_alnreg_t) * (size_t)(plan.out_hi - plan.out_lo))) return rc;
    return up(g.out_off, ooff.data(), sizeof(int64_t) * (nr + 1));
  }
  int uploaded() { return done(hipStreamSynchronize(st), "H2D"); }  // the sources of the uploads may be pageable locals
  int start() { return done(ev.start(st), "event"); }
  int stop() { return done(ev.stop(st), "event"); }
  int finish(const char* what, const int64_t* d_stats = nullptr) {  // d_stats: the ST_* words the kernels added up
    if (d_stats) HIPC(hipMemcpyAsync(hs, d_stats, sizeof hs, hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipStreamSynchronize(st), what);
    open = false;
    bwagpu_stats_t& last = ctx->slot[0].last;
    last = bwagpu_stats_t{};
    last.kernel_ms = ev.ms();
    last.h2d_bytes = h2d;
    last.d2h_bytes = d2h;
    last.cells = hs[ST_CELLS];
    last.rows = hs[ST_ROWS];
    last.ext_calls = hs[ST_CALLS];
    return BWAGPU_OK;
  }
};

}  // namespace bwagpu
