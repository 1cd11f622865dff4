// capi_stages.hip — the C ABI's stages after mem_chain2aln (include/bwagpu.h):
// region post-processing, mem_pestat, mate rescue, primary marking and pair
// selection.  Each stage has an enqueue_* over device memory, a _device entry
// on the caller's stream, and a blocking host-buffer entry that stages the
// caller's arrays through the context's shared set (HostCall, ctx.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "align2.h"
#include "chain.h"
#include "ctx.h"
#include "engine.h"
#include "pairsel.h"
#include "regpost.h"
#include "rescue.h"
#include "stage_host.h"

using namespace bwagpu;

// the post-processing pass over read spans in device memory (regpost.hip)
int bwagpu::enqueue_regpost(bwagpu_ctx_t* ctx, const bwagpu_postopt_t& po, int32_t flags, int64_t id0, int32_t n_reads,
                            const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off, const int32_t* rco,
                            const int32_t* cso, bwagpu_alnreg_t* regs, int32_t* n, int64_t* stats, hipStream_t st) {
  RegPostArgs a{};
  a.n_reads = n_reads;
  a.flags = flags;
  a.id0 = id0;
  a.po = po;
  a.opt_b = ctx->opt_b;
  a.seq_off = seq_off;
  a.seq = seq;
  a.reg_off = reg_off;
  a.rco = rco;
  a.cso = cso;
  a.regs = regs;
  a.n = n;
  a.alt = ctx->has_alt ? ctx->ch_alt.as<uint8_t>() : nullptr;
  a.stats = stats;
  HIPC(launch_regpost(ctx->opt, ctx->ref, a, st), "regpost launch");
  return BWAGPU_OK;
}

// ------------------------------------------------------------------ region post-processing
extern "C" int bwagpu_set_regs_post(bwagpu_ctx_t* ctx, const bwagpu_postopt_t* popt, int32_t flags,
                                    int64_t id0_of_next_batch) {
  if (!ctx) return BWAGPU_E_INVAL;
  const char* why = "";
  if (int rc = post_flags_check(flags, &why)) return fail(ctx, rc, why);
  if (flags && !post_opt_ok(popt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_postopt_t");
  if (popt) ctx->post_opt = *popt;
  ctx->post_flags = flags;
  ctx->post_id0 = id0_of_next_batch;
  return BWAGPU_OK;
}

extern "C" int bwagpu_regs_post_device(bwagpu_ctx_t* ctx, const bwagpu_postopt_t* popt, int32_t flags, int64_t id0,
                                       const bwagpu_batch_t* b, const int64_t* dev_reg_off, bwagpu_alnreg_t* dev_regs,
                                       int32_t* dev_n, void* stream) {
  if (!ctx || !b) return BWAGPU_E_INVAL;
  const char* why = "";
  if (int rc = post_flags_check(flags, &why)) return fail(ctx, rc, why);
  if (!post_opt_ok(popt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_postopt_t");
  if (b->n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (b->n_reads == 0 || flags == 0) return BWAGPU_OK;
  if (!dev_regs || !dev_n || !b->seq_off || !b->seq || (!dev_reg_off && (!b->read_chain_off || !b->chain_seed_off)))
    return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  return enqueue_regpost(ctx, *popt, flags, id0, b->n_reads, b->seq_off, b->seq, dev_reg_off, b->read_chain_off,
                         b->chain_seed_off, dev_regs, dev_n, nullptr, st);
}

extern "C" int bwagpu_regs_post(bwagpu_ctx_t* ctx, const bwagpu_postopt_t* popt, int32_t flags, int64_t id0,
                                int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off,
                                bwagpu_alnreg_t* regs, int32_t* n) {
  if (!ctx) return BWAGPU_E_INVAL;
  StagePlan plan;
  const char* why = "";
  if (int rc = post_check(popt, flags, n_reads, seq_off, seq, reg_off, regs, n, &plan, &why)) return fail(ctx, rc, why);
  if (n_reads == 0 || flags == 0 || plan.n_regs == 0) return BWAGPU_OK;
  const size_t nr = (size_t)n_reads, span = (size_t)(plan.hi - plan.lo);
  int64_t hst[ST_N] = {};  // before hc: a copy into it may be in flight until hc is gone
  HostCall hc(ctx);
  Staging& g = hc.g;
  TRY(hc.begin());
  TRY(hc.up_spans(plan, nr, reg_off, regs, n));
  TRY(hc.up_seq(plan, nr, seq_off, seq));
  int64_t* d_stats = nullptr;
  HIPC(ctx->rp_stats.get(d_stats, ST_N), "hipMalloc");
  HIPC(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * ST_N, hc.st), "memset");
  TRY(hc.uploaded());
  TRY(hc.start());
  TRY(enqueue_regpost(ctx, *popt, flags, id0, n_reads, g.seq_off.as<int64_t>(), g.seq.as<uint8_t>(),
                      g.reg_off.as<int64_t>(), nullptr, nullptr, g.regs.as<bwagpu_alnreg_t>(), g.n.as<int32_t>(),
                      d_stats, hc.st));
  TRY(hc.stop());
  TRY(hc.down(regs + plan.lo, g.regs, sizeof(bwagpu_alnreg_t) * span));
  TRY(hc.down(n, g.n, sizeof(int32_t) * nr));
  HIPC(hipMemcpyAsync(hst, d_stats, sizeof(hst), hipMemcpyDeviceToHost, hc.st), "D2H");
  TRY(hc.finish("regpost execution"));
  ctx->slot[0].last.ext_calls = hst[ST_CALLS];
  if (hst[ST_ERR] & ERR_POST) return fail(ctx, BWAGPU_E_UNSUPPORTED, "a patch candidate's window exceeds 4096 bases");
  return BWAGPU_OK;
}

// ------------------------------------------------------------------ paired ends: mem_pestat, mate rescue
namespace {

// mem_pestat over spans in device memory (rescue.hip); pes: 4 records in device memory
int enqueue_pestat(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t& po, int32_t n_reads, const int64_t* reg_off,
                   const bwagpu_alnreg_t* regs, const int32_t* n, bwagpu_pestat_t* pes, hipStream_t st) {
  PestatArgs a{};
  a.n_pairs = n_reads >> 1;
  a.cap = 1;
  while (a.cap < a.n_pairs) a.cap <<= 1;
  a.po = po;
  a.reg_off = reg_off;
  a.regs = regs;
  a.n = n;
  HIPC(ctx->pe_isize.get(a.isize, 4 * (size_t)a.cap), "hipMalloc");
  HIPC(ctx->pe_cnt.get(a.cnt, 4), "hipMalloc");
  HIPC(hipMemsetAsync(a.cnt, 0, sizeof(int32_t) * 4, st), "memset");
  a.pes = pes;
  HIPC(launch_pestat(ctx->opt, ctx->ref, a, st), "pestat launch");
  return BWAGPU_OK;
}

struct RescueRun {
  int rounds = 0;
  int64_t tasks = 0;  // ksw_align2 tasks computed over all rounds
  float ms = 0;
};

// Mate rescue over device memory.  The counts of every round come to the host
// (stream waits); the last round's replay is left running on st.
int enqueue_rescue(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t& po, const bwagpu_pestat_t* dev_pes, int32_t n_reads,
                   int64_t seq_bytes, const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off,
                   const bwagpu_alnreg_t* regs, const int32_t* n, const int64_t* out_off, bwagpu_alnreg_t* out_regs,
                   int32_t* out_n, int32_t* status, int32_t* n_sw, hipStream_t st, RescueRun* run) {
  const int32_t np = n_reads >> 1;
  const size_t npz = (size_t)np;
  RescueArgs a{};
  a.n_pairs = np;
  a.po = po;
  a.pes = dev_pes;
  a.seq_off = seq_off;
  a.seq = seq;
  a.reg_off = reg_off;
  a.regs = regs;
  a.n = n;
  a.out_off = out_off;
  a.out_regs = out_regs;
  a.out_n = out_n;
  a.status = status;
  a.n_sw = n_sw;
  // per pair: pstate | nb0 | nslot | ntask | tbytes
  HIPC(ctx->rs_pair.ensure(sizeof(int32_t) * 5 * npz), "hipMalloc");
  int64_t *soff = nullptr, *toff = nullptr, *boff = nullptr, *tot = nullptr;  // the scans of nslot, ntask, tbytes
  HIPC(ctx->rs_soff.get(soff, npz + 1), "hipMalloc");
  HIPC(ctx->rs_toff.get(toff, npz + 1), "hipMalloc");
  HIPC(ctx->rs_boff.get(boff, npz + 1), "hipMalloc");
  HIPC(ctx->rs_qpool.ensure(2 * (size_t)seq_bytes + 64), "hipMalloc");
  HIPC(ctx->rs_ctr.get(a.ctr, RC_WORDS), "hipMalloc");
  HIPC(ctx->chh_tot.get(tot, 16), "hipHostMalloc");
  a.pstate = ctx->rs_pair.as<int32_t>();
  a.nb0 = a.pstate + npz;
  a.nslot = a.nb0 + npz;
  a.ntask = a.nslot + npz;
  a.tbytes = a.ntask + npz;
  a.slot_off = soff;
  a.task_off = toff;
  a.tb_off = boff;
  a.qpool = ctx->rs_qpool.as<uint8_t>();
  a.rc_base = seq_bytes;
  ctx->rs_ev_rounds = 0;
  ctx->rs_ev_stream = st;
  HIPC(launch_rescue_pool(a, st), "rescue_pool launch");
  HIPC(launch_rescue_init(ctx->opt, a, st), "rescue_init launch");
  HIPC(launch_scan_i32(a.nslot, soff, np, st), "scan launch");
  HIPC(hipMemcpyAsync(tot + 8, soff + np, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  const int64_t S = tot[8];
  HIPC(ctx->rs_tab.get(a.tab, (size_t)S), "hipMalloc");
  HIPC(hipMemsetAsync(a.tab, 0xff, sizeof(int32_t) * (size_t)std::max<int64_t>(S, 1), st), "memset");  // RS_NONE
  HIPC(hipMemsetAsync(a.ctr, 0, sizeof(int32_t) * RC_WORDS, st), "memset");
  for (int round = 0; round < po.max_rounds; ++round) {
    a.round = round;
    a.drop = round == 0 ? ctx->rescue_drop : 0;
    HIPC(hipMemsetAsync(a.ctr + RC_PENDING, 0, sizeof(int32_t), st), "memset");
    hipEvent_t* ev = ctx->rs_ev + 4 * round;
    for (int k = 0; k < 4; ++k)
      if (!ev[k]) HIPC(hipEventCreate(&ev[k]), "hipEventCreate");
    HIPC(hipEventRecord(ev[0], st), "event");
    HIPC(launch_rescue_plan(ctx->opt, ctx->ref, a, false, st), "rescue_plan launch");
    HIPC(launch_scan_i32(a.ntask, toff, np, st), "scan launch");
    HIPC(launch_scan_i32(a.tbytes, boff, np, st), "scan launch");
    HIPC(hipMemcpyAsync(tot + 9, toff + np, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipMemcpyAsync(tot + 10, boff + np, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipStreamSynchronize(st), "sync");
    const int64_t T = tot[9], B = tot[10];
    if (T >= (int64_t)1 << kRescueIdxBits) return fail(ctx, BWAGPU_E_UNSUPPORTED, "too many rescue alignments in one batch");
    if (T) {
      bwagpu_kswr_t* res = nullptr;
      HIPC(ctx->rs_tasks[round].get(a.tasks, (size_t)T), "hipMalloc");
      HIPC(ctx->rs_tpool[round].ensure((size_t)B + 64), "hipMalloc");
      HIPC(ctx->rs_res[round].get(res, (size_t)T), "hipMalloc");
      HIPC(ctx->rs_scr.ensure(8 * ((size_t)B + (size_t)T)), "hipMalloc");
      a.tpool = ctx->rs_tpool[round].as<uint8_t>();
      a.res[round] = res;
      HIPC(launch_rescue_plan(ctx->opt, ctx->ref, a, true, st), "rescue_plan launch");
      HIPC(hipEventRecord(ev[1], st), "event");
      if (int rc = bwagpu_align2_device(ctx, (int32_t)T, a.tasks, a.qpool, a.tpool, res, ctx->rs_scr.p, st)) return rc;
      run->tasks += T;
    } else {
      HIPC(hipEventRecord(ev[1], st), "event");
    }
    HIPC(hipEventRecord(ev[2], st), "event");
    HIPC(launch_rescue_apply(ctx->opt, ctx->ref, a, st), "rescue_apply launch");
    HIPC(hipEventRecord(ev[3], st), "event");
    run->rounds = ctx->rs_ev_rounds = round + 1;
    if (round + 1 == po.max_rounds) break;
    HIPC(hipMemcpyAsync(tot + 11, a.ctr, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipStreamSynchronize(st), "sync");
    if (reinterpret_cast<const int32_t*>(tot + 11)[RC_PENDING] == 0) break;
  }
  return BWAGPU_OK;
}

}  // namespace

extern "C" int bwagpu_debug_rescue_drop(bwagpu_ctx_t* ctx, int32_t k) {
  if (!ctx || k < 0) return BWAGPU_E_INVAL;
  ctx->rescue_drop = k;
  return BWAGPU_OK;
}

extern "C" int bwagpu_debug_rescue_times(bwagpu_ctx_t* ctx, double* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  out[0] = out[1] = out[2] = 0;
  out[3] = ctx->rs_ev_rounds;
  if (ctx->rs_ev_rounds == 0) return BWAGPU_OK;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  HIPC(hipEventSynchronize(ctx->rs_ev[4 * (ctx->rs_ev_rounds - 1) + 3]), "event sync");
  for (int r = 0; r < ctx->rs_ev_rounds; ++r)
    for (int k = 0; k < 3; ++k) {
      float ms = 0;
      HIPC(hipEventElapsedTime(&ms, ctx->rs_ev[4 * r + k], ctx->rs_ev[4 * r + k + 1]), "event time");
      out[k] += ms;
    }
  return BWAGPU_OK;
}

extern "C" int bwagpu_pestat_device(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t* popt, int32_t n_reads,
                                    const int64_t* dev_reg_off, const bwagpu_alnreg_t* dev_regs, const int32_t* dev_n,
                                    bwagpu_pestat_t* dev_pes, void* stream) {
  if (!ctx) return BWAGPU_E_INVAL;
  if (!pair_opt_ok(popt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_pairopt_t");
  if (n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (!dev_pes || ((n_reads >> 1) && (!dev_reg_off || !dev_regs || !dev_n))) return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  return enqueue_pestat(ctx, *popt, n_reads, dev_reg_off, dev_regs, dev_n, dev_pes, st);
}

extern "C" int bwagpu_pestat(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t* popt, int32_t n_reads, const int64_t* reg_off,
                             const bwagpu_alnreg_t* regs, const int32_t* n, bwagpu_pestat_t* pes) {
  if (!ctx) return BWAGPU_E_INVAL;
  StagePlan plan;
  const char* why = "";
  if (int rc = pestat_check(popt, n_reads, reg_off, regs, n, pes, &plan, &why)) return fail(ctx, rc, why);
  const size_t nr = (size_t)(n_reads & ~1);
  HostCall hc(ctx);
  Staging& g = hc.g;
  TRY(hc.begin());
  TRY(hc.up_spans(plan, nr, reg_off, regs, n));
  TRY(hc.reserve(g.pes, sizeof(bwagpu_pestat_t) * 4));
  TRY(hc.uploaded());
  TRY(hc.start());
  TRY(enqueue_pestat(ctx, *popt, (int32_t)nr, g.reg_off.as<int64_t>(), g.regs.as<bwagpu_alnreg_t>(), g.n.as<int32_t>(),
                     g.pes.as<bwagpu_pestat_t>(), hc.st));
  TRY(hc.stop());
  HIPC(hipMemcpyAsync(pes, g.pes.p, sizeof(bwagpu_pestat_t) * 4, hipMemcpyDeviceToHost, hc.st), "D2H");
  return hc.finish("pestat execution");
}

extern "C" int bwagpu_mate_rescue_device(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t* popt, const bwagpu_pestat_t* dev_pes,
                                         const bwagpu_batch_t* b, const int64_t* dev_reg_off,
                                         const bwagpu_alnreg_t* dev_regs, const int32_t* dev_n,
                                         const int64_t* dev_out_off, bwagpu_alnreg_t* dev_out_regs, int32_t* dev_out_n,
                                         int32_t* dev_status, int32_t* dev_n_sw, void* stream) {
  if (!ctx || !b) return BWAGPU_E_INVAL;
  if (!pair_opt_ok(popt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_pairopt_t");
  if (b->n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (b->n_reads & 1) return fail(ctx, BWAGPU_E_INVAL, "odd read count: reads 2i and 2i+1 are a pair");
  if (!dev_pes) return fail(ctx, BWAGPU_E_INVAL, "NULL pes");
  if (const char* why = align2_opt_unsupported(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, why);
  if (!align2_byte_ok(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, kA2ByteRescueWhy);
  if (b->n_reads == 0) return BWAGPU_OK;
  if (!b->seq_off || !b->seq || b->seq_bytes < 0 || !dev_reg_off || !dev_regs || !dev_n || !dev_out_off ||
      !dev_out_regs || !dev_out_n || !dev_status || !dev_n_sw)
    return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  bwagpu_pestat_t hp[4];  // the windows' size bound needs the ranges here
  HIPC(hipMemcpyAsync(hp, dev_pes, sizeof(hp), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  const char* why = "";
  if (int rc = pes_check(hp, &why)) return fail(ctx, rc, why);
  RescueRun run;
  int rc = enqueue_rescue(ctx, *popt, dev_pes, b->n_reads, b->seq_bytes, b->seq_off, b->seq, dev_reg_off, dev_regs,
                          dev_n, dev_out_off, dev_out_regs, dev_out_n, dev_status, dev_n_sw, st, &run);
  if (rc) return rc;
  Slot& s0 = ctx->slot[0];
  s0.last = bwagpu_stats_t{};
  s0.last.ext_calls = run.tasks;
  s0.last.rows = run.rounds;
  return BWAGPU_OK;
}

extern "C" int bwagpu_mate_rescue(bwagpu_ctx_t* ctx, const bwagpu_pairopt_t* popt, const bwagpu_pestat_t* pes,
                                  int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, const int64_t* reg_off,
                                  const bwagpu_alnreg_t* regs, const int32_t* n, const int64_t* out_off,
                                  bwagpu_alnreg_t* out_regs, int32_t* out_n, int32_t* status, int32_t* n_sw) {
  if (!ctx) return BWAGPU_E_INVAL;
  StagePlan plan;
  const char* why = "";
  if (int rc = rescue_check(popt, pes, n_reads, seq_off, seq, reg_off, regs, n, out_off, out_regs, out_n, status, n_sw,
                            &plan, &why))
    return fail(ctx, rc, why);
  if (const char* w = align2_opt_unsupported(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, w);
  if (!align2_byte_ok(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, kA2ByteRescueWhy);
  if (n_reads == 0) return BWAGPU_OK;
  const size_t nr = (size_t)n_reads, np = nr / 2;
  int32_t hctr[RC_WORDS] = {};  // before hc: a copy into it may be in flight until hc is gone
  HostCall hc(ctx);
  Staging& g = hc.g;
  TRY(hc.begin());
  TRY(hc.up_spans(plan, nr, reg_off, regs, n));
  TRY(hc.up_seq(plan, nr, seq_off, seq));
  TRY(hc.up_out_off(plan, nr, out_off));
  TRY(hc.reserve(g.out_n, sizeof(int32_t) * nr));
  TRY(hc.reserve(g.status, sizeof(int32_t) * np));
  TRY(hc.reserve(g.n_sw, sizeof(int32_t) * np));
  TRY(hc.reserve(g.pes, sizeof(bwagpu_pestat_t) * 4));
  HIPC(hipMemcpyAsync(g.pes.p, pes, sizeof(bwagpu_pestat_t) * 4, hipMemcpyHostToDevice, hc.st), "H2D");
  TRY(hc.uploaded());
  TRY(hc.start());
  RescueRun run;
  TRY(enqueue_rescue(ctx, *popt, g.pes.as<bwagpu_pestat_t>(), n_reads, plan.seq_hi - plan.seq_lo,
                     g.seq_off.as<int64_t>(), g.seq.as<uint8_t>(), g.reg_off.as<int64_t>(), g.regs.as<bwagpu_alnreg_t>(),
                     g.n.as<int32_t>(), g.out_off.as<int64_t>(), g.out_regs.as<bwagpu_alnreg_t>(), g.out_n.as<int32_t>(),
                     g.status.as<int32_t>(), g.n_sw.as<int32_t>(), hc.st, &run));
  TRY(hc.stop());
  // only the regions of every span that the pass wrote: spans are copied back whole
  TRY(hc.down(out_regs + plan.out_lo, g.out_regs, sizeof(bwagpu_alnreg_t) * (size_t)(plan.out_hi - plan.out_lo)));
  TRY(hc.down(out_n, g.out_n, sizeof(int32_t) * nr));
  TRY(hc.down(status, g.status, sizeof(int32_t) * np));
  TRY(hc.down(n_sw, g.n_sw, sizeof(int32_t) * np));
  HIPC(hipMemcpyAsync(hctr, ctx->rs_ctr.p, sizeof(hctr), hipMemcpyDeviceToHost, hc.st), "D2H");
  TRY(hc.finish("mate rescue execution"));
  bwagpu_stats_t& last = ctx->slot[0].last;
  last.ext_calls = run.tasks;
  last.rows = run.rounds;
  last.cells = hctr[RC_USED];
  return BWAGPU_OK;
}

// ------------------------------------------------------------------ paired ends: primary marking, pair selection
namespace {

int sel_tmp(const bwagpu_ctx_t* ctx) {  // bwamem.c:505-507
  int tmp = ctx->opt.a + ctx->opt_b;
  tmp = std::max(tmp, ctx->opt.o_del + ctx->opt.e_del);
  return std::max(tmp, ctx->opt.o_ins + ctx->opt.e_ins);
}

int enqueue_mark(bwagpu_ctx_t* ctx, const bwagpu_selopt_t& so, int64_t id0, int32_t n_reads, const int64_t* reg_off,
                 bwagpu_alnreg_t* regs, const int32_t* n, int32_t* n_pri, int32_t* status, hipStream_t st) {
  MarkArgs a{};
  HIPC(ctx->ps_scratch.get(a.scratch, (size_t)kSelCap * kSelMaxBlocks), "hipMalloc");
  a.n_reads = n_reads;
  a.tmp = sel_tmp(ctx);
  a.mask_level = so.mask_level;
  a.id0 = id0;
  a.reg_off = reg_off;
  a.regs = regs;
  a.n = n;
  a.n_pri = n_pri;
  a.status = status;
  HIPC(launch_mark_primary(a, st), "mark_primary launch");
  return BWAGPU_OK;
}

// hpes: the four records on the host.  The tables go to the device before the
// launch (the call waits for the copies: their sources are pageable).
int enqueue_pairsel(bwagpu_ctx_t* ctx, const bwagpu_selopt_t& so, const bwagpu_pestat_t* hpes, int64_t pair_id0,
                    int32_t n_reads, const int64_t* reg_off, bwagpu_alnreg_t* regs, const int32_t* n,
                    const int32_t* n_pri, const int32_t* in_status, bwagpu_pairsel_t* sel, int32_t* out_mapq,
                    hipStream_t st) {
  if (!ctx->ps_log_ready) {
    std::vector<double> lg((size_t)kSelLogN);
    fill_log_table(lg.data(), kSelLogN);
    double* d_lg = nullptr;
    HIPC(ctx->ps_log.get(d_lg, (size_t)kSelLogN), "hipMalloc");
    HIPC(hipMemcpyAsync(d_lg, lg.data(), sizeof(double) * (size_t)kSelLogN, hipMemcpyHostToDevice, st), "H2D");
    HIPC(hipStreamSynchronize(st), "H2D");
    ctx->ps_log_ready = true;
  }
  int64_t len[4], total = 0;
  for (int r = 0; r < 4; ++r) total += len[r] = erfc_table_len(hpes[r]);
  std::vector<double> tab((size_t)total);
  double* d_erfc = nullptr;
  HIPC(ctx->ps_erfc.get(d_erfc, tab.size()), "hipMalloc");
  PairSelArgs a{};
  int64_t at = 0;
  for (int r = 0; r < 4; ++r) {
    a.pes[r] = hpes[r];
    a.erfc_tab[r] = d_erfc + at;
    if (len[r]) fill_erfc_table(hpes[r], tab.data() + at);
    at += len[r];
  }
  if (total) {
    HIPC(hipMemcpyAsync(d_erfc, tab.data(), sizeof(double) * (size_t)total, hipMemcpyHostToDevice, st), "H2D");
    HIPC(hipStreamSynchronize(st), "H2D");
  }
  a.n_pairs = n_reads >> 1;
  a.a = ctx->opt.a;
  a.b = ctx->opt_b;
  a.tmp = sel_tmp(ctx);
  a.so = so;
  a.pair_id0 = pair_id0;
  a.log_tab = ctx->ps_log.as<double>();
  a.log_n = kSelLogN;
  a.reg_off = reg_off;
  a.regs = regs;
  a.n = n;
  a.n_pri = n_pri;
  a.in_status = in_status;
  a.sel = sel;
  a.out_mapq = out_mapq;
  HIPC(launch_pair_select(ctx->ref, a, st), "pair_select launch");
  return BWAGPU_OK;
}

}  // namespace

extern "C" int bwagpu_mark_primary_device(bwagpu_ctx_t* ctx, const bwagpu_selopt_t* sopt, int64_t id0, int32_t n_reads,
                                          const int64_t* dev_reg_off, bwagpu_alnreg_t* dev_regs, const int32_t* dev_n,
                                          int32_t* dev_n_pri, int32_t* dev_status, void* stream) {
  if (!ctx) return BWAGPU_E_INVAL;
  if (!sel_opt_ok(sopt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_selopt_t");
  if (n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (n_reads == 0) return BWAGPU_OK;
  if (!dev_reg_off || !dev_regs || !dev_n || !dev_n_pri || !dev_status) return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  return enqueue_mark(ctx, *sopt, id0, n_reads, dev_reg_off, dev_regs, dev_n, dev_n_pri, dev_status, st);
}

extern "C" int bwagpu_mark_primary(bwagpu_ctx_t* ctx, const bwagpu_selopt_t* sopt, int64_t id0, int32_t n_reads,
                                   const int64_t* reg_off, bwagpu_alnreg_t* regs, const int32_t* n, int32_t* n_pri,
                                   int32_t* status) {
  if (!ctx) return BWAGPU_E_INVAL;
  StagePlan plan;
  const char* why = "";
  if (int rc = mark_check(sopt, n_reads, reg_off, regs, n, n_pri, status, &plan, &why)) return fail(ctx, rc, why);
  if (n_reads == 0) return BWAGPU_OK;
  const size_t nr = (size_t)n_reads, span = (size_t)(plan.hi - plan.lo);
  HostCall hc(ctx);
  Staging& g = hc.g;
  TRY(hc.begin());
  TRY(hc.up_spans(plan, nr, reg_off, regs, n));
  TRY(hc.reserve(g.n_pri, sizeof(int32_t) * nr));
  TRY(hc.reserve(g.status, sizeof(int32_t) * nr));
  TRY(hc.uploaded());
  TRY(hc.start());
  TRY(enqueue_mark(ctx, *sopt, id0, n_reads, g.reg_off.as<int64_t>(), g.regs.as<bwagpu_alnreg_t>(), g.n.as<int32_t>(),
                   g.n_pri.as<int32_t>(), g.status.as<int32_t>(), hc.st));
  TRY(hc.stop());
  TRY(hc.down(regs + plan.lo, g.regs, sizeof(bwagpu_alnreg_t) * span));
  TRY(hc.down(n_pri, g.n_pri, sizeof(int32_t) * nr));
  TRY(hc.down(status, g.status, sizeof(int32_t) * nr));
  return hc.finish("mark_primary execution");
}

extern "C" int bwagpu_pair_select_device(bwagpu_ctx_t* ctx, const bwagpu_selopt_t* sopt, const bwagpu_pestat_t* dev_pes,
                                         int64_t pair_id0, int32_t n_reads, const int64_t* dev_reg_off,
                                         bwagpu_alnreg_t* dev_regs, const int32_t* dev_n, const int32_t* dev_n_pri,
                                         const int32_t* dev_in_status, bwagpu_pairsel_t* dev_sel,
                                         int32_t* dev_out_mapq, void* stream) {
  if (!ctx) return BWAGPU_E_INVAL;
  if (!sel_opt_ok(sopt)) return fail(ctx, BWAGPU_E_INVAL, "bad bwagpu_selopt_t");
  const char* why = "";
  if (int rc = sel_flags_check(sopt->flags, &why)) return fail(ctx, rc, why);
  if (n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (n_reads & 1) return fail(ctx, BWAGPU_E_INVAL, "odd read count: reads 2i and 2i+1 are a pair");
  if (!dev_pes) return fail(ctx, BWAGPU_E_INVAL, "NULL pes");
  if (n_reads == 0) return BWAGPU_OK;
  if (!dev_reg_off || !dev_regs || !dev_n || !dev_n_pri || !dev_sel || !dev_out_mapq)
    return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  bwagpu_pestat_t hp[4];  // the pairing tables are made from the ranges here
  HIPC(hipMemcpyAsync(hp, dev_pes, sizeof(hp), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  if (int rc = pes_check(hp, &why)) return fail(ctx, rc, why);
  return enqueue_pairsel(ctx, *sopt, hp, pair_id0, n_reads, dev_reg_off, dev_regs, dev_n, dev_n_pri, dev_in_status,
                         dev_sel, dev_out_mapq, st);
}

extern "C" int bwagpu_pair_select(bwagpu_ctx_t* ctx, const bwagpu_selopt_t* sopt, const bwagpu_pestat_t* pes,
                                  int64_t pair_id0, int32_t n_reads, const int64_t* reg_off, bwagpu_alnreg_t* regs,
                                  const int32_t* n, const int32_t* n_pri, const int32_t* in_status,
                                  bwagpu_pairsel_t* sel, int32_t* out_mapq) {
  if (!ctx) return BWAGPU_E_INVAL;
  StagePlan plan;
  const char* why = "";
  if (int rc = pairsel_check(sopt, pes, n_reads, reg_off, regs, n, n_pri, sel, out_mapq, ctx->ref.n_seqs, &plan, &why))
    return fail(ctx, rc, why);
  if (n_reads == 0) return BWAGPU_OK;
  const size_t nr = (size_t)n_reads, np = nr / 2, span = (size_t)(plan.hi - plan.lo);
  HostCall hc(ctx);
  Staging& g = hc.g;
  TRY(hc.begin());
  TRY(hc.up_spans(plan, nr, reg_off, regs, n));
  // regions between the spans keep the caller's out_mapq
  TRY(hc.up(g.mapq, out_mapq + plan.lo, sizeof(int32_t) * span));
  TRY(hc.up(g.n_pri, n_pri, sizeof(int32_t) * nr));
  if (in_status) TRY(hc.up(g.status, in_status, sizeof(int32_t) * np));
  TRY(hc.reserve(g.sel, sizeof(bwagpu_pairsel_t) * np));
  TRY(hc.uploaded());
  TRY(hc.start());
  TRY(enqueue_pairsel(ctx, *sopt, pes, pair_id0, n_reads, g.reg_off.as<int64_t>(), g.regs.as<bwagpu_alnreg_t>(),
                      g.n.as<int32_t>(), g.n_pri.as<int32_t>(), in_status ? g.status.as<int32_t>() : nullptr,
                      g.sel.as<bwagpu_pairsel_t>(), g.mapq.as<int32_t>(), hc.st));
  TRY(hc.stop());
  TRY(hc.down(regs + plan.lo, g.regs, sizeof(bwagpu_alnreg_t) * span));
  TRY(hc.down(out_mapq + plan.lo, g.mapq, sizeof(int32_t) * span));
  TRY(hc.down(sel, g.sel, sizeof(bwagpu_pairsel_t) * np));
  return hc.finish("pair_select execution");
}

