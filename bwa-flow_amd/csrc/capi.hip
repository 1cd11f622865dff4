// capi.hip — the core of the C ABI declared in include/bwagpu.h: the context's
// lifecycle, the side-stream probe and choice, mem_chain2aln's entries (submit /
// wait / stage / results / device) with their dense-result kernels, and the
// debug and profiling entries.  The stages after mem_chain2aln are in
// capi_stages.hip, the task-list entries in capi_tasks.hip, seeding and
// chaining in capi_seed.hip; a batch's host-side checks and staging copy are
// plain C++ in batch_host.h.
//
// One context = one device.  It owns the HBM-resident reference (pac +
// contig table), the scoring options, and BWAGPU_NUM_SLOTS independent
// submission slots, each with its own HIP stream, device buffers, pinned
// host staging and events — the MI355X form of the reference's two
// ping-ponged SWTask objects (src/fpga/FPGAPipeline.cpp:373-386,
// SWTask.cpp:40-104).  No C++ exception crosses the ABI.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "batch_host.h"
#include "ctx.h"
#include "engine.h"
#include "regpost.h"

using namespace bwagpu;

namespace {


// Side-stream probes.  HIP maps every stream of the process onto one of
// GPU_MAX_HW_QUEUES hardware queues (4 on the pool's boxes), and work on two
// streams that share a queue runs in submission order: a selection side
// stream on the same queue as a caller stream serializes the two (the GRCh38
// regime leg of round 4: 2.56 against 1.75 ms per batch).
// Whether two streams share a queue is measured: a ~150 us spin on `a`, then
// an empty kernel on `b`; b done while a still spins = separate queues.
__global__ void side_probe_spin(uint64_t ticks) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
__global__ void side_probe_nop() {}

bool streams_concurrent(hipStream_t a, hipStream_t b) {
  hipEvent_t ea = nullptr, eb = nullptr;
  if (hipEventCreateWithFlags(&ea, hipEventDisableTiming) != hipSuccess) return false;
  if (hipEventCreateWithFlags(&eb, hipEventDisableTiming) != hipSuccess) {
    (void)hipEventDestroy(ea);
    return false;
  }
  hipLaunchKernelGGL(side_probe_spin, dim3(1), dim3(64), 0, a, (uint64_t)15000);
  bool conc = false;
  if (hipGetLastError() == hipSuccess && hipEventRecord(ea, a) == hipSuccess) {
    hipLaunchKernelGGL(side_probe_nop, dim3(1), dim3(64), 0, b);
    if (hipGetLastError() == hipSuccess && hipEventRecord(eb, b) == hipSuccess &&
        hipEventSynchronize(eb) == hipSuccess)
      conc = hipEventQuery(ea) == hipErrorNotReady;
  }
  (void)hipEventSynchronize(ea);
  (void)hipEventDestroy(ea);
  (void)hipEventDestroy(eb);
  return conc;
}

// Per-read offsets of the dense result layout: off[r] = n[0] + ... + n[r-1]
// (one workgroup; a batch has < 2^31 regions), written to the device (for the
// copy) and to pinned host memory (for the caller).
constexpr int kDenseScanBlock = 1024;
__global__ void __launch_bounds__(kDenseScanBlock) dense_scan_kernel(const int32_t* __restrict__ n, int nr,
                                                                     int32_t* __restrict__ off,
                                                                     int32_t* __restrict__ h_off) {
  __shared__ int32_t part[kDenseScanBlock];
  const int t = (int)threadIdx.x;
  const int per = (nr + kDenseScanBlock - 1) / kDenseScanBlock;
  const int r0 = min(t * per, nr), r1 = min(r0 + per, nr);
  int sum = 0;
  for (int r = r0; r < r1; ++r) sum += n[r];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kDenseScanBlock; d <<= 1) {  // inclusive scan of the parts
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int r = r0; r < r1; ++r) {
    off[r] = run;
    h_off[r] = run;
    run += n[r];
  }
  if (t == kDenseScanBlock - 1) {
    off[nr] = part[t];
    h_off[nr] = part[t];
  }
}

// Regions of read r from its slots (chain_seed_off[read_chain_off[r]], the
// ABI's layout) to dense[off[r] ..], 16 lanes per read, 8-byte words: the
// D2H moves the sum of n (~1.8 regions per read on C2) instead of every seed slot.
__global__ void __launch_bounds__(256) dense_copy_kernel(const bwagpu_alnreg_t* __restrict__ out,
                                                         const int32_t* __restrict__ n,
                                                         const int32_t* __restrict__ off,
                                                         const int32_t* __restrict__ rco,
                                                         const int32_t* __restrict__ cso, int nr,
                                                         bwagpu_alnreg_t* __restrict__ dense) {
  constexpr int kW = (int)(sizeof(bwagpu_alnreg_t) / 8);
  const int r = (int)((blockIdx.x * 256u + threadIdx.x) >> 4), l = (int)(threadIdx.x & 15);
  if (r >= nr) return;
  const int words = n[r] * kW;
  const uint2* src = reinterpret_cast<const uint2*>(out + cso[rco[r]]);
  uint2* dst = reinterpret_cast<uint2*>(dense + off[r]);
  for (int w = l; w < words; w += 16) dst[w] = src[w];
}

}  // namespace

namespace {

bool make_opt(const bwagpu_opt_t* o, DevOpt* d, std::string* why) {
  if (!o) { *why = "opt is NULL"; return false; }
  if (o->e_del <= 0 || o->e_ins <= 0) { *why = "gap extension penalties must be > 0"; return false; }
  if (o->w < 0 || o->a < 0) { *why = "negative band width or match score"; return false; }
  // bounds under which the kernels' integer forms of the reference's double
  // expressions (cal_max_gap, the ksw_extend2 band clamp) are exact
  if (o->a > 127 || o->e_del > 65535 || o->e_ins > 65535 || o->o_del < 0 || o->o_del > 65535 || o->o_ins < 0 ||
      o->o_ins > 65535 || o->pen_clip5 < 0 || o->pen_clip5 >= (1 << 20) || o->pen_clip3 < 0 ||
      o->pen_clip3 >= (1 << 20) || o->w > (1 << 20)) {
    *why = "scoring option out of range";
    return false;
  }
  memset(d, 0, sizeof(*d));
  d->a = o->a;
  d->o_del = o->o_del;
  d->e_del = o->e_del;
  d->o_ins = o->o_ins;
  d->e_ins = o->e_ins;
  d->oe_del = o->o_del + o->e_del;
  d->oe_ins = o->o_ins + o->e_ins;
  d->pen_clip5 = o->pen_clip5;
  d->pen_clip3 = o->pen_clip3;
  d->w = o->w;
  d->zdrop = o->zdrop;
  int mx = 0;  // ksw.c:397-398 — max over the m*m matrix, starting from 0
  for (int i = 0; i < 25; ++i) mx = std::max<int>(mx, o->mat[i]);
  d->max_mat = mx;
  d->row_bound = 1;
  memcpy(d->mat, o->mat, 25);
  for (int q = 0; q < 5; ++q) {
    uint32_t w = 0;
    for (int t = 0; t < 4; ++t) w |= (uint32_t)(uint8_t)o->mat[t * 5 + q] << (8 * t);
    d->qprof[q] = w;
    d->qprof4[q] = o->mat[20 + q];
  }
  return true;
}

int create_common(int device, const bwagpu_opt_t* opt, const bwagpu_bns_t* bns, bwagpu_ctx_t** out,
                  bwagpu_ctx_t** made) {
  if (!out || !bns || bns->l_pac <= 0 || bns->n_seqs <= 0 || !bns->ann_offset || !bns->ann_len)
    return BWAGPU_E_INVAL;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return BWAGPU_E_NODEVICE;
  if (device < 0 || device >= n) return BWAGPU_E_NODEVICE;
  bwagpu_ctx_t* ctx = new (std::nothrow) bwagpu_ctx_t();
  if (!ctx) return BWAGPU_E_NOMEM;
  std::string why;
  if (!make_opt(opt, &ctx->opt, &why)) {
    delete ctx;
    return BWAGPU_E_INVAL;
  }
  ctx->device = device;
  ctx->opt_b = opt->b;
  ctx->ext_form = set_ext_form(-1);
  ctx->ext_short = ext_short_default();
  ctx->ext_short_fill = ext_short_fill_default();
  ctx->light_pack = light_pack_default();
  ctx->ungapped = ungapped_default();
  ctx->ungapped_right = ungapped_right_default();
  ctx->emu_finish = emu_finish_default();
  ctx->fused_launches = fused_launches_default();
  *made = ctx;
  HIPC(hipSetDevice(device), "hipSetDevice");
  HIPC(hipMalloc(&ctx->d_ann_off, sizeof(int64_t) * bns->n_seqs), "hipMalloc(ann_offset)");
  HIPC(hipMalloc(&ctx->d_ann_len, sizeof(int32_t) * bns->n_seqs), "hipMalloc(ann_len)");
  HIPC(hipMemcpy(ctx->d_ann_off, bns->ann_offset, sizeof(int64_t) * bns->n_seqs, hipMemcpyHostToDevice),
       "upload ann_offset");
  HIPC(hipMemcpy(ctx->d_ann_len, bns->ann_len, sizeof(int32_t) * bns->n_seqs, hipMemcpyHostToDevice),
       "upload ann_len");
  for (auto& s : ctx->slot) {
    HIPC(hipEventCreate(&s.ev0), "hipEventCreate");
    HIPC(hipEventCreate(&s.ev1), "hipEventCreate");
    HIPC(hipEventCreate(&s.ev2), "hipEventCreate");
    HIPC(hipEventCreate(&s.ev3), "hipEventCreate");
  }
  ctx->ref.l_pac = bns->l_pac;
  ctx->ref.n_seqs = bns->n_seqs;
  ctx->ref.ann_offset = ctx->d_ann_off;
  ctx->ref.ann_len = ctx->d_ann_len;
  return BWAGPU_OK;
}

// every Slot of a context whose spec path may hold a side stream
std::vector<Slot*> all_slots(bwagpu_ctx_t* ctx) {
  std::vector<Slot*> v;
  for (auto& x : ctx->slot) v.push_back(&x);
  for (auto& x : ctx->dev_scratch) v.push_back(&x);
  v.push_back(&ctx->ch_slot);
  return v;
}

void destroy_ctx(bwagpu_ctx_t* ctx) {
  if (!ctx) return;
  // 1. every wait, free and destroy below is on the context's device, whatever the calling thread had current
  (void)hipSetDevice(ctx->device);
  // 2. before anything is freed: every stream and pending event the context can have work on (only
  //    those: other contexts and the caller's own streams share the device).  A half-built context
  //    has null handles.
  std::vector<hipStream_t> busy = ctx->side_graveyard;
  for (Slot* s : all_slots(ctx)) busy.insert(busy.end(), {s->stream, s->spec.side});
  busy.insert(busy.end(), ctx->dev_stream, ctx->dev_stream + BWAGPU_NUM_SLOTS);
  busy.insert(busy.end(), ctx->a2_st, ctx->a2_st + bwagpu_ctx::kA2Streams);
  busy.insert(busy.end(), ctx->ch_cs.side, ctx->ch_cs.side + 2);
  for (hipStream_t x : busy)
    if (x) (void)hipStreamSynchronize(x);
  if (ctx->sdh_done) (void)hipEventSynchronize(ctx->sdh_done);
  if (ctx->r2d_done && ctx->r2d_pending) (void)hipEventSynchronize(ctx->r2d_done);
  // 3. only now, with nothing left running: the handles the context owns outside its slots (the
  //    caller's dev_stream[] are not ours), the reference, and with `delete` every slot and buffer
  std::vector<hipStream_t> own = ctx->side_graveyard;
  own.insert(own.end(), ctx->a2_st, ctx->a2_st + bwagpu_ctx::kA2Streams);
  own.insert(own.end(), ctx->ch_cs.side, ctx->ch_cs.side + 2);
  for (hipStream_t x : own)
    if (x) (void)hipStreamDestroy(x);
  std::vector<hipEvent_t> evs = ctx->prof_ev;
  evs.insert(evs.end(), {ctx->sdh_done, ctx->r2d_done, ctx->r2d_ev[0], ctx->r2d_ev[1], ctx->a2_fork, ctx->ch_cs.fork,
                         ctx->ch_cs.join[0], ctx->ch_cs.join[1]});
  evs.insert(evs.end(), ctx->a2_join, ctx->a2_join + bwagpu_ctx::kA2Streams);
  evs.insert(evs.end(), ctx->rs_ev, ctx->rs_ev + 4 * kRescueMaxRounds);
  for (hipEvent_t e : evs)
    if (e) (void)hipEventDestroy(e);
  if (ctx->own_pac && ctx->d_pac) (void)hipFree(ctx->d_pac);
  if (ctx->d_ann_off) (void)hipFree(ctx->d_ann_off);
  if (ctx->d_ann_len) (void)hipFree(ctx->d_ann_len);
  delete ctx;
}

// BWAGPU_C2A_PATH=fast: the wave-per-read kernels (chain2aln_fast_kernel /
// chain2aln_kernel, DESIGN.md §3 "per-read kernels"); default: the speculative
// path (extension tasks + selection passes)
bool use_read_kernels() {
  const char* e = getenv("BWAGPU_C2A_PATH");
  return e && (strcmp(e, "fast") == 0 || strcmp(e, "read") == 0);
}

// dynamic LDS bytes of variant v's launch for reads up to lq_max
size_t variant_lds(const DevOpt& o, int v, int lq_max) {
  const Variant& vk = kVariants[v];
  const int lqv = std::min(lq_max, vk.max_len());
  const int tb = tb_bytes_for(o, std::max(lqv, 1));
  return vk.kind == VK_FAST ? (size_t)(kBlock / 64) * fast_wave_lds(tb) : (size_t)tb * (kBlock / vk.G);
}

}  // namespace

// Options that need more LDS per workgroup than a launch may take are refused
// BEFORE anything is enqueued (a refusal after the H2D would leave a DMA
// reading the slot's pinned staging buffer while the caller reuses the slot).
int bwagpu::check_lds(bwagpu_ctx_t* ctx, int lq_max) {
  if (!use_read_kernels()) {
    if (spec_redo_cap(tb_bytes_for(ctx->opt, std::max(lq_max, 1))) < 64)
      return fail(ctx, BWAGPU_E_UNSUPPORTED, "LDS row buffer too large for these options (w, pen_clip, read length)");
    return BWAGPU_OK;
  }
  for (int v = 0; v < kNumVariants; ++v) {
    if (variant_lds(ctx->opt, v, lq_max) > 64 * 1024)
      return fail(ctx, BWAGPU_E_UNSUPPORTED, "LDS row buffer too large for these options (w, pen_clip, read length)");
  }
  return BWAGPU_OK;
}

namespace {

// The caller stream st of a spec-path batch: a side stream for its heavy
// selection kernels on a hardware queue that none of this context's caller
// streams and other side streams use (streams_concurrent), or none at all
// (the heavy selection then runs on st) when six candidates all share one.
// A caller stream seen for the first time retires the side streams that share
// its queue (their slots choose again at their next batch).
void register_caller_locked(bwagpu_ctx_t* ctx, hipStream_t st) {
  for (hipStream_t c : ctx->callers)
    if (c == st) return;
  for (Slot* x : all_slots(ctx))
    if (x->side_chosen && x->spec.side && hipStreamSynchronize(x->spec.side) == hipSuccess &&
        !streams_concurrent(x->spec.side, st)) {  // spin on the (drained) side, probe st
      ctx->side_graveyard.push_back(x->spec.side);  // may still hold queued work: destroyed with the context
      x->spec.side = nullptr;
      x->side_chosen = false;
    }
  ctx->callers.push_back(st);
}

// *snap: the slot's streams as of this call, copied under side_mu — a later
// caller stream may retire s.spec.side from another thread (register_caller_locked)
// while this slot's launches are being enqueued; they use the copy (a retired
// side stream stays alive in the graveyard until the context goes)
hipError_t choose_side(bwagpu_ctx_t* ctx, Slot& s, hipStream_t st, SpecStreams* snap) {
  std::lock_guard<std::mutex> g(ctx->side_mu);
  register_caller_locked(ctx, st);
  if (s.side_chosen) {
    *snap = s.spec;
    return hipSuccess;
  }
  if (!s.spec.fork) {
    hipError_t e = hipEventCreateWithFlags(&s.spec.fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.spec.join, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  std::vector<hipStream_t> avoid = ctx->callers;
  for (Slot* x : all_slots(ctx))
    if (x != &s && x->side_chosen && x->spec.side) avoid.push_back(x->spec.side);
  std::vector<hipStream_t> tried;  // kept until the end: each holds its queue's place
  hipStream_t pick = nullptr;
  hipError_t e = hipSuccess;
  for (int t = 0; t < 6 && !pick; ++t) {
    hipStream_t c = nullptr;
    if ((e = hipStreamCreateWithFlags(&c, hipStreamNonBlocking)) != hipSuccess) break;
    bool ok = true;
    for (hipStream_t a : avoid)
      if (!streams_concurrent(c, a)) {  // spin on the candidate, never on a caller stream
        ok = false;
        break;
      }
    if (ok) pick = c;
    else tried.push_back(c);
  }
  for (hipStream_t c : tried) (void)hipStreamDestroy(c);  // only the probe ran on them
  if (e != hipSuccess) return e;
  s.spec.side = pick;
  s.side_chosen = true;
  *snap = s.spec;
  return hipSuccess;
}

int enqueue_spec(bwagpu_ctx_t* ctx, Slot& s, const DevBatch& db, int lq_max, bwagpu_alnreg_t* d_out, int32_t* d_n,
                 int64_t* d_stats, hipStream_t st) {
  const size_t nc = (size_t)std::max(db.n_chains, 1), ns = (size_t)std::max(db.n_seeds, 1),
               nr = (size_t)std::max(db.n_reads, 1);
  const size_t n_tasks = kSpecBins * (nc + (kSpecRounds - 1) * ns);  // every list of every round
  SpecArgs a;
  HIPC(s.d_win.get(a.win, nc), "hipMalloc(win)");
  HIPC(s.d_cread.get(a.chain_read, nc), "hipMalloc(chain_read)");
  HIPC(s.d_prog.get(a.prog, ns), "hipMalloc(prog)");
  HIPC(s.d_ext.get(a.ext, ns), "hipMalloc(ext)");
  HIPC(s.d_tasks.get(a.tasks, n_tasks), "hipMalloc(tasks)");
  HIPC(s.d_ctr.get(a.ctr, SPC_WORDS), "hipMalloc(ctr)");
  HIPC(s.d_regpos.get(a.regpos, ns), "hipMalloc(regpos)");
  HIPC(s.d_skipf.get(a.skipf, ns), "hipMalloc(skipf)");
  HIPC(s.d_heavy.get(a.heavy, nr), "hipMalloc(heavy)");
  HIPC(s.d_redo.get(a.redo, nr), "hipMalloc(redo)");
  HIPC(s.d_rbits.get(a.rbits, 2 * (nr / 32 + 1)), "hipMalloc(rbits)");
  a.fbits = a.rbits + (nr / 32 + 1);  // the finished bits: a second plane
  HIPC(s.d_rlist.get(a.rlist, nr), "hipMalloc(rlist)");
  HIPC(s.d_desc.get(a.rdesc, nr), "hipMalloc(desc)");
  HIPC(s.d_schain.get(a.seedchain, ns), "hipMalloc(seedchain)");
  HIPC(s.d_hinfo.get(a.hinfo, nr), "hipMalloc(hinfo)");
  HIPC(s.d_cov.get(a.cov, ns), "hipMalloc(cov)");
  HIPC(s.d_hflag.get(a.hflag, ns), "hipMalloc(hflag)");
  HIPC(s.d_colent.get(a.colent, ns), "hipMalloc(colent)");
  HIPC(s.d_longc.get(a.longc, nc), "hipMalloc(longc)");
  HIPC(s.d_qh.get(a.qh, kQHWords), "hipMalloc(qh)");
  HIPC(s.d_sorth.get(a.sorth, kSortWords), "hipMalloc(sorth)");
  HIPC(s.d_stasks.get(a.stasks, n_tasks), "hipMalloc(stasks)");
  HIPC(s.d_ftask.get(a.ftask, n_tasks), "hipMalloc(ftask)");
  HIPC(s.d_ftaskR.get(a.ftaskR, n_tasks), "hipMalloc(ftaskR)");
  // the certificate only moves work out of the DP, as the row bound does: it acts under that switch
  a.ung = nullptr;
  if (ctx->ungapped && ctx->opt.row_bound) HIPC(s.d_ung.get(a.ung, n_tasks), "hipMalloc(ung)");
  a.ungt = nullptr;
  if (a.ung && ctx->ungapped_right) HIPC(s.d_ungt.get(a.ungt, n_tasks), "hipMalloc(ungt)");
  // pair matrices of heavy reads: sum over them of 2 * ns * ceil(ns / 64) words,
  // <= 2 * ns_total * (1 + ns_max / 64); reads that do not fit take the per-seed kernel
  HIPC(s.d_mat.get(a.mat, (size_t)std::max<int64_t>(1 << 20, 16 * (int64_t)ns)), "hipMalloc(mat)");
  a.mat_words = (int64_t)(s.d_mat.cap / sizeof(uint64_t));
  static const int ext_prefetch = [] {  // A/B knob of the claim-ahead
    const char* e = getenv("BWAGPU_EXT_PREFETCH");
    return e ? std::max(0, atoi(e)) : 0;
  }();
  a.ext_prefetch = ext_prefetch;
  static const int risky_first = [] {  // A/B knob (neutral, off)
    const char* e = getenv("BWAGPU_LIGHT_RISKY_FIRST");
    return e && e[0] == '1';
  }();
  a.risky_first = risky_first;
  static const int emu_strict = [] {  // A/B knob (0: misses extended inline)
    const char* e = getenv("BWAGPU_EMU_STRICT");
    return !(e && e[0] == '0');
  }();
  a.emu_strict = emu_strict;
  a.light_pack = ctx->light_pack;
  a.emu_finish = ctx->emu_finish;
  a.out = d_out;
  a.out_n = d_n;
  a.stats = d_stats;
  SpecStreams ss;
  HIPC(choose_side(ctx, s, st, &ss), "side stream");
  a.lq_bound = lq_max;
  const int tb = tb_bytes_for(ctx->opt, std::max(lq_max, 1));
  ss.form = ctx->ext_form;
  ss.short_q = ctx->ext_short;
  ss.short_fill = ctx->ext_short_fill;
  ss.fused = ctx->fused_launches;
  ss.pool = ctx->prof_ev.empty() ? nullptr : ctx->prof_ev.data();
  ss.pool_n = (int)ctx->prof_ev.size();
  ss.pool_used = &ctx->prof_used;
  // the batch's zeroed state (counters, queue heads, sort histograms, the
  // round-B bits, SeedExt slots, region counts): one launch, not six memsets
  HIPC(launch_spec_clear(a, db.n_reads, db.n_seeds, st), "spec clear");
  HIPC(launch_spec_chain2aln(ctx->opt, ctx->ref, db, a, tb, lq_max, st, ss), "spec chain2aln launch");
  return BWAGPU_OK;
}

}  // namespace

// enqueue prep + binning + the per-variant kernels for a batch whose arrays
// are already in device memory (check_lds has passed for lq_max)
int bwagpu::enqueue_chain2aln(bwagpu_ctx_t* ctx, Slot& s, const DevBatch& db, int lq_max, bwagpu_alnreg_t* d_out,
                              int32_t* d_n, int64_t* d_stats, hipStream_t st) {
  if (!use_read_kernels()) return enqueue_spec(ctx, s, db, lq_max, d_out, d_n, d_stats, st);
  ChainWin* win = nullptr;
  bwagpu_seed_t* prog = nullptr;
  ReadDesc* desc = nullptr;
  C2AArgs a;
  HIPC(s.d_win.get(win, (size_t)db.n_chains), "hipMalloc(win)");
  HIPC(s.d_srt.get(a.srt, (size_t)db.n_seeds), "hipMalloc(srt)");
  HIPC(s.d_prog.get(prog, (size_t)db.n_seeds), "hipMalloc(prog)");
  const size_t nr = (size_t)std::max(db.n_reads, 1);
  HIPC(s.d_desc.get(desc, nr), "hipMalloc(desc)");
  // bins | read_list, n_reads each
  HIPC(s.d_lists.ensure(2 * sizeof(int32_t) * nr), "hipMalloc(lists)");
  int32_t* bins = s.d_lists.as<int32_t>();
  int32_t* read_list = bins + nr;
  HIPC(s.d_counts.get(a.counts, kCountWords), "hipMalloc(counts)");
  HIPC(hipMemsetAsync(a.counts, 0, sizeof(int32_t) * kCountWords, st), "memset counts");
  if (db.n_reads) HIPC(hipMemsetAsync(d_n, 0, sizeof(int32_t) * db.n_reads, st), "memset out_n");
  HIPC(launch_chain_prep(ctx->opt, ctx->ref, db, win, a.srt, prog, d_stats, st), "chain_prep launch");
  HIPC(launch_read_order(db, bins, a.counts + kHistOff, a.counts, desc, read_list, d_stats, st), "read order launch");
  a.read_list = read_list;
  a.desc = desc;
  a.win = win;
  a.prog = prog;
  a.out = d_out;
  a.out_n = d_n;
  a.stats = d_stats;
  for (int v = 0; v < kNumVariants; ++v) {
    const int lqv = std::min(lq_max, kVariants[v].max_len());
    const int tb = tb_bytes_for(ctx->opt, std::max(lqv, 1));
    HIPC(launch_chain2aln(v, ctx->opt, ctx->ref, db, db.n_reads, tb, a, st), "chain2aln launch");
  }
  return BWAGPU_OK;
}

extern "C" {

int bwagpu_abi_version(void) { return BWAGPU_ABI_VERSION; }

int bwagpu_device_count(int* n) {
  if (!n) return BWAGPU_E_INVAL;
  int k = 0;
  if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
  *n = k;
  return k > 0 ? BWAGPU_OK : BWAGPU_E_NODEVICE;
}

int bwagpu_create(int device, const bwagpu_opt_t* opt, const bwagpu_bns_t* bns, const uint8_t* pac_host,
                  bwagpu_ctx_t** out) {
  if (!pac_host) return BWAGPU_E_INVAL;
  bwagpu_ctx_t* ctx = nullptr;
  int rc = create_common(device, opt, bns, out, &ctx);
  if (rc == BWAGPU_OK) {
    const size_t pac_bytes = (size_t)(bns->l_pac / 4 + 1);  // bwa.c:281-282
    hipError_t e = hipMalloc(&ctx->d_pac, pac_bytes);
    if (e == hipSuccess) {
      ctx->own_pac = true;
      e = hipMemcpy(ctx->d_pac, pac_host, pac_bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) rc = hip_fail(ctx, e, "pac upload");
    ctx->ref.pac = (const uint8_t*)ctx->d_pac;
  }
  if (rc != BWAGPU_OK) {
    destroy_ctx(ctx);
    return rc;
  }
  *out = ctx;
  return BWAGPU_OK;
}

int bwagpu_create_resident(int device, const bwagpu_opt_t* opt, const bwagpu_bns_t* bns, const void* pac_device,
                           bwagpu_ctx_t** out) {
  if (!pac_device) return BWAGPU_E_INVAL;
  bwagpu_ctx_t* ctx = nullptr;
  int rc = create_common(device, opt, bns, out, &ctx);
  if (rc != BWAGPU_OK) {
    destroy_ctx(ctx);
    return rc;
  }
  ctx->d_pac = (void*)pac_device;
  ctx->own_pac = false;
  ctx->ref.pac = (const uint8_t*)pac_device;
  *out = ctx;
  return BWAGPU_OK;
}

int bwagpu_destroy(bwagpu_ctx_t* ctx) {
  if (!ctx) return BWAGPU_E_INVAL;
  destroy_ctx(ctx);
  return BWAGPU_OK;
}

const char* bwagpu_last_error(const bwagpu_ctx_t* ctx) { return ctx ? ctx->err.c_str() : "NULL context"; }

int bwagpu_set_watchdog_ms(bwagpu_ctx_t* ctx, int ms) {
  if (!ctx || ms < 0) return BWAGPU_E_INVAL;
  ctx->watchdog_ms = ms;
  return BWAGPU_OK;
}

namespace {
// the ABI's slot layout (read r's regions from chain_seed_off[read_chain_off[r]])
// from a finished batch's dense results; the offsets come from the staged input
void expand_slots(const Slot& s, bwagpu_alnreg_t* dst) {
  const char* h = s.h_in.as<const char>();
  const int32_t* rco = s.kept ? s.keep_rco.data() : (const int32_t*)(h + s.in_rco);
  const int32_t* cso = s.kept ? s.keep_cso.data() : (const int32_t*)(h + s.in_cso);
  const int32_t* n = s.h_n.as<const int32_t>();
  const int32_t* off = s.h_off.as<const int32_t>();
  const bwagpu_alnreg_t* src = s.h_dense.as<const bwagpu_alnreg_t>();
  for (int32_t r = 0; r < s.n_reads; ++r)
    if (n[r]) memcpy(dst + cso[rco[r]], src + off[r], sizeof(bwagpu_alnreg_t) * (size_t)n[r]);
}
}  // namespace

int bwagpu_chain2aln_submit(bwagpu_ctx_t* ctx, int slot, const bwagpu_batch_t* b) {
  if (!ctx || slot < 0 || slot >= BWAGPU_NUM_SLOTS) return BWAGPU_E_INVAL;
  Slot& s = ctx->slot[slot];
  if (s.busy) return fail(ctx, BWAGPU_E_INVAL, "slot already has a batch in flight");
  // the previous batch's results end here, whether or not this submit succeeds
  s.has_results = false;
  s.kept = false;
  s.slot_view = false;
  int lq_max = 0;
  std::string why;
  int rc = check_batch_header(b, &why);
  if (rc) return fail(ctx, rc, why);
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  s.t_submit = std::chrono::steady_clock::now();
  InLayout L;
  L.make(*b);
  HIPC(s.h_in.ensure(L.total), "hipHostMalloc(in)");
  HIPC(s.d_in.ensure(L.total), "hipMalloc(in)");
  bwagpu_alnreg_t *d_out = nullptr, *h_dense = nullptr;
  int32_t *d_n = nullptr, *h_n = nullptr, *h_off = nullptr, *d_off = nullptr;
  int64_t *d_stats = nullptr, *h_stats = nullptr;
  HIPC(s.d_out.get(d_out, (size_t)b->n_seeds), "hipMalloc(out)");
  HIPC(s.d_n.get(d_n, (size_t)b->n_reads), "hipMalloc(out_n)");
  HIPC(s.d_stats.get(d_stats, ST_N), "hipMalloc(stats)");
  HIPC(s.h_dense.get(h_dense, (size_t)b->n_seeds), "hipHostMalloc(out)");
  HIPC(s.h_n.get(h_n, (size_t)b->n_reads), "hipHostMalloc(out_n)");
  HIPC(s.h_off.get(h_off, (size_t)b->n_reads + 1), "hipHostMalloc(out_off)");
  HIPC(s.d_off.get(d_off, (size_t)b->n_reads + 1), "hipMalloc(out_off)");
  HIPC(s.h_stats.get(h_stats, ST_N), "hipHostMalloc(stats)");
  s.slot_view = false;
  // stage into pinned memory so the caller's buffers are free on return —
  // unless the caller packed into that memory already (bwagpu_chain2aln_stage)
  char* h = s.h_in.as<char>();
  const bool staged = b->n_reads > 0 && (const void*)b->seq_off == (const void*)(h + L.seq_off) &&
                      (const void*)b->seeds == (const void*)(h + L.seeds) &&
                      (const void*)b->seq == (const void*)(h + L.seq) &&
                      (const void*)b->chain_seed_off == (const void*)(h + L.cso);
  // the staging copy (~20 MB for a C2 record) and the check of every read,
  // chain and seed in one pass on a few threads (stage_and_check): nothing is
  // enqueued before both are done, so a refused batch leaves no DMA reading
  // the staging buffer
  if (!staged && b->n_reads) {
    rc = stage_and_check(b, ctx->ref.l_pac, h, L, &lq_max, &why);
  } else {
    if (!staged) memcpy(h + L.cso, b->chain_seed_off, sizeof(int32_t) * (size_t)(b->n_chains + 1));
    rc = check_batch_seeds(b, ctx->ref.l_pac, &lq_max, &why);
  }
  if (rc) return fail(ctx, rc, why);
  if ((rc = check_lds(ctx, lq_max))) return rc;

  hipStream_t st = nullptr;
  HIPC(lazy_stream(s, &st), "hipStreamCreate");
  HIPC(hipEventRecord(s.ev0, st), "event");
  HIPC(hipMemcpyAsync(s.d_in.p, s.h_in.p, L.total, hipMemcpyHostToDevice, st), "H2D batch");
  HIPC(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * ST_N, st), "memset stats");
  char* d = s.d_in.as<char>();
  DevBatch db;
  db.n_reads = b->n_reads;
  db.n_chains = b->n_chains;
  db.n_seeds = b->n_seeds;
  db.seq_off = (const int64_t*)(d + L.seq_off);
  db.seq = (const uint8_t*)(d + L.seq);
  db.read_chain_off = (const int32_t*)(d + L.rco);
  db.chain_seed_off = (const int32_t*)(d + L.cso);
  db.chain_rid = (const int32_t*)(d + L.rid);
  db.chain_frac_rep = (const float*)(d + L.frac);
  db.seeds = (const bwagpu_seed_t*)(d + L.seeds);
  HIPC(hipEventRecord(s.ev1, st), "event");
  rc = enqueue_chain2aln(ctx, s, db, lq_max, d_out, d_n, d_stats, st);
  if (rc) {
    // work already queued on the slot's stream may still read h_in / d_in:
    // drain it before the caller may reuse the slot
    (void)hipStreamSynchronize(st);
    return rc;
  }
  if (ctx->post_flags && b->n_reads) {  // bwagpu_set_regs_post: in place on the slot layout, before the dense copy
    rc = enqueue_regpost(ctx, ctx->post_opt, ctx->post_flags, ctx->post_id0, b->n_reads, db.seq_off, db.seq, nullptr,
                         db.read_chain_off, db.chain_seed_off, d_out, d_n, d_stats, st);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    ctx->post_id0 += b->n_reads;
  }
  HIPC(hipEventRecord(s.ev2, st), "event");
  // the results: per-read offsets, then the regions densely into pinned memory
  // (the device writes them over PCIe: only the sum of n is moved, not the
  // n_seeds slots the kernels fill)
  int32_t* h_off_dev = nullptr;
  bwagpu_alnreg_t* h_dense_dev = nullptr;
  HIPC(hipHostGetDevicePointer((void**)&h_off_dev, h_off, 0), "hipHostGetDevicePointer");
  HIPC(hipHostGetDevicePointer((void**)&h_dense_dev, h_dense, 0), "hipHostGetDevicePointer");
  hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(kDenseScanBlock), 0, st, d_n, b->n_reads, d_off, h_off_dev);
  if (b->n_reads)
    hipLaunchKernelGGL(dense_copy_kernel, dim3((unsigned)((b->n_reads + 15) / 16)), dim3(256), 0, st, d_out, d_n,
                       d_off, db.read_chain_off, db.chain_seed_off, b->n_reads, h_dense_dev);
  HIPC(hipGetLastError(), "dense results launch");
  if (b->n_reads)
    HIPC(hipMemcpyAsync(h_n, d_n, sizeof(int32_t) * (size_t)b->n_reads, hipMemcpyDeviceToHost, st), "D2H counts");
  HIPC(hipMemcpyAsync(h_stats, d_stats, sizeof(int64_t) * ST_N, hipMemcpyDeviceToHost, st), "D2H stats");
  HIPC(hipEventRecord(s.ev3, st), "event");
  s.h2d = (int64_t)L.total;
  s.in_rco = L.rco;
  s.in_cso = L.cso;
  // the batch's sizes only once it is in flight: _wait and _results read them
  s.n_reads = b->n_reads;
  s.n_chains = b->n_chains;
  s.n_seeds = b->n_seeds;
  s.busy = true;
  return BWAGPU_OK;
}

int bwagpu_chain2aln_wait(bwagpu_ctx_t* ctx, int slot, bwagpu_alnreg_t* out_regs, int32_t* out_n) {
  if (!ctx || slot < 0 || slot >= BWAGPU_NUM_SLOTS) return BWAGPU_E_INVAL;
  Slot& s = ctx->slot[slot];
  if (!s.busy) return fail(ctx, BWAGPU_E_INVAL, "slot has no batch in flight");
  if (ctx->fail_after == 0) {  // injected failure: the batch stays in flight, as after a real watchdog expiry
    ctx->fail_after = -1;
    return fail(ctx, ctx->fail_code, "injected failure (bwagpu_debug_fail_wait)");
  }
  if (ctx->fail_after > 0) --ctx->fail_after;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  // watchdog (SWTask::finish, SWTask.cpp:162-169): poll the completion event,
  // backing off from 20 to 320 us (every query takes the runtime's lock, which
  // other host threads driving the device contend for)
  const auto t0 = std::chrono::steady_clock::now();
  int nap_us = 20;
  for (;;) {
    hipError_t q = hipEventQuery(s.ev3);
    if (q == hipSuccess) break;
    if (q != hipErrorNotReady) {
      s.busy = false;
      return hip_fail(ctx, q, "batch execution");
    }
    if (ctx->watchdog_ms > 0 &&
        std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() >
            ctx->watchdog_ms) {
      return fail(ctx, BWAGPU_E_HANG, "watchdog: batch did not finish in time");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(nap_us));
    nap_us = std::min(nap_us * 2, 320);
  }
  s.busy = false;
  s.has_results = true;
  const int64_t* st = s.h_stats.as<int64_t>();
  float k_ms = 0, t_ms = 0;
  (void)hipEventElapsedTime(&k_ms, s.ev1, s.ev2);
  (void)hipEventElapsedTime(&t_ms, s.ev0, s.ev3);
  s.last.kernel_ms = k_ms;
  s.last.total_ms = t_ms;
  s.last.cells = st[ST_CELLS];
  s.last.rows = st[ST_ROWS];
  s.last.ext_calls = st[ST_CALLS];
  const int32_t* off = s.h_off.as<int32_t>();
  s.d2h = (int64_t)sizeof(bwagpu_alnreg_t) * off[s.n_reads] + (int64_t)sizeof(int32_t) * (2 * (int64_t)s.n_reads + 1);
  s.last.h2d_bytes = s.h2d;
  s.last.d2h_bytes = s.d2h;
  if (st[ST_ERR] & ERR_LEN) return fail(ctx, BWAGPU_E_UNSUPPORTED, "read longer than BWAGPU_MAX_READ_LEN");
  // on a flagged chain the results are still copied: every other chain's
  // regions are valid, the flagged ones were skipped (the caller's error path)
  if (out_n && s.n_reads) memcpy(out_n, s.h_n.p, sizeof(int32_t) * (size_t)s.n_reads);
  if (out_regs && s.n_seeds) expand_slots(s, out_regs);
  if (st[ST_ERR] & ERR_POST) return fail(ctx, BWAGPU_E_UNSUPPORTED, "a patch candidate's window exceeds 4096 bases");
  if (st[ST_ERR] & ERR_RID)
    return fail(ctx, BWAGPU_E_RESULTS, "a chain's first seed is not inside contig chain_rid (bwamem.c:669 assert)");
  return BWAGPU_OK;
}

int bwagpu_chain2aln_stage(bwagpu_ctx_t* ctx, int slot, int32_t n_reads, int32_t n_chains, int32_t n_seeds,
                           int64_t seq_bytes, bwagpu_batch_t* view) {
  if (!ctx || slot < 0 || slot >= BWAGPU_NUM_SLOTS || !view || n_reads < 0 || n_chains < 0 || n_seeds < 0 ||
      seq_bytes < 0)
    return BWAGPU_E_INVAL;
  Slot& s = ctx->slot[slot];
  if (s.busy) return fail(ctx, BWAGPU_E_INVAL, "slot already has a batch in flight");
  bwagpu_batch_t b{};
  b.n_reads = n_reads;
  b.n_chains = n_chains;
  b.n_seeds = n_seeds;
  b.seq_bytes = seq_bytes;
  InLayout L;
  L.make(b);
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  // the caller packs the next batch over h_in: the finished batch's offsets
  // move out first, so that its _results (valid until the next _submit) can
  // still build the slot layout
  if (s.has_results && !s.slot_view && !s.kept && s.n_reads) {
    const char* hp = s.h_in.as<const char>();
    const int32_t* rco = (const int32_t*)(hp + s.in_rco);
    s.keep_rco.assign(rco, rco + s.n_reads + 1);
    const int32_t* cso = (const int32_t*)(hp + s.in_cso);
    s.keep_cso.assign(cso, cso + s.n_chains + 1);
    s.kept = true;
  }
  HIPC(s.h_in.ensure(L.total), "hipHostMalloc(in)");
  char* h = s.h_in.as<char>();
  b.seq_off = (const int64_t*)(h + L.seq_off);
  b.seq = (const uint8_t*)(h + L.seq);
  b.read_chain_off = (const int32_t*)(h + L.rco);
  b.chain_seed_off = (const int32_t*)(h + L.cso);
  b.chain_rid = (const int32_t*)(h + L.rid);
  b.chain_frac_rep = (const float*)(h + L.frac);
  b.seeds = (const bwagpu_seed_t*)(h + L.seeds);
  *view = b;
  return BWAGPU_OK;
}

int bwagpu_chain2aln_results(bwagpu_ctx_t* ctx, int slot, const bwagpu_alnreg_t** regs, const int32_t** n) {
  if (!ctx || slot < 0 || slot >= BWAGPU_NUM_SLOTS || !regs || !n) return BWAGPU_E_INVAL;
  Slot& s = ctx->slot[slot];
  if (s.busy) return fail(ctx, BWAGPU_E_INVAL, "slot's batch still in flight (wait first)");
  if (!s.has_results) return fail(ctx, BWAGPU_E_INVAL, "slot has no results");
  if (!s.slot_view) {  // the slot layout, built from the dense results once per batch
    bwagpu_alnreg_t* h_out = nullptr;
    HIPC(s.h_out.get(h_out, (size_t)s.n_seeds), "hipHostMalloc(out)");
    if (s.n_seeds) expand_slots(s, h_out);
    s.slot_view = true;
  }
  *regs = s.h_out.as<const bwagpu_alnreg_t>();
  *n = s.h_n.as<const int32_t>();
  return BWAGPU_OK;
}

int bwagpu_chain2aln_results_dense(bwagpu_ctx_t* ctx, int slot, const bwagpu_alnreg_t** regs, const int32_t** n,
                                   const int32_t** off) {
  if (!ctx || slot < 0 || slot >= BWAGPU_NUM_SLOTS || !regs || !n || !off) return BWAGPU_E_INVAL;
  Slot& s = ctx->slot[slot];
  if (s.busy) return fail(ctx, BWAGPU_E_INVAL, "slot's batch still in flight (wait first)");
  if (!s.has_results || !s.h_dense.p || !s.h_off.p) return fail(ctx, BWAGPU_E_INVAL, "slot has no results");
  *regs = s.h_dense.as<const bwagpu_alnreg_t>();
  *n = s.h_n.as<const int32_t>();
  *off = s.h_off.as<const int32_t>();
  return BWAGPU_OK;
}

int bwagpu_chain2aln(bwagpu_ctx_t* ctx, const bwagpu_batch_t* b, bwagpu_alnreg_t* out_regs, int32_t* out_n) {
  int rc = bwagpu_chain2aln_submit(ctx, 0, b);
  if (rc) return rc;
  return bwagpu_chain2aln_wait(ctx, 0, out_regs, out_n);
}

int bwagpu_chain2aln_device(bwagpu_ctx_t* ctx, const bwagpu_batch_t* db_in, bwagpu_alnreg_t* dev_out,
                            int32_t* dev_n, int64_t* dev_stats, void* stream) {
  if (!ctx || !db_in || !dev_out || !dev_n) return BWAGPU_E_INVAL;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  // reads are bounded by bwagpu_set_device_read_len (default BWAGPU_MAX_READ_LEN)
  // on the speculative path, by BWAGPU_MAX_READ_LEN on the per-read one; the
  // LDS row buffers are sized for the bound
  const int lq_bound = use_read_kernels() ? BWAGPU_MAX_READ_LEN : ctx->dev_read_len;
  int rc = check_lds(ctx, lq_bound);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!st) HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  int k = 0;
  while (k < BWAGPU_NUM_SLOTS && ctx->dev_stream[k] && ctx->dev_stream[k] != st) ++k;
  if (k == BWAGPU_NUM_SLOTS) return fail(ctx, BWAGPU_E_INVAL, "more than BWAGPU_NUM_SLOTS streams on one context");
  ctx->dev_stream[k] = st;
  Slot& s = ctx->dev_scratch[k];
  DevBatch db;
  db.n_reads = db_in->n_reads;
  db.n_chains = db_in->n_chains;
  db.n_seeds = db_in->n_seeds;
  db.seq_off = db_in->seq_off;
  db.seq = db_in->seq;
  db.read_chain_off = db_in->read_chain_off;
  db.chain_seed_off = db_in->chain_seed_off;
  db.chain_rid = db_in->chain_rid;
  db.chain_frac_rep = db_in->chain_frac_rep;
  db.seeds = db_in->seeds;
  int64_t* stats = dev_stats;
  if (!stats) {
    HIPC(s.d_stats.get(stats, ST_N), "hipMalloc(stats)");
    HIPC(hipMemsetAsync(stats, 0, sizeof(int64_t) * ST_N, st), "memset stats");
  }
  return enqueue_chain2aln(ctx, s, db, lq_bound, dev_out, dev_n, stats, st);
}

int bwagpu_set_device_read_len(bwagpu_ctx_t* ctx, int32_t max_len) {
  if (!ctx || max_len < 1 || max_len > BWAGPU_MAX_READ_LEN) return BWAGPU_E_INVAL;
  ctx->dev_read_len = max_len;
  return BWAGPU_OK;
}

int bwagpu_debug_set_trace(bwagpu_ctx_t* ctx, void* dev_ptr) {
  if (!ctx) return BWAGPU_E_INVAL;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  HIPC(set_trace(dev_ptr), "set trace");
  HIPC(set_trace_spec(dev_ptr), "set trace");
  return BWAGPU_OK;
}

int bwagpu_debug_fail_wait(bwagpu_ctx_t* ctx, int after_n_waits, int code) {
  if (!ctx || code <= 0) return BWAGPU_E_INVAL;
  ctx->fail_after = after_n_waits;
  ctx->fail_code = code;
  return BWAGPU_OK;
}

int bwagpu_debug_live_buffers(int64_t* n, int64_t* bytes) {
  if (!n || !bytes) return BWAGPU_E_INVAL;
  *n = g_live_bufs.load(std::memory_order_relaxed);
  *bytes = g_live_bytes.load(std::memory_order_relaxed);
  return BWAGPU_OK;
}

// the SPC_* counter words of the last device-entry batch on `stream` (waits for it): what the
// bwagpu_debug_spec_* readers share
static int spec_ctr_words(bwagpu_ctx_t* ctx, void* stream, int32_t* c) {
  hipStream_t st = nullptr;
  if (int rc = entry_stream(ctx, stream, &st)) return rc;
  int k = 0;
  while (k < BWAGPU_NUM_SLOTS && ctx->dev_stream[k] != st) ++k;
  if (k == BWAGPU_NUM_SLOTS || !ctx->dev_scratch[k].d_ctr.p) return fail(ctx, BWAGPU_E_INVAL, "no device-entry batch on this stream");
  HIPC(hipStreamSynchronize(st), "hipStreamSynchronize");
  HIPC(hipMemcpy(c, ctx->dev_scratch[k].d_ctr.p, sizeof(int32_t) * SPC_WORDS, hipMemcpyDeviceToHost), "hipMemcpy(ctr)");
  return BWAGPU_OK;
}

int bwagpu_debug_occupancy(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  memcpy(out, c + 32, 14 * sizeof(int64_t));
#ifdef BWAGPU_OCC_DIAG
  return BWAGPU_OK;
#else
  return fail(ctx, BWAGPU_E_UNSUPPORTED, "built without BWAGPU_OCC_DIAG");
#endif
}

int bwagpu_debug_spec_counters(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  for (int r = 0; r < kSpecRounds; ++r) {
    out[r] = 0;
    for (int b = 0; b < kSpecBins; ++b) out[r] += c[SPC_CNT + r * kSpecBins + b];
  }
  int64_t spec = 0;
  memcpy(&spec, c + SPC_SPEC64, 8);
  out[3] = spec;
  out[4] = c[SPC_MISS];
  out[5] = c[SPC_HEAVY_N];
  out[6] = c[SPC_REDO_N];
  out[7] = c[SPC_HCOLS];
  return BWAGPU_OK;
}

int bwagpu_debug_spec_ext(bwagpu_ctx_t* ctx, void* stream, void* host_out, int32_t n) {
  if (!ctx || !host_out || n < 0) return BWAGPU_E_INVAL;
  hipStream_t st = nullptr;
  if (int rc = entry_stream(ctx, stream, &st)) return rc;
  int k = 0;
  while (k < BWAGPU_NUM_SLOTS && ctx->dev_stream[k] != st) ++k;
  if (k == BWAGPU_NUM_SLOTS || !ctx->dev_scratch[k].d_ext.p || ctx->dev_scratch[k].d_ext.cap < sizeof(SeedExt) * (size_t)n)
    return fail(ctx, BWAGPU_E_INVAL, "no device-entry batch of that size on this stream");
  HIPC(hipStreamSynchronize(st), "hipStreamSynchronize");
  HIPC(hipMemcpy(host_out, ctx->dev_scratch[k].d_ext.p, sizeof(SeedExt) * (size_t)n, hipMemcpyDeviceToHost),
       "hipMemcpy(ext)");
  return BWAGPU_OK;
}

int bwagpu_debug_ext_form(int form) { return set_ext_form(form); }

int bwagpu_streams_concurrent(void* a, void* b) {
  if (!a || !b || a == b) return BWAGPU_E_INVAL;
  return streams_concurrent((hipStream_t)a, (hipStream_t)b) ? 1 : 0;
}

int bwagpu_ctx_ext_form(bwagpu_ctx_t* ctx, int form) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->ext_form;
  if (form >= 0) ctx->ext_form = form > 2 ? 1 : form;
  return prev;
}

int bwagpu_ctx_ext_short(bwagpu_ctx_t* ctx, int q) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->ext_short;
  if (q >= 0) ctx->ext_short = q > 63 ? 63 : q;
  return prev;
}

int bwagpu_ctx_ext_short_fill(bwagpu_ctx_t* ctx, int percent) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->ext_short_fill;
  if (percent >= 0) ctx->ext_short_fill = percent > 100000 ? 100000 : percent;
  return prev;
}

int bwagpu_ctx_light_pack(bwagpu_ctx_t* ctx, int on) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->light_pack;
  if (on >= 0) ctx->light_pack = on != 0;
  return prev;
}

int bwagpu_debug_spec_short(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  out[0] = c[SPC_SHORT_N];
  for (int r = 0; r < 2; ++r) {  // rounds A and B, the first length bin's lists
    const int l = r * kSpecBins;
    out[1 + 4 * r] = c[SPC_LCNT + l];
    out[2 + 4 * r] = c[SPC_LLONG + l];
    out[3 + 4 * r] = c[SPC_RCNT + l];
    out[4 + 4 * r] = c[SPC_RLONG + l];
  }
  return BWAGPU_OK;
}

int bwagpu_ctx_ungapped(bwagpu_ctx_t* ctx, int on) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->ungapped;
  if (on >= 0) ctx->ungapped = on ? 1 : 0;
  return prev;
}

int bwagpu_debug_spec_ungapped(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  for (int r = 0; r < kSpecRounds; ++r) {
    out[4 * r + 0] = c[SPC_UNG_N + r];
    out[4 * r + 1] = c[SPC_UNG_Q + r];
    out[4 * r + 2] = out[4 * r + 3] = 0;
    for (int bin = 0; bin < kSpecBins; ++bin) {  // the sides left on the lists (0 for a bin that is not phased)
      out[4 * r + 2] += c[SPC_LCNT + r * kSpecBins + bin];
      out[4 * r + 3] += c[SPC_RCNT + r * kSpecBins + bin];
    }
  }
  return BWAGPU_OK;
}

int bwagpu_ctx_ungapped_right(bwagpu_ctx_t* ctx, int on) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->ungapped_right;
  if (on >= 0) ctx->ungapped_right = on ? 1 : 0;
  return prev;
}

int bwagpu_debug_spec_ungapped_right(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  for (int r = 0; r < kSpecRounds; ++r) {
    out[2 * r + 0] = c[SPC_UNGR_N + r];
    out[2 * r + 1] = c[SPC_UNGR_Q + r];
  }
  return BWAGPU_OK;
}

int bwagpu_ctx_emu_finish(bwagpu_ctx_t* ctx, int on) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->emu_finish;
  if (on >= 0) ctx->emu_finish = on ? 1 : 0;
  return prev;
}

int bwagpu_ctx_fused_launches(bwagpu_ctx_t* ctx, int mask) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->fused_launches;
  if (mask >= 0) ctx->fused_launches = mask & 7;
  return prev;
}

int bwagpu_debug_spec_finish(bwagpu_ctx_t* ctx, void* stream, int64_t* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  int32_t c[SPC_WORDS];
  if (int rc = spec_ctr_words(ctx, stream, c)) return rc;
  out[0] = c[SPC_FIN_NAR];
  out[1] = c[SPC_FIN_WIDE];
  out[2] = c[SPC_LIST_N];
  out[3] = c[SPC_LIGHT_N];
  return BWAGPU_OK;
}

int bwagpu_ctx_row_bound(bwagpu_ctx_t* ctx, int on) {
  if (!ctx) return BWAGPU_E_INVAL;
  const int prev = ctx->opt.row_bound;
  if (on >= 0) ctx->opt.row_bound = on ? 1 : 0;
  return prev;
}

int bwagpu_debug_ext_kernel(bwagpu_ctx_t* ctx, int32_t lq_max) {
  if (!ctx || lq_max < 1 || lq_max > BWAGPU_MAX_READ_LEN) return BWAGPU_E_INVAL;
  return ext_kernel_for(ctx->opt, ctx->ext_form, tb_bytes_for(ctx->opt, lq_max));
}

int bwagpu_prof_start(bwagpu_ctx_t* ctx, int max_launches) {
  if (!ctx || max_launches < 0) return BWAGPU_E_INVAL;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  for (hipEvent_t e : ctx->prof_ev) HIPC(hipEventSynchronize(e), "hipEventSynchronize");
  for (hipEvent_t e : ctx->prof_ev) (void)hipEventDestroy(e);
  ctx->prof_ev.clear();
  ctx->prof_used = 0;
  for (int i = 0; i < 2 * max_launches; ++i) {
    hipEvent_t e = nullptr;
    HIPC(hipEventCreate(&e), "hipEventCreate");
    ctx->prof_ev.push_back(e);
  }
  return BWAGPU_OK;
}

int bwagpu_prof_read(bwagpu_ctx_t* ctx, double* total_ms, int32_t* launches) {
  if (!ctx || !total_ms || !launches) return BWAGPU_E_INVAL;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  double t = 0;
  for (int i = 0; i + 1 < ctx->prof_used; i += 2) {
    HIPC(hipEventSynchronize(ctx->prof_ev[i + 1]), "hipEventSynchronize");
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, ctx->prof_ev[i], ctx->prof_ev[i + 1]), "hipEventElapsedTime");
    t += ms;
  }
  *total_ms = t;
  *launches = ctx->prof_used / 2;
  return BWAGPU_OK;
}

int bwagpu_prof_intervals(bwagpu_ctx_t* ctx, double* start_ms, double* end_ms, int32_t max, int32_t* n) {
  if (!ctx || !n || max < 0 || (max && (!start_ms || !end_ms))) return BWAGPU_E_INVAL;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  int k = 0;
  for (int i = 0; i + 1 < ctx->prof_used && k < max; i += 2, ++k) {
    HIPC(hipEventSynchronize(ctx->prof_ev[i + 1]), "hipEventSynchronize");
    float a = 0, b = 0;
    HIPC(hipEventElapsedTime(&a, ctx->prof_ev[0], ctx->prof_ev[i]), "hipEventElapsedTime");
    HIPC(hipEventElapsedTime(&b, ctx->prof_ev[0], ctx->prof_ev[i + 1]), "hipEventElapsedTime");
    start_ms[k] = a;
    end_ms[k] = b;
  }
  *n = k;
  return BWAGPU_OK;
}

int bwagpu_last_stats(const bwagpu_ctx_t* ctx, int slot, bwagpu_stats_t* out) {
  if (!ctx || !out || slot < 0 || slot >= BWAGPU_NUM_SLOTS) return BWAGPU_E_INVAL;
  *out = ctx->slot[slot].last;
  return BWAGPU_OK;
}

}  // extern "C"
