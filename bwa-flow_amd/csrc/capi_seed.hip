// capi_seed.hip — the seeding and chaining entries of the C ABI: the FM-index
// upload (bwagpu_set_bwt, bwagpu_bwt_sa, bwagpu_set_alt), mem_collect_intv
// (bwagpu_collect_intv) and SeqsToChains / SeqsToRegions on the device
// (bwagpu_seqs2chains, bwagpu_seqs2regions).  Their checks of the caller's
// arrays, the staging copy and the host's tables are plain C++ in seed_host.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "chain.h"
#include "ctx.h"
#include "engine.h"
#include "regpost.h"
#include "seed.h"
#include "seed_host.h"

using namespace bwagpu;

// ------------------------------------------------------------------ seeding
extern "C" int bwagpu_set_bwt(bwagpu_ctx_t* ctx, const bwagpu_bwt_t* bwt) {
  if (!ctx || !bwt || !bwt->bwt || bwt->bwt_size == 0) return BWAGPU_E_INVAL;
  const char* why = "";
  if (int rc = bwt_header_check(bwt, &why)) return fail(ctx, rc, why);
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  HIPC(ctx->bwt_words.ensure(sizeof(uint32_t) * bwt->bwt_size + 64), "hipMalloc");
  HIPC(hipMemcpy(ctx->bwt_words.p, bwt->bwt, sizeof(uint32_t) * bwt->bwt_size, hipMemcpyHostToDevice), "H2D");
  ctx->bwt.primary = bwt->primary;
  for (int i = 0; i < 5; ++i) ctx->bwt.L2[i] = bwt->L2[i];
  ctx->bwt.seq_len = bwt->seq_len;
  ctx->bwt.bwt = ctx->bwt_words.as<uint32_t>();
  {  // the device occurrence layout (seed.hip: 64-position blocks)
    uint4* occ = nullptr;
    uint64_t* sup = nullptr;
    HIPC(ctx->occ_d.get(occ, 2 * (size_t)occ64_blocks(bwt->seq_len)), "hipMalloc");
    ctx->bwt.sup_shift = ctx->sup_shift;
    HIPC(ctx->sup_d.get(sup, 4 * (size_t)occ64_supers(bwt->seq_len, ctx->sup_shift)), "hipMalloc");
    HIPC(hipMemset(occ, 0, 2 * sizeof(uint4) * (size_t)occ64_blocks(bwt->seq_len)), "memset");
    hipStream_t st = nullptr;
    HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
    HIPC(launch_build_occ64(ctx->bwt, occ, sup, st), "build_occ64 launch");
    HIPC(hipStreamSynchronize(st), "sync");
    ctx->bwt.occ = occ;
    ctx->bwt.sup = sup;
  }
  ctx->bwt.sa = nullptr;
  ctx->bwt.sa_mask = 0;
  ctx->bwt.sa_shift = 0;
  ctx->bwt.sa_full32 = nullptr;
  ctx->bwt.sa_full64 = nullptr;
  if (bwt->sa) {
    if (int rc = bwt_sa_check(bwt, &why)) return fail(ctx, rc, why);
    const int iv = bwt->sa_intv;
    uint64_t* sa = nullptr;
    HIPC(ctx->sa_d.get(sa, bwt->n_sa), "hipMalloc");
    HIPC(hipMemcpy(sa, bwt->sa, sizeof(uint64_t) * bwt->n_sa, hipMemcpyHostToDevice), "H2D");
    ctx->bwt.sa = sa;
    ctx->bwt.sa_mask = (uint64_t)iv - 1;
    while ((1 << ctx->bwt.sa_shift) < iv) ++ctx->bwt.sa_shift;
    // every row's entry in HBM (one load per bwt_sa instead of a walk of ~sa_intv
    // dependent occurrence lookups): 32-bit entries below 2^32 rows (chr21: 0.37
    // GB), 64-bit above (GRCh38: 50 GB of the 288), within 64 GB and a quarter
    // of the free memory; BWAGPU_SA_FULL=0 keeps the sampled walk, =64 forces
    // 64-bit entries (tests)
    const char* fe = getenv("BWAGPU_SA_FULL");
    const bool narrow = bwt->seq_len < 0xffffffffull && !(fe && strcmp(fe, "64") == 0);
    const uint64_t bytes = (bwt->seq_len + 1) * (narrow ? 4 : 8);
    size_t free_b = 0, total_b = 0;
    if (!(fe && strcmp(fe, "0") == 0) && iv > 1 && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
        bytes <= ((uint64_t)64 << 30) && bytes <= free_b / 4) {
      HIPC(ctx->sa_full.ensure((size_t)bytes), "hipMalloc");
      hipStream_t st = nullptr;
      HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
      HIPC(launch_sa_expand(ctx->bwt, narrow ? ctx->sa_full.as<uint32_t>() : nullptr,
                            narrow ? nullptr : ctx->sa_full.as<uint64_t>(), st),
           "sa_expand launch");
      HIPC(hipStreamSynchronize(st), "sync");
      if (narrow) ctx->bwt.sa_full32 = ctx->sa_full.as<uint32_t>();
      else ctx->bwt.sa_full64 = ctx->sa_full.as<uint64_t>();
    }
  }
  ctx->has_bwt = true;
  return BWAGPU_OK;
}

extern "C" int bwagpu_bwt_sa(bwagpu_ctx_t* ctx, int64_t n, const uint64_t* k, uint64_t* out) {
  if (!ctx || n < 0 || (n && (!k || !out))) return BWAGPU_E_INVAL;
  if (!ctx->has_bwt || !ctx->bwt.sa) return fail(ctx, BWAGPU_E_INVAL, "no suffix array: pass it to bwagpu_set_bwt");
  for (int64_t i = 0; i < n; ++i)
    if (k[i] > ctx->bwt.seq_len) return fail(ctx, BWAGPU_E_INVAL, "BWT position past seq_len");
  if (n == 0) return BWAGPU_OK;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  uint64_t *d_k = nullptr, *d_out = nullptr;
  HIPC(ctx->sa_in.get(d_k, (size_t)n), "hipMalloc");
  HIPC(ctx->sa_out.get(d_out, (size_t)n), "hipMalloc");
  HIPC(hipMemcpyAsync(d_k, k, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, st), "H2D");
  HIPC(launch_bwt_sa(ctx->bwt, n, d_k, d_out, st), "bwt_sa launch");
  HIPC(hipMemcpyAsync(out, d_out, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  return BWAGPU_OK;
}

namespace {

// The pinned staging buffer of seeding's reads (seq_off, then the bases),
// once the previous call's H2D out of it is done (a caller that returned
// early on an error never synchronized its stream)
int seed_pin(bwagpu_ctx_t* ctx, int32_t n_reads, int64_t nb, char** pin) {
  if (ctx->sdh_done) HIPC(hipEventSynchronize(ctx->sdh_done), "hipEventSynchronize");
  else HIPC(hipEventCreateWithFlags(&ctx->sdh_done, hipEventDisableTiming), "hipEventCreate");
  HIPC(ctx->sdh_in.ensure(sizeof(int64_t) * ((size_t)n_reads + 1) + (size_t)nb), "hipHostMalloc");
  *pin = ctx->sdh_in.as<char>();
  return BWAGPU_OK;
}

// Checks a seeding batch (seed_host.h) and, in the same pass over the bases,
// copies the reads into the pinned staging buffer that seed_enqueue uploads.
// *bases = the batch's bases, *lq_max = the longest read.
int seed_validate(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* opt, int32_t n_reads, const int64_t* seq_off,
                  const uint8_t* seq, int64_t* bases, int* lq_max) {
  if (!ctx->has_bwt) return fail(ctx, BWAGPU_E_INVAL, "no FM-index: call bwagpu_set_bwt first");
  *bases = 0;
  *lq_max = 0;
  const char* why = "";
  int64_t nb = 0;
  if (int rc = seed_batch_check(opt, n_reads, seq_off, seq, &nb, &why)) return fail(ctx, rc, why);
  if (n_reads == 0) return BWAGPU_OK;
  char* pin = nullptr;
  TRY(seed_pin(ctx, n_reads, nb, &pin));
  if (int rc = seed_reads_check(n_reads, seq_off, seq, nb, pin, lq_max, &why)) return fail(ctx, rc, why);
  *bases = nb;
  return BWAGPU_OK;
}

// H2D of the reads out of the staging buffer seed_validate filled (when
// upload) and mem_collect_intv into per-read slots of max_per_read intervals
// (ctx->sd_*), enqueued on st
int seed_enqueue(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* opt, int32_t n_reads, int64_t bases,
                 int32_t max_per_read, bool upload, hipStream_t st, SeedArgs& a) {
  a = SeedArgs{};
  HIPC(ctx->sd_off.get(a.seq_off, (size_t)n_reads + 1), "hipMalloc");
  HIPC(ctx->sd_seq.ensure((size_t)bases + 1), "hipMalloc");
  HIPC(ctx->sd_out.get(a.out, (size_t)n_reads * (size_t)max_per_read), "hipMalloc");
  HIPC(ctx->sd_n.get(a.out_n, (size_t)n_reads), "hipMalloc");
  HIPC(ctx->sd_scratch.get(a.scratch, (size_t)seed_scratch_entries(bases, n_reads)), "hipMalloc");
  if (upload) {  // through the pinned staging buffer (a pageable H2D runs at a fraction)
    const size_t ob = sizeof(int64_t) * ((size_t)n_reads + 1);
    const char* pin = ctx->sdh_in.as<char>();
    HIPC(hipMemcpyAsync(ctx->sd_off.p, pin, ob, hipMemcpyHostToDevice, st), "H2D");
    if (bases) HIPC(hipMemcpyAsync(ctx->sd_seq.p, pin + ob, (size_t)bases, hipMemcpyHostToDevice, st), "H2D");
    HIPC(hipEventRecord(ctx->sdh_done, st), "hipEventRecord");
  }
  a.n_reads = n_reads;
  a.seq = ctx->sd_seq.as<uint8_t>();
  a.max_per_read = max_per_read;
  a.min_seed_len = opt->min_seed_len;
  a.split_width = opt->split_width;
  a.max_mem_intv = opt->max_mem_intv;
  a.split_len = (int)(opt->min_seed_len * opt->split_factor + .499);  // bwamem.c:124
  HIPC(ctx->sd_heavy.ensure(sizeof(int32_t) * (3 * (size_t)n_reads + 1)), "hipMalloc");
  a.budget = ctx->seed_budget;
  a.heavy = ctx->sd_heavy.as<int32_t>() + 1;
  a.n_heavy = ctx->sd_heavy.as<int32_t>();
  a.flags = a.heavy + n_reads;
  a.p3_n = a.flags + n_reads;
  if (getenv("BWAGPU_SEED_DBG")) {  // per-lane tier-1 stamps (tools_dev)
    HIPC(ctx->sd_dbg.get(a.dbg, 8 * (size_t)n_reads), "hipMalloc");
    HIPC(hipMemsetAsync(a.dbg, 0, sizeof(int64_t) * 8 * (size_t)n_reads, st), "memset");
  }
  HIPC(launch_collect_intv(ctx->bwt, a, st), "collect_intv launch");
  return BWAGPU_OK;
}

}  // namespace

extern "C" int bwagpu_collect_intv(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* opt, int32_t n_reads,
                                   const int64_t* seq_off, const uint8_t* seq, int32_t max_per_read,
                                   bwagpu_intv_t* out, int64_t out_cap, int32_t* out_n) {
  if (!ctx || !opt || n_reads < 0 || max_per_read < 1 || out_cap < 0 || (n_reads && (!seq_off || !out_n)) ||
      (out_cap && !out))
    return BWAGPU_E_INVAL;
  int64_t bases = 0;
  int lq_max = 0;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = seed_validate(ctx, opt, n_reads, seq_off, seq, &bases, &lq_max);
  if (rc) return rc;
  if (n_reads == 0) return BWAGPU_OK;
  hipStream_t st = nullptr;
  HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  SeedArgs a;
  if ((rc = seed_enqueue(ctx, opt, n_reads, bases, max_per_read, true, st, a))) return rc;
  HIPC(hipMemcpyAsync(out_n, ctx->sd_n.p, sizeof(int32_t) * (size_t)n_reads, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  if (const char* dp = getenv("BWAGPU_SEED_DBG")) {
    std::vector<int64_t> d(8 * (size_t)n_reads);
    HIPC(hipMemcpy(d.data(), ctx->sd_dbg.p, sizeof(int64_t) * d.size(), hipMemcpyDeviceToHost), "D2H");
    if (FILE* f = fopen(dp, "ab")) {
      fwrite(d.data(), sizeof(int64_t), d.size(), f);
      fclose(f);
    }
  }
  // pack the per-read slots back to back (read order) and copy only those
  std::vector<int64_t> off((size_t)n_reads + 1, 0);
  for (int32_t r = 0; r < n_reads; ++r) {
    if (out_n[r] < 0) return fail(ctx, BWAGPU_E_UNSUPPORTED, "a read has more than max_per_read intervals");
    off[(size_t)r + 1] = off[(size_t)r] + out_n[r];
  }
  const int64_t total = off[(size_t)n_reads];
  if (total > out_cap) return fail(ctx, BWAGPU_E_UNSUPPORTED, "the batch has more than out_cap intervals");
  if (total == 0) return BWAGPU_OK;
  int64_t* d_off = nullptr;
  bwagpu_intv_t* d_pack = nullptr;
  HIPC(ctx->sd_poff.get(d_off, off.size()), "hipMalloc");
  HIPC(ctx->sd_pack.get(d_pack, (size_t)total), "hipMalloc");
  HIPC(hipMemcpyAsync(d_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, st), "H2D");
  HIPC(launch_pack_intv(a, d_off, d_pack, st), "pack launch");
  HIPC(hipMemcpyAsync(out, d_pack, sizeof(bwagpu_intv_t) * (size_t)total, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  return BWAGPU_OK;
}

extern "C" int bwagpu_debug_seed_budget(bwagpu_ctx_t* ctx, int32_t budget) {
  if (!ctx || budget < 0) return BWAGPU_E_INVAL;
  ctx->seed_budget = budget;
  return BWAGPU_OK;
}

extern "C" int bwagpu_debug_sup_shift(bwagpu_ctx_t* ctx, int32_t shift) {
  if (!ctx || shift < 7 || shift > 32) return BWAGPU_E_INVAL;  // a superblock is whole 128-position bwa blocks
  ctx->sup_shift = shift;
  return BWAGPU_OK;
}

extern "C" int bwagpu_set_alt(bwagpu_ctx_t* ctx, const uint8_t* is_alt) {
  if (!ctx) return BWAGPU_E_INVAL;
  if (!is_alt) {
    ctx->has_alt = false;
    return BWAGPU_OK;
  }
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  uint8_t* alt = nullptr;
  HIPC(ctx->ch_alt.get(alt, (size_t)ctx->ref.n_seqs), "hipMalloc");
  HIPC(hipMemcpy(alt, is_alt, (size_t)ctx->ref.n_seqs, hipMemcpyHostToDevice), "H2D");
  ctx->has_alt = true;
  return BWAGPU_OK;
}

// ------------------------------------------------------------------ chaining
// SeqsToChains on the device (chain.h): mem_collect_intv, mem_chain's body,
// mem_chain_flt and mem_flt_chained_seeds, with three host round trips for
// sizes (positions, mem_seed_sw tasks when a read is long enough for them,
// chains out).  run_chaining is these steps, in the order they are enqueued.
namespace {

// the options, and what the chaining kernels need of the context and the device
int chain_gate(bwagpu_ctx_t* ctx, const bwagpu_chainopt_t* copt) {
  const char* why = "";
  if (int rc = chain_opt_check(copt, &why)) return fail(ctx, rc, why);
  if (!ctx->bwt.sa) return fail(ctx, BWAGPU_E_INVAL, "no suffix array: pass it to bwagpu_set_bwt");
  // the largest LDS bin's arena (chain.h) needs gfx950's 160 KB per workgroup
  int lds_max = 0;
  HIPC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device), "attribute");
  if ((size_t)lds_max < lds_arena(kBinCap[kLdsBins - 1]))
    return fail(ctx, BWAGPU_E_UNSUPPORTED, "device LDS per workgroup is smaller than the chaining arena");
  return BWAGPU_OK;
}

// the per-read buffers, the gate table's upload and the batch's constants -> a; *tot = the pinned size words
int chain_args(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* sopt, const bwagpu_chainopt_t* copt, int32_t n_reads,
               const SeedArgs& sa, const std::vector<int32_t>& tab, bool raw, hipStream_t st, ChainArgs& a,
               int64_t** tot) {
  const size_t nr = (size_t)n_reads;
  HIPC(ctx->ch_npos.get(a.n_pos, nr), "hipMalloc");
  HIPC(ctx->ch_posoff.get(a.pos_off, nr + 1), "hipMalloc");
  HIPC(ctx->ch_frac.get(a.frac_rep, nr), "hipMalloc");
  HIPC(ctx->ch_nout.get(a.n_out, nr), "hipMalloc");
  HIPC(ctx->ch_noseed.get(a.n_oseed, nr), "hipMalloc");
  HIPC(ctx->ch_nsw.get(a.n_sw, nr), "hipMalloc");
  HIPC(ctx->ch_need.get(a.need, 1), "hipMalloc");
  HIPC(ctx->ch_swtab.get(a.sw_tab, tab.size()), "hipMalloc");
  HIPC(ctx->chh_tot.get(*tot, 8), "hipHostMalloc");
  HIPC(hipMemcpyAsync(ctx->ch_swtab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, st), "H2D");
  a.n_reads = n_reads;
  a.seq_off = sa.seq_off;
  a.seq = sa.seq;
  a.max_occ = copt->max_occ;
  a.max_chain_gap = copt->max_chain_gap;
  a.min_chain_weight = copt->min_chain_weight;
  a.max_chain_extend = copt->max_chain_extend;
  a.mask_level = copt->mask_level;
  a.drop_ratio = copt->drop_ratio;
  a.min_seed_len = sopt->min_seed_len;
  a.w = ctx->opt.w;
  a.a = ctx->opt.a;
  a.raw = raw ? 1 : 0;
  a.l_pac = ctx->ref.l_pac;
  a.n_seqs = ctx->ref.n_seqs;
  a.ann_off = ctx->ref.ann_offset;
  a.ann_len = ctx->ref.ann_len;
  a.is_alt = ctx->has_alt ? ctx->ch_alt.as<uint8_t>() : nullptr;
  a.pac = ctx->ref.pac;
  return BWAGPU_OK;
}

// positions per read -> tot[0]; a read out of interval slots reruns the search once
int chain_positions(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* sopt, int32_t n_reads, int64_t bases, hipStream_t st,
                    SeedArgs& sa, ChainArgs& a, int64_t* tot) {
  for (int pass = 0;; ++pass) {
    a.intv = sa.out;
    a.intv_n = sa.out_n;
    a.max_per_read = sa.max_per_read;
    HIPC(hipMemsetAsync(a.need, 0, sizeof(int32_t), st), "memset");
    HIPC(launch_chain_count(a, st), "chain_count launch");
    HIPC(launch_scan_i32(a.n_pos, a.pos_off, n_reads, st), "scan launch");
    HIPC(hipMemcpyAsync(tot, a.pos_off + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipMemcpyAsync(tot + 1, a.need, sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H");
    HIPC(hipStreamSynchronize(st), "sync");
    const int32_t need = (int32_t)(uint32_t)tot[1];
    if (need <= 0) return BWAGPU_OK;
    if (pass) return fail(ctx, BWAGPU_E_DEVICE, "interval slots still overflow");
    TRY(seed_enqueue(ctx, sopt, n_reads, bases, need, false, st, sa));
  }
}

// BWAGPU_CHAIN_PHASES=1: the slowest reads' phase times (100 MHz ticks) to stderr
int chain_phase_dump(bwagpu_ctx_t* ctx, int32_t n_reads, hipStream_t st) {
  const size_t nr = (size_t)n_reads;
  std::vector<uint64_t> d(8 * nr);
  HIPC(hipMemcpyAsync(d.data(), ctx->ch_dbg.p, sizeof(uint64_t) * 8 * nr, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  std::vector<int> idx;
  for (int r = 0; r < n_reads; ++r)
    if (d[8 * (size_t)r + 6]) idx.push_back(r);
  std::sort(idx.begin(), idx.end(), [&](int x, int y) {
    return d[8 * (size_t)x + 6] - d[8 * (size_t)x] > d[8 * (size_t)y + 6] - d[8 * (size_t)y];
  });
  for (size_t k = 0; k < idx.size() && k < 8; ++k) {
    const uint64_t* q = &d[8 * (size_t)idx[k]];
    fprintf(stderr, "[chain phases] read %d pos %u chains %u: loop %.1f trav %.1f prep %.1f sort %.1f flt %.1f out %.1f us\n",
            idx[k], (unsigned)(q[7] & 0xffffffff), (unsigned)(q[7] >> 32), (q[1] - q[0]) / 100.0,
            (q[2] - q[1]) / 100.0, (q[3] ? q[3] - q[2] : 0) / 100.0, (q[4] ? q[4] - q[3] : 0) / 100.0,
            (q[5] - (q[4] ? q[4] : q[2])) / 100.0, (q[6] - q[5]) / 100.0);
  }
  return BWAGPU_OK;
}

// the P positions' buffers, then chain_emit, bwt_sa and chain_build
int chain_build(bwagpu_ctx_t* ctx, int32_t n_reads, int64_t P, ChainArgs& a, hipStream_t st) {
  const size_t nr = (size_t)n_reads, np = (size_t)P;
  HIPC(ctx->ch_kpos.get(a.kpos, np), "hipMalloc");
  HIPC(ctx->ch_rbeg.get(a.rbeg, np), "hipMalloc");
  HIPC(ctx->ch_qinfo.get(a.qinfo, np), "hipMalloc");
  HIPC(ctx->ch_label.get(a.label, np), "hipMalloc");
  HIPC(ctx->ch_score.get(a.score, np), "hipMalloc");
  HIPC(ctx->ch_slist.get(a.slist, np), "hipMalloc");
  HIPC(ctx->ch_ord.get(a.ord, np), "hipMalloc");
  HIPC(ctx->ch_chains.get(a.lchains, np), "hipMalloc");
  HIPC(ctx->ch_nodes.get(a.lnodes, (size_t)node_total(P, n_reads)), "hipMalloc");
  HIPC(ctx->ch_ochains.get(a.ochains, np), "hipMalloc");
  HIPC(ctx->ch_oslist.get(a.oslist, np), "hipMalloc");
  HIPC(ctx->ch_bins.ensure(sizeof(int32_t) * ((size_t)(kLdsBins + 1) * nr + kLdsBins + 1)), "hipMalloc");
  a.bin_count = ctx->ch_bins.as<int32_t>();
  a.bin_list = a.bin_count + kLdsBins + 1;
  HIPC(launch_chain_emit(a, st), "chain_emit launch");
  if (P) HIPC(launch_bwt_sa(ctx->bwt, P, a.kpos, a.rbeg, st), "bwt_sa launch");
  if (!ctx->ch_cs.fork) {
    HIPC(hipStreamCreateWithFlags(&ctx->ch_cs.side[0], hipStreamNonBlocking), "hipStreamCreate");
    HIPC(hipEventCreateWithFlags(&ctx->ch_cs.join[0], hipEventDisableTiming), "hipEventCreate");
    HIPC(hipEventCreateWithFlags(&ctx->ch_cs.fork, hipEventDisableTiming), "hipEventCreate");
  }
  const char* dbg_env = getenv("BWAGPU_CHAIN_PHASES");
  const bool dbg_on = dbg_env && dbg_env[0] == '1';
  if (dbg_on) {
    HIPC(ctx->ch_dbg.get(a.dbg, 8 * nr), "hipMalloc");
    HIPC(hipMemsetAsync(a.dbg, 0, sizeof(uint64_t) * 8 * nr, st), "memset");
  }
  HIPC(launch_chain_build(a, st, ctx->ch_cs), "chain_build launch");
  return dbg_on ? chain_phase_dump(ctx, n_reads, st) : BWAGPU_OK;
}

// mem_flt_chained_seeds: every kept seed of a long read realigned (mem_seed_sw); tot[2] = the tasks
int chain_seed_sw(bwagpu_ctx_t* ctx, int32_t n_reads, const ChainArgs& a, int64_t* tot, hipStream_t st) {
  int64_t* sw_off = nullptr;
  HIPC(ctx->ch_swoff.get(sw_off, (size_t)n_reads + 1), "hipMalloc");
  HIPC(launch_scan_i32(a.n_sw, sw_off, n_reads, st), "scan launch");
  HIPC(hipMemcpyAsync(tot + 2, sw_off + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  const int64_t T = tot[2];
  if (T > INT32_MAX / 2) return fail(ctx, BWAGPU_E_UNSUPPORTED, "too many seeds to realign");
  if (!T) return BWAGPU_OK;
  ChainSw sw{};
  bwagpu_kswr_t* res = nullptr;
  sw.sw_off = sw_off;
  HIPC(ctx->ch_swtasks.get(sw.tasks, (size_t)T), "hipMalloc");
  HIPC(ctx->ch_swt.get(sw.tpool, (size_t)kSwWin * (size_t)T), "hipMalloc");
  HIPC(ctx->ch_swskip.get(sw.skip, (size_t)T), "hipMalloc");
  HIPC(ctx->ch_swres.get(res, (size_t)T), "hipMalloc");
  HIPC(ctx->ch_swscr.ensure(8 * ((size_t)kSwWin * (size_t)T + (size_t)T)), "hipMalloc");
  sw.res = res;
  HIPC(launch_chain_sw_prep(a, sw, st), "chain_sw_prep launch");
  TRY(bwagpu_align2_device(ctx, (int32_t)T, sw.tasks, a.seq, sw.tpool, res, ctx->ch_swscr.p, st));
  HIPC(launch_chain_sw_apply(a, sw, st), "chain_sw_apply launch");
  return BWAGPU_OK;
}

// the chains' and seeds' totals (tot[3], tot[4]), then the batch layout packed into ctx->ch_* —
// or, to_host, over PCIe into the pinned chh_* that bwagpu_seqs2chains returns (no D2H step)
int chain_pack(bwagpu_ctx_t* ctx, int32_t n_reads, const ChainArgs& a, int64_t* tot, bool to_host, hipStream_t st,
               int64_t* n_chains, int64_t* n_seeds) {
  const size_t nr = (size_t)n_reads;
  int64_t *oc_off = nullptr, *os_off = nullptr;
  HIPC(ctx->ch_ocoff.get(oc_off, nr + 1), "hipMalloc");
  HIPC(ctx->ch_osoff.get(os_off, nr + 1), "hipMalloc");
  HIPC(launch_scan_i32(a.n_out, oc_off, n_reads, st), "scan launch");
  HIPC(launch_scan_i32(a.n_oseed, os_off, n_reads, st), "scan launch");
  HIPC(hipMemcpyAsync(tot + 3, oc_off + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipMemcpyAsync(tot + 4, os_off + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  const int64_t nc = tot[3], ns = tot[4];
  if (nc > INT32_MAX - 1 || ns > INT32_MAX - 1) return fail(ctx, BWAGPU_E_UNSUPPORTED, "batch has too many chains");
  ChainPack pk{};
  pk.oc_off = oc_off;
  pk.os_off = os_off;
  HIPC(ctx->ch_rco.get(pk.read_chain_off, nr + 1), "hipMalloc");
  HIPC(ctx->ch_cso.get(pk.chain_seed_off, (size_t)nc + 1), "hipMalloc");
  HIPC(ctx->ch_rid.get(pk.chain_rid, (size_t)nc), "hipMalloc");
  HIPC(ctx->ch_cfrac.get(pk.chain_frac, (size_t)nc), "hipMalloc");
  HIPC(ctx->ch_out.get(pk.chains, (size_t)nc), "hipMalloc");
  HIPC(ctx->ch_seeds.get(pk.seeds, (size_t)ns), "hipMalloc");
  if (to_host) {
    HIPC(ctx->chh_rco.get(pk.read_chain_off, nr + 1), "hipHostMalloc");  // the host's pointers, replaced below
    HIPC(ctx->chh_cso.get(pk.chain_seed_off, (size_t)nc + 1), "hipHostMalloc");
    HIPC(ctx->chh_chains.get(pk.chains, (size_t)nc), "hipHostMalloc");
    HIPC(ctx->chh_seeds.get(pk.seeds, (size_t)ns), "hipHostMalloc");
    HIPC(hipHostGetDevicePointer((void**)&pk.read_chain_off, ctx->chh_rco.p, 0), "hipHostGetDevicePointer");
    HIPC(hipHostGetDevicePointer((void**)&pk.chain_seed_off, ctx->chh_cso.p, 0), "hipHostGetDevicePointer");
    HIPC(hipHostGetDevicePointer((void**)&pk.chains, ctx->chh_chains.p, 0), "hipHostGetDevicePointer");
    HIPC(hipHostGetDevicePointer((void**)&pk.seeds, ctx->chh_seeds.p, 0), "hipHostGetDevicePointer");
  }
  HIPC(launch_chain_pack(a, pk, st), "chain_pack launch");
  *n_chains = nc;
  *n_seeds = ns;
  return BWAGPU_OK;
}

int run_chaining(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* sopt, const bwagpu_chainopt_t* copt, int32_t n_reads,
                 const int64_t* seq_off, const uint8_t* seq, bool raw, hipStream_t st, int64_t* n_chains,
                 int64_t* n_seeds, int* lq_max_out, bool to_host = false) {
  *n_chains = *n_seeds = 0;
  TRY(chain_gate(ctx, copt));
  int64_t bases = 0;
  int lq_max = 0;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  TRY(seed_validate(ctx, sopt, n_reads, seq_off, seq, &bases, &lq_max));  // + the staging copy
  *lq_max_out = lq_max;
  if (n_reads == 0) return BWAGPU_OK;
  std::vector<int32_t> tab;
  const bool any_sw = seed_sw_table(copt, ctx->opt.a, sopt->min_seed_len, n_reads, seq_off, lq_max, &tab);
  if (!raw && any_sw)
    if (const char* why = align2_opt_unsupported(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, why);
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  SeedArgs sa;
  // interval slots per read: 2 * lq_max + 64, grown once on overflow (chain_positions)
  TRY(seed_enqueue(ctx, sopt, n_reads, bases, std::max(64, 2 * lq_max + 64), true, st, sa));
  ChainArgs a{};
  int64_t* tot = nullptr;
  TRY(chain_args(ctx, sopt, copt, n_reads, sa, tab, raw, st, a, &tot));
  TRY(chain_positions(ctx, sopt, n_reads, bases, st, sa, a, tot));
  TRY(chain_build(ctx, n_reads, tot[0], a, st));
  if (!raw && any_sw) TRY(chain_seed_sw(ctx, n_reads, a, tot, st));
  return chain_pack(ctx, n_reads, a, tot, to_host, st, n_chains, n_seeds);
}

}  // namespace

extern "C" int bwagpu_seqs2chains(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* sopt, const bwagpu_chainopt_t* copt,
                                  int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, int32_t raw,
                                  bwagpu_chains_t* out) {
  if (!ctx || !sopt || !copt || !out || n_reads < 0 || (n_reads && !seq_off)) return BWAGPU_E_INVAL;
  *out = bwagpu_chains_t{};
  hipStream_t st = nullptr;
  HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  int64_t nc = 0, ns = 0;
  int lq = 0;
  int rc = run_chaining(ctx, sopt, copt, n_reads, seq_off, seq, raw != 0, st, &nc, &ns, &lq, true);
  if (rc) return rc;
  const size_t nr = (size_t)n_reads;
  int32_t *rco = nullptr, *cso = nullptr;
  bwagpu_chain_t* chains = nullptr;
  bwagpu_seed_t* seeds = nullptr;
  HIPC(ctx->chh_rco.get(rco, nr + 1), "hipHostMalloc");
  HIPC(ctx->chh_cso.get(cso, (size_t)nc + 1), "hipHostMalloc");
  HIPC(ctx->chh_chains.get(chains, (size_t)nc), "hipHostMalloc");
  HIPC(ctx->chh_seeds.get(seeds, (size_t)ns), "hipHostMalloc");
  if (n_reads) HIPC(hipStreamSynchronize(st), "sync");  // chain_pack wrote the results into the pinned buffers
  else rco[0] = cso[0] = 0;
  *out = bwagpu_chains_t{n_reads, (int32_t)nc, ns, rco, cso, chains, seeds};
  return BWAGPU_OK;
}

extern "C" int bwagpu_seqs2regions(bwagpu_ctx_t* ctx, const bwagpu_seedopt_t* sopt, const bwagpu_chainopt_t* copt,
                                   int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, int32_t* out_n,
                                   const bwagpu_alnreg_t** regs, int64_t* n_regs) {
  if (!ctx || !sopt || !copt || !regs || !n_regs || n_reads < 0 || (n_reads && (!seq_off || !out_n)))
    return BWAGPU_E_INVAL;
  *regs = nullptr;
  *n_regs = 0;
  for (int32_t r = 0; r < n_reads; ++r)
    if (seq_off[r + 1] - seq_off[r] > BWAGPU_MAX_READ_LEN)
      return fail(ctx, BWAGPU_E_UNSUPPORTED, "read longer than BWAGPU_MAX_READ_LEN");
  hipStream_t st = nullptr;
  HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  int64_t nc = 0, ns = 0;
  int lq = 0;
  int rc = run_chaining(ctx, sopt, copt, n_reads, seq_off, seq, false, st, &nc, &ns, &lq);
  if (rc) return rc;
  if (n_reads == 0) return BWAGPU_OK;
  if ((rc = check_lds(ctx, lq))) return rc;
  Slot& s = ctx->ch_slot;
  const size_t nr = (size_t)n_reads;
  bwagpu_alnreg_t *d_out = nullptr, *d_regc = nullptr, *h_regs = nullptr;
  int32_t* d_n = nullptr;
  int64_t *d_stats = nullptr, *d_regoff = nullptr;
  HIPC(s.d_out.get(d_out, (size_t)ns), "hipMalloc(out)");
  HIPC(s.d_n.get(d_n, nr), "hipMalloc(out_n)");
  HIPC(s.d_stats.get(d_stats, ST_N), "hipMalloc(stats)");
  HIPC(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * ST_N, st), "memset stats");
  DevBatch db;
  db.n_reads = n_reads;
  db.n_chains = (int32_t)nc;
  db.n_seeds = (int32_t)ns;
  db.seq_off = ctx->sd_off.as<int64_t>();
  db.seq = ctx->sd_seq.as<uint8_t>();
  db.read_chain_off = ctx->ch_rco.as<int32_t>();
  db.chain_seed_off = ctx->ch_cso.as<int32_t>();
  db.chain_rid = ctx->ch_rid.as<int32_t>();
  db.chain_frac_rep = ctx->ch_cfrac.as<float>();
  db.seeds = ctx->ch_seeds.as<bwagpu_seed_t>();
  if ((rc = enqueue_chain2aln(ctx, s, db, lq, d_out, d_n, d_stats, st))) return rc;
  if (ctx->post_flags) {  // bwagpu_set_regs_post: before the counts are scanned and the regions compacted
    if ((rc = enqueue_regpost(ctx, ctx->post_opt, ctx->post_flags, ctx->post_id0, n_reads, db.seq_off, db.seq, nullptr,
                              db.read_chain_off, db.chain_seed_off, d_out, d_n, d_stats, st)))
      return rc;
    ctx->post_id0 += n_reads;
  }
  HIPC(ctx->ch_regoff.get(d_regoff, nr + 1), "hipMalloc");
  HIPC(launch_scan_i32(d_n, d_regoff, n_reads, st), "scan launch");
  int64_t* tot = ctx->chh_tot.as<int64_t>();
  HIPC(hipMemcpyAsync(tot + 5, d_regoff + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipMemcpyAsync(tot + 6, d_stats + ST_ERR, sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipMemcpyAsync(out_n, d_n, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  const int64_t nreg = tot[5];
  HIPC(ctx->ch_regc.get(d_regc, (size_t)nreg), "hipMalloc");
  HIPC(ctx->chh_regs.get(h_regs, (size_t)nreg), "hipHostMalloc");
  HIPC(launch_reg_compact(n_reads, db.read_chain_off, db.chain_seed_off, d_out, d_regoff, d_regc, st),
       "reg_compact launch");
  if (nreg) HIPC(hipMemcpyAsync(h_regs, d_regc, sizeof(bwagpu_alnreg_t) * (size_t)nreg, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");
  *regs = h_regs;
  *n_regs = nreg;
  if (tot[6] & ERR_LEN) return fail(ctx, BWAGPU_E_UNSUPPORTED, "read longer than BWAGPU_MAX_READ_LEN");
  if (tot[6] & ERR_POST) return fail(ctx, BWAGPU_E_UNSUPPORTED, "a patch candidate's window exceeds 4096 bases");
  if (tot[6] & ERR_RID)
    return fail(ctx, BWAGPU_E_RESULTS, "a chain's first seed is not inside contig chain_rid (bwamem.c:669 assert)");
  return BWAGPU_OK;
}
