// capi_tasks.hip — the entries that take a list of tasks or a wire stream.  A blocking one
// (but reg2aln_batch: DESIGN.md §19) is its plan (task_host.h), then HostCall (ctx.h).  The plan is
// declared first, so it outlives every copy out of it: an entry that gives up
// half way leaves through HostCall's destructor, which synchronises.  The
// lists, counts, boff, starts and stats words are bookkeeping: plain copies.
#include <hip/hip_runtime.h>
#include <string.h>

#include "align2.h"
#include "ctx.h"
#include "engine.h"
#include "reg2aln.h"
#include "samtext.h"

using namespace bwagpu;

namespace {

// ksw_qinit's profile (ksw.c:69-108) as v_perm byte pools, see A2Prof
A2Prof make_a2prof(const DevOpt& o, bool u8) {
  int mn = 127, mx = 0;
  for (int i = 0; i < 25; ++i) {
    mn = std::min<int>(mn, o.mat[i]);
    mx = std::max<int>(mx, o.mat[i]);
  }
  const int shift = (256 - (mn & 0xff)) & 0xff;
  const int bias = u8 ? shift : 128;
  A2Prof P{};
  P.shift = shift, P.qmax = mx, P.e_del = o.e_del, P.oe_del = o.oe_del, P.e_ins = o.e_ins, P.oe_ins = o.oe_ins;
  for (int t = 0; t < 5; ++t) {
    uint32_t lo = 0;
    for (int q = 0; q < 4; ++q) lo |= (uint32_t)(uint8_t)(o.mat[t * 5 + q] + bias) << (8 * q);
    P.lo[t] = lo;
    P.hi[t] = (uint32_t)(uint8_t)(o.mat[t * 5 + 4] + bias) | (uint32_t)(uint8_t)bias << 8;
  }
  return P;
}

// Launch the given bins concurrently: fork the side streams off `st`, deal the
// bins (in the given order) round-robin over them, join back.
// counts_host: task count per bin when known (0 = unknown -> grid = capacity).
int launch_align2_concurrent(bwagpu_ctx_t* ctx, hipStream_t st, const std::vector<int>& bins, const A2Args& base,
                             const int32_t* list_off, const int32_t* counts_host, int32_t* d_counts,
                             int32_t* d_cursors, size_t list_stride) {
  int used = 0;
  if (int rc = side_fork(ctx, st, bins.size(), &used)) return rc;
  for (size_t k = 0; k < bins.size(); ++k) {
    const int b = bins[k];
    A2Args a = base;
    a.list = base.list + (list_off ? list_off[b] : (size_t)b * list_stride);
    a.count = d_counts + b;
    a.cursor = d_cursors + b;
    HIPC(launch_align2(b, a, make_a2prof(ctx->opt, b >= kA2Buckets), counts_host ? counts_host[b] : 0,
                       ctx->a2_st[k % used]),
         "align2 launch");
  }
  return side_join(ctx, st, used);
}

}  // namespace

extern "C" {

int bwagpu_extend_batch(bwagpu_ctx_t* ctx, int32_t n, const bwagpu_ext_task_t* tasks, const uint8_t* qpool,
                        int64_t qpool_len, const uint8_t* tpool, int64_t tpool_len, bwagpu_ext_result_t* results) {
  if (!ctx) return BWAGPU_E_INVAL;
  ExtendPlan plan;
  const char* why = "";
  if (int rc = extend_plan(ctx->opt, ctx->ext_form == 0, n, tasks, qpool, qpool_len, tpool, tpool_len, results, &plan,
                           &why))
    return refuse(ctx, rc, why);
  if (n == 0) return BWAGPU_OK;
  HostCall h(ctx);
  TRY(h.begin());
  hipStream_t st = h.st;
  TRY(h.up(ctx->ex_tasks, tasks, sizeof(bwagpu_ext_task_t) * n));
  TRY(h.up(ctx->ex_q, qpool, (size_t)qpool_len, 1));
  TRY(h.up(ctx->ex_t, tpool, (size_t)tpool_len, 1));
  int32_t* lists = nullptr;
  bwagpu_ext_result_t* res = nullptr;
  int64_t* stats = nullptr;
  TRY(h.reserve(ctx->ex_list, lists, (size_t)n));
  TRY(h.reserve(ctx->ex_res, res, (size_t)n));
  TRY(h.reserve(ctx->ex_stats, stats, ST_N));
  HIPC(hipMemcpyAsync(lists, plan.all.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st), "H2D");
  HIPC(hipMemsetAsync(stats, 0, sizeof(int64_t) * ST_N, st), "memset");
  TRY(h.start());
  const bwagpu_ext_task_t* d_tasks = ctx->ex_tasks.as<bwagpu_ext_task_t>();
  const uint8_t *d_q = ctx->ex_q.as<uint8_t>(), *d_t = ctx->ex_t.as<uint8_t>();
  for (int v = 0; v < kExtLists; ++v) {
    if (!plan.count[v]) continue;
    const int32_t* list = lists + plan.off[v];
    HIPC(v < kNumExtVariants
             ? launch_extend(v, plan.t5, ctx->opt, n, d_tasks, list, plan.count[v], d_q, d_t, plan.tb[v], res, stats, st)
             : launch_extend4(ctx->opt, d_tasks, list, plan.count[v], d_q, d_t, plan.tb[v], res, stats, st),
         "extend launch");
  }
  TRY(h.stop());
  TRY(h.down(results, ctx->ex_res, sizeof(bwagpu_ext_result_t) * n));
  return h.finish("extend batch", stats);
}

int bwagpu_reg2aln_batch(bwagpu_ctx_t* ctx, int32_t n, const bwagpu_reg2aln_task_t* tasks, const uint8_t* qpool,
                         int64_t qpool_len, int32_t max_ops, int32_t max_md, bwagpu_aln_t* out, uint32_t* cigar,
                         char* md) {
  if (!ctx || n < 0 || (n && (!tasks || !out || !cigar || !md)) || qpool_len < 0 || (qpool_len && !qpool) ||
      max_ops < 1 || max_md < 1)
    return BWAGPU_E_INVAL;
  if (n == 0) return BWAGPU_OK;
  const DevOpt& o = ctx->opt;
  const int64_t l_pac = ctx->ref.l_pac, two = l_pac << 1;
  const int wmax = o.w << 2;
  // validate; bin by [query bucket][matrix class 0 LDS small, 1 LDS large, 2 HBM]
  struct Bin {
    std::vector<int32_t> ids;
    int qmax = 0, rmax = 0;
    int64_t zmax = 0;
  };
  Bin bins[kR2Buckets][3];
  std::vector<int64_t> cost((size_t)n, 0);
  for (int32_t k = 0; k < n; ++k) {
    const bwagpu_reg2aln_task_t& t = tasks[k];
    if (t.l_seq < 0 || t.qoff < 0 || t.qoff > qpool_len - t.l_seq)
      return fail(ctx, BWAGPU_E_INVAL, "job's read outside the query pool");
    int lq = 0, rl = 0, cls = 0;
    int64_t zb = 0;
    if (t.rb >= 0 && t.re >= 0) {
      const int64_t beg = t.rb, end = t.re > two ? two : t.re;
      const bool ok = t.qe > t.qb && t.rb < t.re && !(t.rb < l_pac && t.re > l_pac) &&
                      (beg >= l_pac || end <= l_pac) && end - beg == t.re - t.rb;
      if (ok) {
        if (t.qb < 0 || t.qe > t.l_seq) return fail(ctx, BWAGPU_E_INVAL, "job's qb/qe outside its read");
        lq = t.qe - t.qb;
        if (lq > BWAGPU_MAX_READ_LEN) return fail(ctx, BWAGPU_E_UNSUPPORTED, "qe - qb > BWAGPU_MAX_READ_LEN");
        if (t.re - t.rb > kR2MaxRef) return fail(ctx, BWAGPU_E_UNSUPPORTED, "re - rb > 8192");
        rl = (int)(t.re - t.rb);
        // the widest band any try can use: the first try's w2 (infer_bw,
        // bwamem.c:1123-1126) doubled at most twice (1132), capped at
        // opt->w << 2, then bwa.c:152-159
        auto infer = [&](int q_, int r_) {
          if (lq == rl && lq * o.a - t.truesc < (q_ + r_ - o.a) * 2) return 0;
          const int w = (int)((double)(std::min(lq, rl) * o.a - t.truesc - q_) / r_ + 2.);
          return std::max(w, std::abs(lq - rl));
        };
        int w2 = std::max(infer(o.o_del, o.e_del), infer(o.o_ins, o.e_ins));
        if (w2 > o.w) w2 = std::min(w2, t.w);
        w2 = std::min(w2, wmax);
        const int w2max = (int)std::min<int64_t>((int64_t)w2 * 4, wmax);
        const int half = (lq + 1) >> 1;
        const int mi = (int)((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
        const int mdl = (int)((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
        const int mg = std::max(std::max(mi, mdl), 1), dl = std::abs(rl - lq);
        const int wb = std::max(std::min((mg + dl + 1) >> 1, w2max), dl + 3);
        zb = (int64_t)std::min(lq, 2 * wb + 1) * rl;
        cls = zb <= kR2ZSmall ? 0 : (zb <= kR2ZLarge ? 1 : 2);
      }
    }
    Bin& b = bins[r2_bucket_of(lq)][cls];
    b.ids.push_back(k);
    b.qmax = std::max(b.qmax, lq);
    b.rmax = std::max(b.rmax, rl);
    b.zmax = std::max(b.zmax, zb);
    cost[(size_t)k] = zb + lq + rl;
  }
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIPC(lazy_stream(ctx->slot[0], &st), "hipStreamCreate");
  R2AArgs base{};  // what the launches of all bins share
  int32_t* lists = nullptr;
  HIPC(ctx->r2_tasks.get(base.tasks, (size_t)n), "hipMalloc");
  HIPC(ctx->r2_q.ensure((size_t)qpool_len + 1), "hipMalloc");
  HIPC(ctx->r2_out.get(base.out, (size_t)n), "hipMalloc");
  HIPC(ctx->r2_cig.get(base.cigar, (size_t)n * max_ops), "hipMalloc");
  HIPC(ctx->r2_md.get(base.md, (size_t)n * max_md), "hipMalloc");
  HIPC(ctx->r2_lists.get(lists, (size_t)n), "hipMalloc");
  HIPC(ctx->r2_stats.get(base.stats, ST_N), "hipMalloc");
  base.qpool = ctx->r2_q.as<uint8_t>(), base.max_ops = max_ops, base.max_md = max_md;
  std::vector<int32_t> all;
  all.reserve((size_t)n);
  for (auto& row : bins)
    for (auto& b : row) {
      // largest matrices first: the last claims are the small jobs
      std::stable_sort(b.ids.begin(), b.ids.end(), [&](int32_t x, int32_t y) { return cost[x] > cost[y]; });
      all.insert(all.end(), b.ids.begin(), b.ids.end());
    }
  HIPC(hipMemcpyAsync(ctx->r2_tasks.p, tasks, sizeof(bwagpu_reg2aln_task_t) * n, hipMemcpyHostToDevice, st), "H2D");
  if (qpool_len) HIPC(hipMemcpyAsync(ctx->r2_q.p, qpool, (size_t)qpool_len, hipMemcpyHostToDevice, st), "H2D");
  HIPC(hipMemcpyAsync(ctx->r2_lists.p, all.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st), "H2D");
  HIPC(hipMemsetAsync(ctx->r2_stats.p, 0, sizeof(int64_t) * ST_N, st), "memset");
  // bins run concurrently on the context's side streams, largest first
  struct Launch { int bk, cls; int32_t off; int64_t work; };
  std::vector<Launch> launches;
  int32_t off = 0;
  for (int bk = 0; bk < kR2Buckets; ++bk)
    for (int cls = 0; cls < 3; ++cls) {
      const Bin& b = bins[bk][cls];
      if (b.ids.empty()) continue;
      int64_t w = 0;
      for (int32_t k : b.ids) w += cost[(size_t)k];
      launches.push_back({bk, cls, off, w});
      off += (int32_t)b.ids.size();
    }
  std::sort(launches.begin(), launches.end(), [](const Launch& x, const Launch& y) { return x.work > y.work; });
  EventPair ev;
  HIPC(ev.start(st), "event");
  int used = 0;
  TRY(side_fork(ctx, st, launches.size(), &used));
  auto make_args = [&](const Launch& L, int& wpb) {
    const Bin& b = bins[L.bk][L.cls];
    R2AArgs a = base;
    a.list = lists + L.off, a.n = (int)b.ids.size();
    a.qcap = (b.qmax + 16) & ~15;
    a.rcap = (b.rmax + 16) & ~15;
    a.ocap = a.qcap + a.rcap + 4;
    int lpw = a.qcap + a.rcap + 4 * a.ocap;
    if (L.cls < 2) lpw += L.cls == 0 ? kR2ZSmall : kR2ZLarge;
    a.lds_per_wave = (lpw + 15) & ~15;
    wpb = L.cls == 1 ? 1 : 4;  // LDS-heavy bins: one wave per workgroup packs LDS finer
    a.zstride = L.cls == 2 ? ((b.zmax + 255) & ~(int64_t)255) : 0;
    return a;
  };
  // grids first (HBM matrix slices: one per launched wave, at most 1 GiB per bin)
  size_t zoff = 0;
  for (Launch& L : launches) {
    int wpb = 4;
    const R2AArgs a = make_args(L, wpb);
    if ((size_t)wpb * a.lds_per_wave > 160 * 1024)
      return fail(ctx, BWAGPU_E_UNSUPPORTED, "reg2aln job needs more LDS than a workgroup has");
    int waves = r2_resident_waves(kR2CD[L.bk], (size_t)wpb * a.lds_per_wave, wpb);
    if (L.cls == 2) {
      waves = (int)std::min<int64_t>(waves, std::max<int64_t>(4, ((int64_t)1 << 30) / a.zstride));
      zoff += (size_t)a.zstride * waves;
    }
    L.work = waves;
  }
  uint8_t* z = nullptr;
  HIPC(ctx->r2_z.get(z, std::max<size_t>(zoff, 256)), "hipMalloc(reg2aln matrices)");
  zoff = 0;
  for (size_t li = 0; li < launches.size(); ++li) {
    const Launch& L = launches[li];
    int wpb = 4;
    R2AArgs a = make_args(L, wpb);
    const int nb = a.n, waves = (int)L.work;
    if (L.cls == 2) {
      a.zglob = z + zoff;
      zoff += (size_t)a.zstride * waves;
    }
    const int blocks = std::max(1, std::min((nb + wpb - 1) / wpb, waves / wpb));
    HIPC(launch_reg2aln(kR2CD[L.bk], o, ctx->ref, a, blocks, wpb, ctx->a2_st[li % used]), "reg2aln launch");
  }
  TRY(side_join(ctx, st, used));
  HIPC(ev.stop(st), "event");
  HIPC(hipMemcpyAsync(out, ctx->r2_out.p, sizeof(bwagpu_aln_t) * n, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipMemcpyAsync(cigar, ctx->r2_cig.p, sizeof(uint32_t) * (size_t)n * max_ops, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipMemcpyAsync(md, ctx->r2_md.p, (size_t)n * max_md, hipMemcpyDeviceToHost, st), "D2H");
  int64_t hst[ST_N];
  HIPC(hipMemcpyAsync(hst, ctx->r2_stats.p, sizeof(hst), hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "reg2aln execution");
  bwagpu_stats_t& last = ctx->slot[0].last = bwagpu_stats_t{};
  last.kernel_ms = ev.ms(), last.cells = hst[ST_CELLS], last.rows = hst[ST_ROWS], last.ext_calls = hst[ST_CALLS];
  last.h2d_bytes = (int64_t)sizeof(bwagpu_reg2aln_task_t) * n + qpool_len;
  last.d2h_bytes = (int64_t)n * ((int64_t)sizeof(bwagpu_aln_t) + 4 * (int64_t)max_ops + max_md);
  return BWAGPU_OK;
}

// The CIGAR kernel on jobs that are already in device memory.
// The device classifies and bins (reg2aln_classify_kernel), the bin table comes
// to the host once, and from its measured maxima the bins get the capacities,
// grids and HBM slices of bwagpu_reg2aln_batch's make_args — those formulas are
// written a second time here on purpose (§19: that body is left alone).
int bwagpu_reg2aln_device(bwagpu_ctx_t* ctx, int32_t n_cap, const int32_t* dev_n_tasks,
                          const bwagpu_reg2aln_task_t* dev_tasks, const uint8_t* dev_qpool, int64_t qpool_len,
                          int32_t max_ops, int32_t max_md, bwagpu_aln_t* dev_out, uint32_t* dev_cigar, char* dev_md,
                          void* stream) {
  if (!ctx || n_cap < 0 || max_ops < 1 || max_md < 1 || qpool_len < 0 ||
      (n_cap && (!dev_tasks || !dev_out || !dev_cigar || !dev_md || (qpool_len && !dev_qpool))))
    return BWAGPU_E_INVAL;
  if (n_cap == 0) return BWAGPU_OK;
  const bool timing = ctx->r2d_timing;  // bwagpu_debug_reg2aln_times
  const auto t_call = std::chrono::steady_clock::now();
  const DevOpt& o = ctx->opt;
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  constexpr int kKeys = kR2Bins * kR2CostClasses;
  const size_t list_bytes = sizeof(int32_t) * (size_t)n_cap, tab_bytes = sizeof(int32_t) * (kR2TabWords + kKeys);
  // an earlier device-form call, on any stream, may still be running on the scratch: a buffer grows
  // (is freed) only once that call has finished, and this call's stream touches none of it before
  if (ctx->r2d_pending && (list_bytes > ctx->r2d_keys.cap || list_bytes > ctx->r2d_lists.cap ||
                           tab_bytes > ctx->r2d_tab.cap))
    HIPC(hipEventSynchronize(ctx->r2d_done), "event sync");
  if (ctx->r2d_pending) HIPC(hipStreamWaitEvent(st, ctx->r2d_done, 0), "stream wait");
  int32_t *keys = nullptr, *lists = nullptr, *htab = nullptr;
  HIPC(ctx->r2d_keys.get(keys, (size_t)n_cap), "hipMalloc");
  HIPC(ctx->r2d_lists.get(lists, (size_t)n_cap), "hipMalloc");
  HIPC(ctx->r2d_tab.ensure(tab_bytes), "hipMalloc");  // table | scatter cursors
  HIPC(ctx->r2d_htab.get(htab, kR2TabWords), "hipHostMalloc");
  if (!ctx->r2d_done) HIPC(hipEventCreateWithFlags(&ctx->r2d_done, hipEventDisableTiming), "event");
  if (timing)
    for (hipEvent_t& e : ctx->r2d_ev)
      if (!e) HIPC(hipEventCreate(&e), "event");
  int32_t* const d_tab = ctx->r2d_tab.as<int32_t>();
  const int32_t* const h = htab;
  ctx->r2d_timed = false;
  // every way out from here on leaves the event behind what this call enqueued
  struct Done {
    bwagpu_ctx_t* ctx;
    hipStream_t st;
    ~Done() { ctx->r2d_pending = hipEventRecord(ctx->r2d_done, st) == hipSuccess || ctx->r2d_pending; }
  } done{ctx, st};
  HIPC(hipMemsetAsync(d_tab, 0, sizeof(int32_t) * (kR2TabWords + kKeys), st), "memset");
  HIPC(launch_reg2aln_classify(o, ctx->ref.l_pac, qpool_len, n_cap, dev_n_tasks, dev_tasks, keys, dev_out, d_tab, st),
       "reg2aln classify launch");
  HIPC(hipMemcpyAsync(htab, d_tab, sizeof(int32_t) * kR2TabWords, hipMemcpyDeviceToHost, st), "D2H");
  const auto t_wait = std::chrono::steady_clock::now();
  // the stream waited for the previous device-form call first, so that call has finished too
  HIPC(hipStreamSynchronize(st), "reg2aln classification");
  if (timing)
    ctx->r2d_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wait).count();
  // the one list: bins in order, inside a bin the cost classes from the largest down
  R2Offsets off{};
  int32_t bin_off[kR2Bins], at = 0;
  for (int b = 0; b < kR2Bins; ++b) {
    bin_off[b] = at;
    for (int c = 0; c < kR2CostClasses; ++c) {
      off.at[b * kR2CostClasses + c] = at;
      at += h[kR2TabClass + b * kR2CostClasses + c];
    }
    if (at - bin_off[b] != h[4 * b] || at > n_cap) return fail(ctx, BWAGPU_E_DEVICE, "reg2aln bin table is inconsistent");
  }
  struct Launch { int bk, cls, n; int32_t off; int64_t work; int wpb, waves; R2AArgs a; };
  std::vector<Launch> launches;
  for (int b = 0; b < kR2Bins; ++b)
    if (h[4 * b])
      launches.push_back({b / 3, b % 3, h[4 * b], bin_off[b], (int64_t)h[4 * b] * ((int64_t)h[4 * b + 3] + h[4 * b + 1] + h[4 * b + 2])});
  std::sort(launches.begin(), launches.end(), [](const Launch& x, const Launch& y) { return x.work > y.work; });
  // capacities, grids (HBM matrix slices: one per launched wave, at most 1 GiB per bin)
  size_t zoff = 0;
  for (Launch& L : launches) {
    const int b = L.bk * 3 + L.cls;
    R2AArgs& a = L.a;
    a = R2AArgs{};
    a.tasks = dev_tasks, a.qpool = dev_qpool, a.list = lists + L.off, a.n = L.n;
    a.max_ops = max_ops, a.max_md = max_md, a.out = dev_out, a.cigar = dev_cigar, a.md = dev_md;
    // the issue of this field: a producer's count that stays on the device.  Here it is the table word
    // the host has just read into a.n, so min(a.n, *dev_n) = a.n; but the running bins now read the
    // table, which the next call zeroes: one more reason why r2d_done orders the calls
    a.dev_n = d_tab + 4 * b;
    a.lds_per_wave = r2_lds_per_wave(h[4 * b + 1], h[4 * b + 2], L.cls, &a.qcap, &a.rcap, &a.ocap);
    L.wpb = L.cls == 1 ? 1 : 4;  // LDS-heavy bins: one wave per workgroup packs LDS finer
    // every job fits a workgroup on its own (r2_classify); the longest query and
    // the longest window of a bin may come from two jobs and fit only fewer waves
    while ((size_t)L.wpb * a.lds_per_wave > (size_t)kR2LdsPerBlock && L.wpb > 1) L.wpb >>= 1;
    if ((size_t)L.wpb * a.lds_per_wave > (size_t)kR2LdsPerBlock)
      return fail(ctx, BWAGPU_E_DEVICE, "reg2aln bin needs more LDS than a workgroup has");
    a.zstride = L.cls == 2 ? (((int64_t)h[4 * b + 3] + 255) & ~(int64_t)255) : 0;
    L.waves = r2_resident_waves(kR2CD[L.bk], (size_t)L.wpb * a.lds_per_wave, L.wpb);
    if (L.cls == 2) {
      L.waves = (int)std::min<int64_t>(L.waves, std::max<int64_t>(4, ((int64_t)1 << 30) / a.zstride));
      zoff += (size_t)a.zstride * L.waves;
    }
  }
  uint8_t* z = nullptr;
  HIPC(ctx->r2d_z.get(z, std::max<size_t>(zoff, 256)), "hipMalloc(reg2aln matrices)");  // idle: see the wait above
  if (at) HIPC(launch_reg2aln_scatter(n_cap, keys, off, d_tab + kR2TabWords, lists, st), "reg2aln scatter launch");
  if (timing) HIPC(hipEventRecord(ctx->r2d_ev[0], st), "event");
  if (!launches.empty()) {
    int used = 0;
    TRY(side_fork(ctx, st, launches.size(), &used));
    zoff = 0;
    for (size_t li = 0; li < launches.size(); ++li) {
      Launch& L = launches[li];
      if (L.cls == 2) {
        L.a.zglob = z + zoff;
        zoff += (size_t)L.a.zstride * L.waves;
      }
      const int blocks = std::max(1, std::min((L.n + L.wpb - 1) / L.wpb, L.waves / L.wpb));
      HIPC(launch_reg2aln(kR2CD[L.bk], o, ctx->ref, L.a, blocks, L.wpb, ctx->a2_st[li % used]), "reg2aln launch");
    }
    TRY(side_join(ctx, st, used));
  }
  if (timing) {
    HIPC(hipEventRecord(ctx->r2d_ev[1], st), "event");
    ctx->r2d_timed = true;
    ctx->r2d_jobs = h[kR2TabJobs];
    ctx->r2d_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
  }
  // as bwagpu_mate_rescue_device: zeros (nothing moved, no kernel timed: the bins are still running)
  // but the count.  Refused jobs are counted by their status.
  bwagpu_stats_t& last = ctx->slot[0].last = bwagpu_stats_t{};
  last.ext_calls = h[kR2TabJobs];
  return BWAGPU_OK;
}

int bwagpu_debug_reg2aln_times(bwagpu_ctx_t* ctx, double* out) {
  if (!ctx || !out) return BWAGPU_E_INVAL;
  out[0] = out[1] = out[2] = out[3] = 0;
  ctx->r2d_timing = true;  // from the first use on, the device-form calls of this context are timed
  if (!ctx->r2d_timed) return BWAGPU_OK;
  HIPC(hipSetDevice(ctx->device), "hipSetDevice");
  HIPC(hipEventSynchronize(ctx->r2d_ev[1]), "event sync");
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, ctx->r2d_ev[0], ctx->r2d_ev[1]), "event time");
  out[0] = ctx->r2d_wait_ms, out[1] = ms, out[2] = ctx->r2d_call_ms, out[3] = ctx->r2d_jobs;
  return BWAGPU_OK;
}

int bwagpu_reg2aln_jobs_device(bwagpu_ctx_t* ctx, int32_t n_reads, const int64_t* dev_reg_off,
                               const bwagpu_alnreg_t* dev_regs, const int32_t* dev_n, const int32_t* dev_select,
                               const int64_t* dev_seq_off, int32_t job_cap, bwagpu_reg2aln_task_t* dev_tasks,
                               int32_t* dev_job_of, int32_t* dev_n_jobs, void* stream) {
  if (!ctx || n_reads < 0 || job_cap < 0 || !dev_n_jobs || (job_cap && !dev_tasks) ||
      (n_reads && (!dev_reg_off || !dev_regs || !dev_n || !dev_select || !dev_seq_off || !dev_job_of)))
    return BWAGPU_E_INVAL;
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  if (n_reads == 0) {
    HIPC(hipMemsetAsync(dev_n_jobs, 0, 2 * sizeof(int32_t), st), "memset");
    return BWAGPU_OK;
  }
  const size_t n_sums = ((size_t)n_reads + 255) / 256, sum_bytes = sizeof(int32_t) * n_sums;
  if (!ctx->r2d_done) HIPC(hipEventCreateWithFlags(&ctx->r2d_done, hipEventDisableTiming), "event");
  if (ctx->r2d_pending && sum_bytes > ctx->r2d_sums.cap) HIPC(hipEventSynchronize(ctx->r2d_done), "event sync");
  if (ctx->r2d_pending) HIPC(hipStreamWaitEvent(st, ctx->r2d_done, 0), "stream wait");
  int32_t* sums = nullptr;
  HIPC(ctx->r2d_sums.get(sums, n_sums), "hipMalloc");
  const hipError_t e = launch_reg2aln_jobs(n_reads, dev_reg_off, dev_regs, dev_n, dev_select, dev_seq_off, job_cap,
                                           dev_tasks, dev_job_of, dev_n_jobs, sums, st);
  if (hipEventRecord(ctx->r2d_done, st) == hipSuccess) ctx->r2d_pending = true;
  HIPC(e, "reg2aln jobs launch");
  return BWAGPU_OK;
}

int bwagpu_xa_select_device(bwagpu_ctx_t* ctx, const bwagpu_samopt_t* xopt, int32_t n_reads,
                            const int64_t* dev_reg_off, const bwagpu_alnreg_t* dev_regs, const int32_t* dev_n,
                            const bwagpu_pairsel_t* dev_sel, const int32_t* dev_out_mapq, int32_t* dev_xa_of,
                            int32_t* dev_job_select, void* stream) {
  if (!ctx) return BWAGPU_E_INVAL;
  if (!xopt) return fail(ctx, BWAGPU_E_INVAL, "NULL bwagpu_samopt_t");
  const char* why = "";
  if (int rc = sel_flags_check(xopt->flags, &why)) return fail(ctx, rc, why);
  if (n_reads < 0) return fail(ctx, BWAGPU_E_INVAL, "negative read count");
  if (n_reads & 1) return fail(ctx, BWAGPU_E_INVAL, "odd read count: reads 2i and 2i+1 are a pair");
  if (n_reads == 0) return BWAGPU_OK;
  if (!dev_reg_off || !dev_regs || !dev_n || !dev_sel || !dev_out_mapq || !dev_xa_of || !dev_job_select)
    return fail(ctx, BWAGPU_E_INVAL, "NULL array");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  XaSelArgs a{};
  a.n_reads = n_reads, a.max_hits = xopt->max_XA_hits, a.max_hits_alt = xopt->max_XA_hits_alt;
  a.drop_ratio = xopt->XA_drop_ratio;  // float -> double, as get_pri_idx's caller passes it
  a.reg_off = dev_reg_off, a.regs = dev_regs, a.n = dev_n, a.sel = dev_sel, a.out_mapq = dev_out_mapq;
  a.xa_of = dev_xa_of, a.job_select = dev_job_select;
  HIPC(launch_xa_select(a, st), "xa_select launch");
  return BWAGPU_OK;
}

namespace {

// the argument checks of bwagpu_sam_text_device -> BWAGPU_OK with *rg_len, or the code with *why
int sam_text_check(const bwagpu_samtext_t* t, int32_t n_reads, int32_t* rg_len, const char** why) {
  if (!t) return *why = "NULL bwagpu_samtext_t", BWAGPU_E_INVAL;
  if (int rc = sel_flags_check(t->flags, why)) return rc;
  if (t->flags & BWAGPU_MEM_F_REF_HDR) return *why = "MEM_F_REF_HDR is not implemented", BWAGPU_E_UNSUPPORTED;
  if (n_reads < 0) return *why = "negative read count", BWAGPU_E_INVAL;
  if (n_reads & 1) return *why = "odd read count: reads 2i and 2i+1 are a pair", BWAGPU_E_INVAL;
  if (t->text_cap < 0 || t->n_contigs < 0 || t->job_cap < 0) return *why = "negative capacity", BWAGPU_E_INVAL;
  if (t->max_ops < 1 || t->max_md < 1) return *why = "max_ops and max_md must be at least 1", BWAGPU_E_INVAL;
  *rg_len = 0;
  if (t->rg_id) {
    const size_t l = strnlen(t->rg_id, BWAGPU_SAM_MAX_RG + 1);
    if (l > BWAGPU_SAM_MAX_RG) return *why = "rg_id is longer than BWAGPU_SAM_MAX_RG", BWAGPU_E_INVAL;
    *rg_len = (int32_t)l;
  }
  if (!t->dev_text_off || !t->dev_text_n || (t->text_cap && !t->dev_text))
    return *why = "NULL output array", BWAGPU_E_INVAL;
  if (n_reads &&
      (!t->dev_reg_off || !t->dev_regs || !t->dev_n || !t->dev_sel || !t->dev_out_mapq || !t->dev_xa_of ||
       !t->dev_job_of || !t->dev_aln || !t->dev_cigar || !t->dev_md || !t->dev_seq_off || !t->dev_seq ||
       !t->dev_name_off || !t->dev_names || !t->dev_contig_off || !t->dev_contig_names || !t->dev_status ||
       (t->dev_comment_off && !t->dev_comments)))
    return *why = "NULL array", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// the scratch of bwagpu_sam_text_device on st, behind every earlier user of it
int sam_text_scratch(bwagpu_ctx_t* ctx, int32_t n_reads, hipStream_t st, void** scratch) {
  const size_t bytes = sam_text_scratch_bytes(n_reads);
  if (!ctx->r2d_done) HIPC(hipEventCreateWithFlags(&ctx->r2d_done, hipEventDisableTiming), "event");
  if (ctx->r2d_pending && bytes > ctx->sam_scratch.cap) HIPC(hipEventSynchronize(ctx->r2d_done), "event sync");
  if (ctx->r2d_pending) HIPC(hipStreamWaitEvent(st, ctx->r2d_done, 0), "stream wait");
  HIPC(ctx->sam_scratch.ensure(bytes), "hipMalloc");
  *scratch = ctx->sam_scratch.p;
  return BWAGPU_OK;
}

}  // namespace

int bwagpu_sam_text_device(bwagpu_ctx_t* ctx, const bwagpu_samtext_t* t, int32_t n_reads, void* stream) {
  if (!ctx) return BWAGPU_E_INVAL;
  const char* why = "";
  int32_t rg_len = 0;
  if (int rc = sam_text_check(t, n_reads, &rg_len, &why)) return fail(ctx, rc, why);
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  if (n_reads == 0) {
    HIPC(hipMemsetAsync(t->dev_text_off, 0, sizeof(int64_t), st), "memset");
    HIPC(hipMemsetAsync(t->dev_text_n, 0, 2 * sizeof(int64_t), st), "memset");
    return BWAGPU_OK;
  }
  void* scratch = nullptr;
  TRY(sam_text_scratch(ctx, n_reads, st, &scratch));
  SamRgBytes rg{};
  if (rg_len) memcpy(rg.c, t->rg_id, (size_t)rg_len);
  const hipError_t e = launch_sam_text(*t, n_reads, rg, rg_len, scratch, st);
  if (hipEventRecord(ctx->r2d_done, st) == hipSuccess) ctx->r2d_pending = true;
  HIPC(e, "sam_text launch");
  return BWAGPU_OK;
}

// one step of bwagpu_sam_text_device alone (0 count, 1 scan, 2 write), for tools_dev/sam_text_bench.py;
// the steps of one call share the context's scratch, so they run in order on one stream
int bwagpu_debug_sam_text_step(bwagpu_ctx_t* ctx, const bwagpu_samtext_t* t, int32_t n_reads, int32_t step,
                               void* stream) {
  if (!ctx || step < 0 || step > 2) return BWAGPU_E_INVAL;
  const char* why = "";
  int32_t rg_len = 0;
  if (int rc = sam_text_check(t, n_reads, &rg_len, &why)) return fail(ctx, rc, why);
  if (n_reads == 0) return fail(ctx, BWAGPU_E_INVAL, "no reads");
  hipStream_t st = nullptr;
  TRY(entry_stream(ctx, stream, &st));
  void* scratch = nullptr;
  TRY(sam_text_scratch(ctx, n_reads, st, &scratch));
  SamRgBytes rg{};
  if (rg_len) memcpy(rg.c, t->rg_id, (size_t)rg_len);
  const hipError_t e = launch_sam_text_step(step, *t, n_reads, rg, rg_len, scratch, st);
  if (hipEventRecord(ctx->r2d_done, st) == hipSuccess) ctx->r2d_pending = true;
  HIPC(e, "sam_text step launch");
  return BWAGPU_OK;
}

int bwagpu_align2_batch(bwagpu_ctx_t* ctx, int32_t n, const bwagpu_align2_task_t* tasks, const uint8_t* qpool,
                        int64_t qpool_len, const uint8_t* tpool, int64_t tpool_len, bwagpu_kswr_t* results) {
  if (!ctx) return BWAGPU_E_INVAL;
  Align2Plan plan;
  const char* why = "";
  if (int rc = align2_plan(ctx->opt, n, tasks, qpool, qpool_len, tpool, tpool_len, results, &plan, &why))
    return refuse(ctx, rc, why);
  if (n == 0) return BWAGPU_OK;
  HostCall h(ctx);
  TRY(h.begin());
  hipStream_t st = h.st;
  TRY(h.up(ctx->a2_tasks, tasks, sizeof(bwagpu_align2_task_t) * n));
  TRY(h.up(ctx->a2_q, qpool, (size_t)qpool_len, 1));
  TRY(h.up(ctx->a2_t, tpool, (size_t)tpool_len, 1));
  bwagpu_kswr_t* out = nullptr;
  int2* scratch = nullptr;
  int32_t* lists = nullptr;
  int64_t* boff = nullptr;
  TRY(h.reserve(ctx->a2_out, out, (size_t)n));
  TRY(h.reserve(ctx->a2_scratch, scratch, (size_t)plan.scratch));
  TRY(h.reserve(ctx->a2_lists, lists, (size_t)n));
  // counts[kA2Bins] | cursors[kA2Bins] | stats[ST_N]
  TRY(h.reserve(ctx->a2_counts, sizeof(int32_t) * 2 * kA2Bins + sizeof(int64_t) * ST_N));
  TRY(h.reserve(ctx->a2_boff, boff, (size_t)n));
  int32_t* d_counts = ctx->a2_counts.as<int32_t>();
  int64_t* d_stats = (int64_t*)(d_counts + 2 * kA2Bins);
  HIPC(hipMemcpyAsync(lists, plan.all.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st), "H2D");
  HIPC(hipMemcpyAsync(d_counts, plan.counts, sizeof plan.counts, hipMemcpyHostToDevice, st), "H2D");  // + zero cursors
  HIPC(hipMemsetAsync(d_stats, 0, sizeof(int64_t) * ST_N, st), "memset");
  HIPC(hipMemcpyAsync(boff, plan.boff.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st), "H2D");
  TRY(h.start());
  const A2Args base{ctx->a2_tasks.as<bwagpu_align2_task_t>(), ctx->a2_q.as<uint8_t>(), ctx->a2_t.as<uint8_t>(), out,
                    scratch, boff, lists, nullptr, nullptr, d_stats};
  TRY(launch_align2_concurrent(ctx, st, plan.bins, base, plan.list_off, plan.counts, d_counts, d_counts + kA2Bins, 0));
  TRY(h.stop());
  TRY(h.down(results, ctx->a2_out, sizeof(bwagpu_kswr_t) * n));
  return h.finish("align2 batch", d_stats);
}

int bwagpu_align2_device(bwagpu_ctx_t* ctx, int32_t n, const bwagpu_align2_task_t* dev_tasks,
                         const uint8_t* dev_qpool, const uint8_t* dev_tpool, bwagpu_kswr_t* dev_results,
                         void* dev_scratch, void* stream) {
  if (!ctx || n < 0 || (n && (!dev_tasks || !dev_results || !dev_scratch))) return BWAGPU_E_INVAL;
  if (n == 0) return BWAGPU_OK;
  if (const char* why = align2_opt_unsupported(ctx->opt)) return fail(ctx, BWAGPU_E_UNSUPPORTED, why);
  hipStream_t st = nullptr;
  if (int rc = entry_stream(ctx, stream, &st)) return rc;
  int32_t* lists = nullptr;
  int64_t* boff = nullptr;
  HIPC(ctx->a2_lists.get(lists, (size_t)kA2Bins * n), "hipMalloc");
  HIPC(ctx->a2_boff.get(boff, (size_t)n), "hipMalloc");
  // counts[kA2Bins] | cursors[kA2Bins] | scratch cursor (u64) | stats[ST_N]
  const size_t cbytes = sizeof(int32_t) * 2 * kA2Bins + sizeof(int64_t) * (1 + ST_N);
  HIPC(ctx->a2_counts.ensure(cbytes), "hipMalloc");
  int32_t* d_counts = ctx->a2_counts.as<int32_t>();
  unsigned long long* cursor = (unsigned long long*)(d_counts + 2 * kA2Bins);
  int64_t* d_stats = (int64_t*)(cursor + 1);
  HIPC(hipMemsetAsync(d_counts, 0, cbytes, st), "memset");
  HIPC(launch_align2_bins(ctx->opt, dev_tasks, n, lists, d_counts, boff, cursor, dev_results, d_stats, st),
       "align2 bin launch");
  // counts are on the device only: every bin's kernel is launched with a
  // resident-capacity grid; an empty bin's waves exit on their first claim
  const std::vector<int> bins{2, 3, 10, 11, 1, 9, 0, 8, 4, 12, 5, 13, 6, 14, 7, 15};
  A2Args base{dev_tasks, dev_qpool, dev_tpool, dev_results, (int2*)dev_scratch, boff, lists, nullptr, nullptr, d_stats};
  return launch_align2_concurrent(ctx, st, bins, base, nullptr, nullptr, d_counts, d_counts + kA2Bins, (size_t)n);
}

// The FPGA back end's own job (sw_top, xlnx/XCLAgent.cpp:89-106) on its wire
// format: the host walks the record chain and checks lengths (stream_plan);
// the device decodes and checks everything else (stream_decode_kernel) and
// extends every task (stream_ext_kernel).  Device-found problems come back as
// BWAGPU_E_RESULTS, the fpgaResultsError of processOutput's checks
// (FPGAPipeline.cpp:38-74).
int bwagpu_sw_stream(bwagpu_ctx_t* ctx, const int32_t* i_buf, int64_t i_words, int16_t* o_buf, int32_t o_cap_tasks,
                     int32_t* o_tasks) {
  if (!ctx || !o_tasks || i_words < 0 || o_cap_tasks < 0 || (i_words && !i_buf) || (o_cap_tasks && !o_buf))
    return BWAGPU_E_INVAL;
  *o_tasks = 0;
  if (i_words == 0) return BWAGPU_OK;
  StreamPlan plan;
  const char* why = "";
  if (int rc = stream_plan(i_buf, i_words, &plan, &why)) return refuse(ctx, rc, why);
  const int tb = tb_bytes_for(ctx->opt, plan.lq_max);
  if ((size_t)(kBlock / 64) * 2 * tb > 64 * 1024)
    return fail(ctx, BWAGPU_E_UNSUPPORTED, "LDS row buffer too large for these options (w, pen_clip, read length)");
  int32_t c[8];
  HostCall h(ctx);
  TRY(h.begin());
  hipStream_t st = h.st;
  const size_t cap = (size_t)std::max(o_cap_tasks, 1), nr = plan.starts.size();
  TRY(h.up(ctx->st_buf, i_buf, sizeof(int32_t) * (size_t)i_words));
  StreamArgs a{};
  TRY(h.reserve(ctx->st_start, a.rstart, nr));
  TRY(h.reserve(ctx->st_q, a.qpool, 8 * (size_t)i_words));
  TRY(h.reserve(ctx->st_tasks, a.tasks, cap));
  TRY(h.reserve(ctx->st_lists, a.lists, kSpecBins * cap));
  TRY(h.reserve(ctx->st_seen, a.seen, cap));
  TRY(h.reserve(ctx->st_ctr, a.ctr, kStrCtrWords));
  TRY(h.reserve(ctx->st_out, a.out, 5 * cap));
  HIPC(hipMemcpyAsync(ctx->st_start.p, plan.starts.data(), sizeof(int64_t) * nr, hipMemcpyHostToDevice, st), "H2D");
  HIPC(hipMemsetAsync(a.seen, 0, sizeof(int32_t) * cap, st), "memset");
  HIPC(hipMemsetAsync(a.ctr, 0, sizeof(int32_t) * kStrCtrWords, st), "memset");
  a.buf = ctx->st_buf.as<int32_t>(), a.n_reads = (int32_t)nr;
  a.cap = o_cap_tasks, a.l_pac = ctx->ref.l_pac;  // cap 0: every task index is then out of range
  TRY(h.start());
  HIPC(launch_sw_stream(ctx->opt, ctx->ref, a, tb, st), "sw_stream launch");
  TRY(h.stop());
  HIPC(hipMemcpyAsync(c, ctx->st_ctr.p, sizeof c, hipMemcpyDeviceToHost, st), "D2H");
  HIPC(hipStreamSynchronize(st), "sync");  // the counters say how many records come back
  if (c[kStrErr]) {
    const int e = c[kStrErr];
    return fail(ctx, BWAGPU_E_RESULTS,
                std::string("stream: ") + (e & STR_ERR_RECORD ? "a record does not end at its end word; " : "") +
                    (e & STR_ERR_TASK ? "task index out of range; " : "") +
                    (e & STR_ERR_DUP ? "task index repeated; " : "") +
                    (e & STR_ERR_SEED ? "seed outside its read or window; " : "") +
                    (e & STR_ERR_BASE ? "base > 4; " : ""));
  }
  if (c[kStrDecoded] != c[kStrMax]) return fail(ctx, BWAGPU_E_RESULTS, "stream: task indices are not 0..n-1");
  const int32_t n = c[kStrMax];
  TRY(h.down(o_buf, ctx->st_out, sizeof(int32_t) * 5 * (size_t)n));
  TRY(h.finish("sync"));
  *o_tasks = n;
  return BWAGPU_OK;
}

}  // extern "C"
