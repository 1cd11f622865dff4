// task_host.h — host-side validation, binning and launch planning of the
// entries that take a list of tasks or a wire stream (capi_tasks.hip).  Plain
// C++: compiles without HIP, so that the plans run under the host sanitizers
// (tests/cpp/task_host_asan.cpp).  Every *_plan returns BWAGPU_OK, or
// BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED with *why set ("" for a bad argument,
// which has no text), and reads nothing beyond tasks[n - 1], the pools'
// lengths and i_buf[i_words - 1].  The first failing task in task order wins;
// the pools' bases are looked at after all tasks.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "bwagpu.h"
#include "pure.h"

namespace bwagpu {

// [off, off + len) lies in a pool of pool_len entries (off, len >= 0 checked by the caller)
inline bool in_pool(int64_t off, int64_t len, int64_t pool_len) { return off <= pool_len - len; }

inline int pool_bases_check(const uint8_t* qpool, int64_t qpool_len, const uint8_t* tpool, int64_t tpool_len,
                            const char** why) {
  for (int64_t i = 0; i < qpool_len; ++i)
    if (qpool[i] > 4) return *why = "query base > 4", BWAGPU_E_INVAL;
  for (int64_t i = 0; i < tpool_len; ++i)
    if (tpool[i] > 4) return *why = "target base > 4", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// ------------------------------------------------------------ bwagpu_extend_batch
// lists: the wave kernels by column segments (kExtVariants), then the
// four-per-wave kernel (packed 16-bit DP) for the tasks it takes (extend4_kernel)
constexpr int kExtLists = kNumExtVariants + 1;
struct ExtendPlan {
  std::vector<int32_t> all;  // the lists, one after the other
  int32_t count[kExtLists] = {}, off[kExtLists] = {};
  int tb[kExtLists] = {};    // LDS row-buffer bytes per group of each list's launch
  bool t5 = false;           // some target base is an N
};

inline int extend_plan(const DevOpt& o, bool quad, int32_t n, const bwagpu_ext_task_t* tasks, const uint8_t* qpool,
                       int64_t qpool_len, const uint8_t* tpool, int64_t tpool_len, const bwagpu_ext_result_t* results,
                       ExtendPlan* plan, const char** why) {
  *plan = ExtendPlan{};
  *why = "";
  if (n < 0 || (n && (!tasks || !results)) || qpool_len < 0 || tpool_len < 0 || (qpool_len && !qpool) ||
      (tpool_len && !tpool))
    return BWAGPU_E_INVAL;
  if (n == 0) return BWAGPU_OK;
  const int max_q = kExtVariants[kNumExtVariants - 1].max_len();  // qlen + 1 columns
  std::vector<int32_t> lists[kExtLists];
  for (int32_t k = 0; k < n; ++k) {
    const bwagpu_ext_task_t& t = tasks[k];
    if (t.qlen < 0 || t.tlen < 0 || t.qoff < 0 || t.toff < 0 || !in_pool(t.qoff, t.qlen, qpool_len) ||
        !in_pool(t.toff, t.tlen, tpool_len) || t.w < 0)
      return *why = "task outside its pools", BWAGPU_E_INVAL;
    if (t.qlen >= max_q) return *why = "qlen too long", BWAGPU_E_UNSUPPORTED;
    if (!wave_bound_ok(t.h0 + (long)t.qlen * o.max_mat))
      return *why = "h0 + qlen * max score >= 2^21: over the 32-bit kernels' row-max key", BWAGPU_E_UNSUPPORTED;
    int v = kNumExtVariants - 1;
    for (int i = kNumExtVariants - 1; i >= 0; --i)
      if (t.qlen + 1 <= kExtVariants[i].max_len()) v = i;
    if (quad && t.h0 > 0 && t.qlen >= 1 && t.qlen + 1 <= 256 && quad_bound_ok(o, t.h0 + (long)t.qlen * o.max_mat) &&
        quad_rows_ok(o, t.tlen)) {
      bool nt = true;  // no N in the target rows
      for (int64_t i = t.toff; i < t.toff + t.tlen && nt; ++i) nt = tpool[i] <= 3;
      if (nt) v = kNumExtVariants;
    }
    lists[v].push_back(k);
  }
  for (int64_t i = 0; i < tpool_len && !plan->t5; ++i) plan->t5 = tpool[i] > 3;
  if (int rc = pool_bases_check(qpool, qpool_len, tpool, tpool_len, why)) return rc;
  plan->all.reserve((size_t)n);
  for (int v = 0; v < kExtLists; ++v) {
    plan->off[v] = (int32_t)plan->all.size();
    plan->count[v] = (int32_t)lists[v].size();
    plan->all.insert(plan->all.end(), lists[v].begin(), lists[v].end());
    if (lists[v].empty()) continue;
    int rows = 16;  // LDS rows needed per task (rows_needed on the host) -> the list's max
    for (int32_t k : lists[v]) {
      const bwagpu_ext_task_t& t = tasks[k];
      if (t.tlen <= rows) continue;  // min(tlen, ..) cannot raise the maximum
      const int mi = band_cap(t.qlen, o.max_mat, t.end_bonus, o.o_ins, o.e_ins);
      const int md = band_cap(t.qlen, o.max_mat, t.end_bonus, o.o_del, o.e_del);
      const int we = std::min(t.w, std::min(mi, md));
      rows = std::max(rows, std::min(t.tlen, t.qlen + we + 1));
    }
    plan->tb[v] = (rows + 2 + 15) & ~15;
    const int gpb = v < kNumExtVariants ? kBlock / kExtVariants[v].G : 2 * kBlock / 32;
    if ((size_t)plan->tb[v] * gpb > 64 * 1024) return *why = "task needs too many LDS rows", BWAGPU_E_UNSUPPORTED;
  }
  return BWAGPU_OK;
}

// ------------------------------------------------------------ bwagpu_align2_batch
struct Align2Plan {
  std::vector<int32_t> all;   // the bins' lists, longest target first inside a bin (rows ~ tlen)
  std::vector<int64_t> boff;  // per task: its first row-maximum entry in the scratch
  int64_t scratch = 0;        // row-maximum entries of all tasks (tlen + 1 each)
  int32_t counts[2 * kA2Bins] = {};  // per bin, then the bins' zeroed cursors
  int32_t list_off[kA2Bins] = {};
  std::vector<int> bins;      // non-empty bins by total rows x columns per lane, largest first
};

inline int align2_plan(const DevOpt& o, int32_t n, const bwagpu_align2_task_t* tasks, const uint8_t* qpool,
                       int64_t qpool_len, const uint8_t* tpool, int64_t tpool_len, const bwagpu_kswr_t* results,
                       Align2Plan* plan, const char** why) {
  *plan = Align2Plan{};
  *why = "";
  if (n < 0 || (n && (!tasks || !results)) || qpool_len < 0 || tpool_len < 0 || (qpool_len && !qpool) ||
      (tpool_len && !tpool))
    return BWAGPU_E_INVAL;
  if (n == 0) return BWAGPU_OK;
  if (const char* w = align2_opt_unsupported(o)) return *why = w, BWAGPU_E_UNSUPPORTED;
  const bool byte_ok = align2_byte_ok(o);
  std::vector<int32_t> lists[kA2Bins];
  plan->boff.resize((size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    const bwagpu_align2_task_t& t = tasks[k];
    if (t.qlen < 0 || t.tlen < 0 || t.qoff < 0 || t.toff < 0 || !in_pool(t.qoff, t.qlen, qpool_len) ||
        !in_pool(t.toff, t.tlen, tpool_len))
      return *why = "task outside its pools", BWAGPU_E_INVAL;
    if (t.qlen > BWAGPU_MAX_READ_LEN) return *why = "qlen > BWAGPU_MAX_READ_LEN", BWAGPU_E_UNSUPPORTED;
    const bool u8 = (t.xtra & BWAGPU_KSW_XBYTE) != 0;
    if (u8 && !byte_ok) return *why = kA2ByteWhy, BWAGPU_E_UNSUPPORTED;  // word tasks of the batch stay admitted
    if (!u8 && !align2_word_fits(t.qlen, o.max_mat))
      return *why = "i16 scores could saturate (qlen * max score > 32767)", BWAGPU_E_UNSUPPORTED;
    lists[a2_bin_of(t.qlen, u8)].push_back(k);
    plan->boff[(size_t)k] = plan->scratch;
    plan->scratch += (int64_t)t.tlen + 1;
  }
  if (int rc = pool_bases_check(qpool, qpool_len, tpool, tpool_len, why)) return rc;
  plan->all.reserve((size_t)n);
  std::vector<std::pair<int64_t, int>> order;
  for (int b = 0; b < kA2Bins; ++b) {
    std::stable_sort(lists[b].begin(), lists[b].end(),
                     [&](int32_t x, int32_t y) { return tasks[x].tlen > tasks[y].tlen; });
    plan->counts[b] = (int32_t)lists[b].size();
    plan->list_off[b] = (int32_t)plan->all.size();
    plan->all.insert(plan->all.end(), lists[b].begin(), lists[b].end());
    int64_t rows = 0;
    for (int32_t k : lists[b]) rows += tasks[k].tlen;
    if (plan->counts[b]) order.push_back({rows * kA2CD[b % kA2Buckets], b});
  }
  std::sort(order.begin(), order.end(),
            [](const std::pair<int64_t, int>& x, const std::pair<int64_t, int>& y) { return x.first > y.first; });
  for (auto& e : order) plan->bins.push_back(e.second);
  return BWAGPU_OK;
}

// --------------------------------------------------------------- bwagpu_sw_stream
// The host walks the record chain (one load per read record — the "end" words
// of packReadData, FPGAPipeline.cpp:258,336) and checks lengths; the device
// decodes and checks everything else.
struct StreamPlan {
  std::vector<int64_t> starts;  // first word of each read record
  int lq_max = 1;
};

inline int stream_plan(const int32_t* i_buf, int64_t i_words, StreamPlan* plan, const char** why) {
  *plan = StreamPlan{};
  *why = "";
  if (i_words < 0 || (i_words && !i_buf)) return BWAGPU_E_INVAL;
  for (int64_t p = 0; p < i_words;) {
    const int64_t end = i_buf[p];
    if (end <= p + 2 || end > i_words) return *why = "stream: a record's end word is out of range", BWAGPU_E_INVAL;
    const int lq = i_buf[p + 1];
    if (lq < 0) return *why = "stream: negative read length", BWAGPU_E_INVAL;
    if (lq > BWAGPU_MAX_READ_LEN) return *why = "stream: read longer than BWAGPU_MAX_READ_LEN", BWAGPU_E_UNSUPPORTED;
    plan->lq_max = std::max(plan->lq_max, lq);
    plan->starts.push_back(p);
    p = end;
  }
  return BWAGPU_OK;
}

}  // namespace bwagpu
