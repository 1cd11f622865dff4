// seed_host.h — host-side checks, staging copy and tables of the seeding and
// chaining entries (capi_seed.hip: bwagpu_set_bwt, bwagpu_collect_intv,
// bwagpu_seqs2chains, bwagpu_seqs2regions).  Plain C++: compiles without HIP,
// so that the passes run under the host sanitizers
// (tests/cpp/batch_host_asan.cpp).
//
// Every *_check returns BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED
// with *why set.  The read checks read seq_off[0 .. n_reads] and
// seq[0 .. seq_off[n_reads]) and write nothing beyond the same number of
// bytes of the destination; the bwt checks read the header's fields only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bwagpu.h"
#include "host_pool.h"

namespace bwagpu {

// bwagpu_set_bwt: the occurrence array covers every position (16 words per 128 positions)
inline int bwt_header_check(const bwagpu_bwt_t* bwt, const char** why) {
  if (bwt->bwt_size < ((bwt->seq_len + 127) >> 7) * 16 || bwt->L2[4] != bwt->seq_len || bwt->primary > bwt->seq_len)
    return *why = "bwt header inconsistent with its occurrence array", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// ... and its sampled suffix array: a power-of-two interval, one entry per interval
inline int bwt_sa_check(const bwagpu_bwt_t* bwt, const char** why) {
  const int iv = bwt->sa_intv;
  if (iv < 1 || (iv & (iv - 1)) || bwt->n_sa < bwt->seq_len / (uint64_t)iv + 1)
    return *why = "suffix array sample interval / size inconsistent", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// a seeding batch's options and extent: *nb = its bases (0 for an empty batch, which reads nothing)
inline int seed_batch_check(const bwagpu_seedopt_t* opt, int32_t n_reads, const int64_t* seq_off, const uint8_t* seq,
                            int64_t* nb, const char** why) {
  *nb = 0;
  if (opt->min_seed_len < 1 || opt->split_width < 0) return *why = "bad seeding options", BWAGPU_E_INVAL;
  if (n_reads == 0) return BWAGPU_OK;
  *nb = seq_off[n_reads] - seq_off[0];
  if (seq_off[0] != 0 || *nb < 0 || (*nb && !seq)) return *why = "seq_off must start at 0", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// The reads of a batch that passed seed_batch_check (n_reads > 0): the read
// lengths and every base (nt4: 0..4), on up to 8 threads for a batch of
// megabases.  dst (optional, sizeof(int64_t) * (n_reads + 1) + nb bytes): the
// same pass also copies seq_off, then the bases, there.  *lq_max = the longest read.
inline int seed_reads_check(int32_t n_reads, const int64_t* seq_off, const uint8_t* seq, int64_t nb, char* dst,
                            int* lq_max, const char** why) {
  const size_t ob = sizeof(int64_t) * ((size_t)n_reads + 1);
  // one thread takes ~1 ms per 10 Mbases
  const int nt = nb >= (1 << 22) ? 8 : 1;
  int len_bad[8] = {}, base_bad[8] = {};
  int64_t lms[8] = {};
  auto part = [&](int t) {
    int64_t lm = 0;
    for (int32_t r = (int32_t)((int64_t)n_reads * t / nt); r < (int32_t)((int64_t)n_reads * (t + 1) / nt); ++r) {
      const int64_t l = seq_off[r + 1] - seq_off[r];
      if (l < 0) len_bad[t] |= 1;
      if (l > BWAGPU_MAX_SEED_READ) len_bad[t] |= 2;
      lm = std::max(lm, l);
    }
    lms[t] = lm;
    if (dst && t == 0) memcpy(dst, seq_off, ob);
    // eight bytes at a time: (b & 0x7f) + 0x7b carries into bit 7 iff b > 4
    int64_t i = (nb * t / nt) & ~(int64_t)7;
    const int64_t e = t == nt - 1 ? nb : (nb * (t + 1) / nt) & ~(int64_t)7;
    uint64_t bad = 0;
    char* const out = dst ? dst + ob : nullptr;
    for (; i + 8 <= e; i += 8) {
      uint64_t w;
      memcpy(&w, seq + i, 8);
      bad |= (((w & 0x7f7f7f7f7f7f7f7fULL) + 0x7b7b7b7b7b7b7b7bULL) | w) & 0x8080808080808080ULL;
      if (out) memcpy(out + i, &w, 8);
    }
    for (; i < e; ++i) {
      bad |= seq[i] > 4;
      if (out) out[i] = (char)seq[i];
    }
    base_bad[t] = bad != 0;
  };
  host_parallel(nt, part);
  int lb = 0, bb = 0;
  int64_t lm = 0;
  for (int t = 0; t < nt; ++t) {
    lb |= len_bad[t];
    bb |= base_bad[t];
    lm = std::max(lm, lms[t]);
  }
  if (lb & 1) return *why = "seq_off not monotone", BWAGPU_E_INVAL;
  if (lb & 2) return *why = "read longer than BWAGPU_MAX_SEED_READ", BWAGPU_E_UNSUPPORTED;
  if (bb) return *why = "read base > 4 (bases are nt4)", BWAGPU_E_INVAL;
  *lq_max = (int)lm;
  return BWAGPU_OK;
}

inline int chain_opt_check(const bwagpu_chainopt_t* copt, const char** why) {
  if (copt->max_occ < 1 || copt->max_chain_gap < 0 || copt->max_chain_extend < 0 || !(copt->mask_level >= 0) ||
      !(copt->drop_ratio >= 0))
    return *why = "bad chaining options", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// mem_flt_chained_seeds' gate and min_HSP_score per read length
// (bwamem.c:609-611), in the host's double arithmetic: tab[l] for l in
// 0 .. lq_max, -1 where a read of that length is not realigned (a = the match
// score).  -> some read of the batch (validated, none longer than lq_max) is.
inline bool seed_sw_table(const bwagpu_chainopt_t* copt, int a, int min_seed_len, int32_t n_reads,
                          const int64_t* seq_off, int lq_max, std::vector<int32_t>* tab) {
  tab->assign((size_t)lq_max + 1, -1);
  bool any_sw = false;
  std::vector<char> has((size_t)lq_max + 1, 0);
  for (int32_t r = 0; r < n_reads; ++r) has[(size_t)(seq_off[r + 1] - seq_off[r])] = 1;
  for (int l = 1; l <= lq_max; ++l) {
    const double min_l = copt->min_chain_weight ? 1.1f * copt->min_chain_weight : 5.5f * log((double)l);
    if (min_l > 0.05f * l) continue;
    (*tab)[(size_t)l] = (int)(a * min_l + .499);
    any_sw = any_sw || (has[(size_t)l] && l >= min_seed_len);
  }
  return any_sw;
}

}  // namespace bwagpu
