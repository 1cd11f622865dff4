// batch_host.h — host-side validation and staging copy of a chain2aln batch
// (capi.hip: bwagpu_chain2aln_submit, bwagpu_chain2aln_stage).  Plain C++:
// compiles without HIP, so that the passes run under the host sanitizers
// (tests/cpp/batch_host_asan.cpp).
//
// Every check returns BWAGPU_OK, or BWAGPU_E_INVAL / BWAGPU_E_UNSUPPORTED with
// *why set.  check_batch_header reads the dimensions and the first and last
// entry of each offset array.  The passes after it read nothing beyond the
// arrays as the header sizes them (seq_off and read_chain_off n_reads + 1,
// chain_seed_off n_chains + 1, chain_rid and chain_frac_rep n_chains, seeds
// n_seeds, seq seq_bytes) and write nothing beyond InLayout::total bytes.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "bwagpu.h"
#include "host_pool.h"

namespace bwagpu {

// layout of one batch inside a slot's single input allocation
struct InLayout {
  size_t seq_off, seq, rco, cso, rid, frac, seeds, total;
  void make(const bwagpu_batch_t& b) {
    size_t o = 0;
    auto take = [&](size_t n) {
      size_t at = o;
      o += (n + 255) & ~(size_t)255;
      return at;
    };
    seq_off = take(sizeof(int64_t) * (size_t)(b.n_reads + 1));
    rco = take(sizeof(int32_t) * (size_t)(b.n_reads + 1));
    cso = take(sizeof(int32_t) * (size_t)(b.n_chains + 1));
    rid = take(sizeof(int32_t) * (size_t)b.n_chains);
    frac = take(sizeof(float) * (size_t)b.n_chains);
    seeds = take(sizeof(bwagpu_seed_t) * (size_t)b.n_seeds);
    seq = take((size_t)b.seq_bytes);
    total = o;
  }
};

// validate the flattened batch on the host (cheap O(n) checks so that a
// malformed batch is an E_INVAL here, never an out-of-bounds access on device);
// one pass over reads -> chains -> seeds, which also yields the longest read
// the batch's dimensions and array pointers (O(1)): what the staging copy relies on
inline int check_batch_header(const bwagpu_batch_t* b, std::string* why) {
  if (!b) return *why = "batch is NULL", BWAGPU_E_INVAL;
  if (b->n_reads < 0 || b->n_chains < 0 || b->n_seeds < 0 || b->seq_bytes < 0)
    return *why = "negative batch dimension", BWAGPU_E_INVAL;
  if (b->n_reads == 0) return BWAGPU_OK;
  if (!b->seq_off || !b->read_chain_off || !b->chain_seed_off) return *why = "NULL offset array", BWAGPU_E_INVAL;
  if (b->seq_off[0] != 0 || b->seq_off[b->n_reads] != b->seq_bytes)
    return *why = "seq_off does not span seq_bytes", BWAGPU_E_INVAL;
  if (b->read_chain_off[0] != 0 || b->read_chain_off[b->n_reads] != b->n_chains)
    return *why = "read_chain_off does not span n_chains", BWAGPU_E_INVAL;
  if (b->chain_seed_off[0] != 0 || b->chain_seed_off[b->n_chains] != b->n_seeds)
    return *why = "chain_seed_off does not span n_seeds", BWAGPU_E_INVAL;
  if (b->n_chains && (!b->chain_rid || !b->chain_frac_rep)) return *why = "NULL chain array", BWAGPU_E_INVAL;
  if (b->n_seeds && !b->seeds) return *why = "NULL seeds", BWAGPU_E_INVAL;
  if (b->seq_bytes && !b->seq) return *why = "NULL seq", BWAGPU_E_INVAL;
  return BWAGPU_OK;
}

// reads [r0, r1) of a header-checked batch: seq_off and the offsets monotone,
// every read at most BWAGPU_MAX_READ_LEN (*bad_read), every seed inside its
// read and inside [0, 2*l_pac).  -> 0 ok, 1 seq_off, 2 read too long, 3 rco,
// 4 cso, 5 seed; *lmax = the longest read.
inline int check_reads(const bwagpu_batch_t* b, int64_t l_pac, int r0, int r1, int64_t* lmax, int* bad_read) {
  const int64_t two = l_pac << 1;
  const int64_t* so = b->seq_off;
  const int32_t* rco = b->read_chain_off;
  const int32_t* cso = b->chain_seed_off;
  const bwagpu_seed_t* sd = b->seeds;
  int64_t lm = 0;
  for (int r = r0; r < r1; ++r) {
    const int64_t l = so[r + 1] - so[r];
    if (l < 0) return 1;
    if (l > BWAGPU_MAX_READ_LEN) {
      *bad_read = r;
      return 2;
    }
    lm = std::max(lm, l);
    // every offset is range-checked BEFORE it indexes: a range may start
    // anywhere, and a later read's failing check must not come after an
    // earlier read walked past the caller's arrays
    const int c0 = rco[r], c1 = rco[r + 1];
    if (c0 < 0 || c1 < c0 || c1 > b->n_chains) return 3;
    bool bad_seed = false;
    for (int c = c0; c < c1; ++c) {
      const int k0 = cso[c], k1 = cso[c + 1];
      if (k0 < 0 || k1 < k0 || k1 > b->n_seeds) return 4;
      for (int k = k0; k < k1; ++k) {  // branch-free accumulation: one test per read
        const bwagpu_seed_t& s = sd[k];
        bad_seed |= (s.qbeg < 0) | (s.len <= 0) | ((int64_t)s.qbeg + s.len > l) | (s.rbeg < 0) | (s.rbeg + s.len > two);
      }
    }
    if (bad_seed) return 5;
  }
  *lmax = lm;
  return 0;
}

// the first failing range's code as one sequential pass would report it
inline int check_report(const bwagpu_batch_t* b, const int* code, const int* bad_read, int nt, std::string* why) {
  for (int t = 0; t < nt; ++t) {
    switch (code[t]) {
      case 1: return *why = "seq_off not monotone", BWAGPU_E_INVAL;
      case 2: {
        char m[128];
        snprintf(m, sizeof m, "read %d has length %lld > %d", bad_read[t],
                 (long long)(b->seq_off[bad_read[t] + 1] - b->seq_off[bad_read[t]]), BWAGPU_MAX_READ_LEN);
        return *why = m, BWAGPU_E_UNSUPPORTED;
      }
      case 3: return *why = "read_chain_off not monotone", BWAGPU_E_INVAL;
      case 4: return *why = "chain_seed_off not monotone", BWAGPU_E_INVAL;
      case 5: return *why = "seed outside its read or the reference", BWAGPU_E_INVAL;
      default: break;
    }
  }
  return BWAGPU_OK;
}

// every read, chain and seed (O(n), after check_batch_header): the longest read -> *lq_max_out
inline int check_batch_seeds(const bwagpu_batch_t* b, int64_t l_pac, int* lq_max_out, std::string* why) {
  *lq_max_out = 0;
  if (b->n_reads == 0) return BWAGPU_OK;
  const int nt = b->n_seeds >= (1 << 16) ? 4 : 1;
  int code[4] = {0, 0, 0, 0}, bad_read[4] = {0, 0, 0, 0};
  int64_t lmaxs[4] = {0, 0, 0, 0};
  host_parallel(nt, [&](int t) {
    code[t] = check_reads(b, l_pac, (int)((int64_t)b->n_reads * t / nt), (int)((int64_t)b->n_reads * (t + 1) / nt),
                          &lmaxs[t], &bad_read[t]);
  });
  if (int rc = check_report(b, code, bad_read, nt, why)) return rc;
  *lq_max_out = (int)std::max(std::max(lmaxs[0], lmaxs[1]), std::max(lmaxs[2], lmaxs[3]));
  return BWAGPU_OK;
}

// The staging copy and the check in one pass (bwagpu_chain2aln_submit): nt
// threads, each a read range in blocks of 1024 reads — a block's arrays are
// copied into the pinned staging buffer h (layout L), then checked while still
// in cache.  A block's copy ranges come from its boundary offsets, which are
// range-checked first, so a malformed batch never makes the copy leave the
// caller's arrays (sizes from the header); it is refused after the pass.
inline int stage_and_check(const bwagpu_batch_t* b, int64_t l_pac, char* h, const InLayout& L, int* lq_max_out,
                           std::string* why) {
  *lq_max_out = 0;
  const int nr = b->n_reads;
  if (nr == 0) return BWAGPU_OK;
  constexpr int kBlk = 1024, kMaxT = 8;
  const int nt = b->n_seeds >= (1 << 16) ? kMaxT : 1;
  const int nblk = (nr + kBlk - 1) / kBlk;
  int code[kMaxT] = {}, bad_read[kMaxT] = {};
  int64_t lmaxs[kMaxT] = {};
  auto work = [&](int t) {
    // this thread's blocks: [nblk*t/nt, nblk*(t+1)/nt), in order
    for (int k = (int)((int64_t)nblk * t / nt), ke = (int)((int64_t)nblk * (t + 1) / nt); k < ke; ++k) {
      const int r0 = k * kBlk, r1 = std::min(nr, r0 + kBlk);
      const int64_t b0 = b->seq_off[r0], b1 = b->seq_off[r1];
      const int c0 = b->read_chain_off[r0], c1 = b->read_chain_off[r1];
      if (b0 < 0 || b1 < b0 || b1 > b->seq_bytes) {
        code[t] = 1;
        return;
      }
      if (c0 < 0 || c1 < c0 || c1 > b->n_chains) {
        code[t] = 3;
        return;
      }
      const int k0 = b->chain_seed_off[c0], k1 = b->chain_seed_off[c1];
      if (k0 < 0 || k1 < k0 || k1 > b->n_seeds) {
        code[t] = 4;
        return;
      }
      const int re = r1 == nr ? r1 + 1 : r1, ce = c1 == b->n_chains ? c1 + 1 : c1;  // the last block: the end offsets
      memcpy(h + L.seq_off + sizeof(int64_t) * r0, b->seq_off + r0, sizeof(int64_t) * (size_t)(re - r0));
      memcpy(h + L.rco + sizeof(int32_t) * r0, b->read_chain_off + r0, sizeof(int32_t) * (size_t)(re - r0));
      memcpy(h + L.cso + sizeof(int32_t) * c0, b->chain_seed_off + c0, sizeof(int32_t) * (size_t)(ce - c0));
      if (c1 > c0) {
        memcpy(h + L.rid + sizeof(int32_t) * c0, b->chain_rid + c0, sizeof(int32_t) * (size_t)(c1 - c0));
        memcpy(h + L.frac + sizeof(float) * c0, b->chain_frac_rep + c0, sizeof(float) * (size_t)(c1 - c0));
      }
      if (k1 > k0) memcpy(h + L.seeds + sizeof(bwagpu_seed_t) * k0, b->seeds + k0, sizeof(bwagpu_seed_t) * (size_t)(k1 - k0));
      if (b1 > b0) memcpy(h + L.seq + b0, b->seq + b0, (size_t)(b1 - b0));
      int64_t lm = 0;
      if ((code[t] = check_reads(b, l_pac, r0, r1, &lm, &bad_read[t]))) return;
      lmaxs[t] = std::max(lmaxs[t], lm);
    }
  };
  host_parallel(nt, work);
  if (int rc = check_report(b, code, bad_read, nt, why)) return rc;
  int64_t lm = 0;
  for (int t = 0; t < nt; ++t) lm = std::max(lm, lmaxs[t]);
  *lq_max_out = (int)lm;
  return BWAGPU_OK;
}

}  // namespace bwagpu
