// samtext.hip — the SAM stage after bwagpu_pair_select_device.
//
//   xa_select_kernel: the selection of mem_gen_alt (bwa/bwamem_extra.c:98-118,
//   called at bwamem_pair.c:337-340 and bwamem.c:1026-1027): which regions of a
//   read become hits of an XA string and which record carries that string, and
//   from it the regions that need a CIGAR job.
//
//   sam_count_kernel / sam_write_kernel: mem_gen_alt's strings
//   (bwamem_extra.c:120-135) and mem_aln2sam (bwa/bwamem.c:837-961) for every
//   record of a pair; see "the SAM text" below.
//
// xa_select_kernel: one wave per read, four reads per workgroup, three passes over the read's
// regions with lane i, i + 64, ... on region i.  Every loop is bounded by the
// read's count n, loaded once; every index into the read's span is below n.
// The two output arrays double as the passes' scratch, so the kernel needs no
// memory of its own and no bound on n:
//   1. job_select[i] = get_pri_idx(i)                        (reads regs only)
//   2. xa_of[i]      = that index if its string is within the caps and printed
//                      (reads job_select of the whole read, writes xa_of[i])
//   3. job_select[i] = 0 / -1                                (reads xa_of[i] only)
// A pass reads what other lanes (and, past 64 regions, the same lane) wrote in
// the pass before, so a workgroup barrier stands between them; it is reached by
// all four waves, which carry n = 0 when they have no read.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "pure.h"
#include "samtext.h"

namespace bwagpu {

namespace {
constexpr int kXaReadsPerBlock = 4;
}

__global__ void __launch_bounds__(64 * kXaReadsPerBlock) xa_select_kernel(XaSelArgs g) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t r64 = (int64_t)blockIdx.x * kXaReadsPerBlock + (threadIdx.x >> 6);
  const bool live = r64 < g.n_reads;
  const int r = live ? (int)r64 : 0;
  const int n = live ? g.n[r] : 0;
  const int64_t base = live ? g.reg_off[r] : 0;
  const bwagpu_alnreg_t* a = g.regs + base;
  const int32_t* mapq = g.out_mapq + base;
  int32_t* xa_of = g.xa_of + base;
  int32_t* job_select = g.job_select + base;
  bool done = false;
  int mate = -1;  // the no-pairing branch's mate record (bwamem_pair.c:375-384)
  if (live) {
    const bwagpu_pairsel_t& s = g.sel[r >> 1];
    done = s.status == BWAGPU_SEL_DONE;
    if (done && s.branch == BWAGPU_SEL_NO_PAIRING) mate = s.z[r & 1];
  }

  for (int i = lane; i < n; i += 64) job_select[i] = done ? xa_pri_idx(g.drop_ratio, a, n, i) : -1;
  __syncthreads();

  for (int i = lane; i < n; i += 64) {
    const int k = job_select[i];
    int x = -1;
    if (k >= 0) {  // k < n (xa_pri_idx)
      int cnt = 0;
      bool has_alt = false;
      for (int j = 0; j < n; ++j)
        if (job_select[j] == k) {
          ++cnt;
          has_alt |= (a[j].n_comp_is_alt >> 30) != 0;
        }
      // a string is printed only on an emitted record (h[i].XA, g[i].XA, q->XA)
      if (!xa_over_cap(cnt, has_alt, g.max_hits, g.max_hits_alt) && mapq[k] >= 0) x = k;
    }
    xa_of[i] = x;
  }
  __syncthreads();

  for (int i = lane; i < n; i += 64) job_select[i] = done && (mapq[i] >= 0 || xa_of[i] >= 0 || i == mate) ? 0 : -1;
}

hipError_t launch_xa_select(const XaSelArgs& a, hipStream_t st) {
  const unsigned nb = (unsigned)(((int64_t)a.n_reads + kXaReadsPerBlock - 1) / kXaReadsPerBlock);
  hipLaunchKernelGGL(xa_select_kernel, dim3(nb), dim3(64 * kXaReadsPerBlock), 0, st, a);
  return hipGetLastError();
}


// ------------------------------------------------------------ the SAM text
// One wave per read writes the read's lines.  sam_read<STORE> is the one body of
// the count pass (STORE = false: only the position advances) and of the write
// pass, so the two cannot disagree about a line.  Everything that decides a
// branch is wave-uniform; the lanes share a piece's bytes:
//   * a number: lane d writes digit d;
//   * a CIGAR: lane k takes op k (+64, ...), its width is the op's digits + 1, a
//     wave prefix sum places it, the lane writes its own digits and letter;
//   * an XA string: lane j takes region j (+64, ...); a hit's width is its whole
//     "name,+pos,CIGAR,NM;" piece, placed the same way and written by its lane;
//   * SEQ and QUAL: 64 bases per step, through the complement table and the
//     mirrored index on the reverse strand;
//   * names, MD, the comment: strided copies.
// Every loop is bounded by a count loaded once (a read's n, a record's n_cigar
// checked against max_ops, md_len against max_md, a job index against job_cap),
// and every store by the read's span [off, off + len) from the count pass.
// The offsets are the exclusive scan of the reads' lengths: per 256 reads a sum
// (sam_sums_kernel), one workgroup scans the sums (sam_scan_kernel), and a
// read's wave adds the lengths before it within its 256 (sam_write_kernel).
namespace {

constexpr int kSamReadsPerBlock = 4;

__device__ __forceinline__ int wave_incl(int v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v, int lane) { return __shfl(wave_incl(v, lane), 63, 64); }
__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0; }

// one lane's bytes from `at` on, inside [.., lim)
template <bool STORE>
struct LaneOut {
  char* out;
  int64_t at, lim;
  __device__ __forceinline__ void ch(char c) {
    if (STORE && at < lim) out[at] = c;
    ++at;
  }
  __device__ __forceinline__ void num(int64_t v) {
    const int w = dec_width(v);
    if (STORE) {
      uint64_t m = dec_mag(v);
      if (v < 0 && at < lim) out[at] = '-';
      for (int k = w - 1; k >= (v < 0); --k, m /= 10)
        if (at + k < lim) out[at + k] = (char)('0' + m % 10);
    }
    at += w;
  }
};

// the wave's position in the text; every call is made by all 64 lanes with the same arguments
template <bool STORE>
struct Emit {
  char* out;
  int64_t pos, lim;
  int lane;
  __device__ __forceinline__ void put(int64_t at, char c) const {
    if (STORE && at < lim) out[at] = c;
  }
  __device__ __forceinline__ void ch(char c) {
    if (lane == 0) put(pos, c);
    ++pos;
  }
  __device__ __forceinline__ void lit(const char* s, int n) {  // n <= 64
    if (lane < n) put(pos + lane, s[lane]);
    pos += n;
  }
  __device__ __forceinline__ void copy(const char* src, int64_t n) {
    if (STORE)
      for (int64_t i = lane; i < n; i += 64) put(pos + i, src[i]);
    pos += n;
  }
  __device__ __forceinline__ void num(int64_t v) {  // kputw / kputl
    const int w = dec_width(v);
    if (STORE && lane < w) put(pos + lane, v < 0 && lane == 0 ? '-' : (char)('0' + dec_digit(dec_mag(v), w - 1 - lane)));
    pos += w;
  }
  // ops over tab (nt letters), clips rewritten to op `clip` when clip >= 0
  __device__ void cigar(const uint32_t* cig, int n, const char* tab, int ntab, int clip) {
    for (int k0 = 0; k0 < n; k0 += 64) {
      const int k = k0 + lane;
      const uint32_t op = k < n ? cig[k] : 0;
      int c = (int)(op & 0xf);
      if (clip >= 0 && (c == 3 || c == 4)) c = clip;
      const int w = k < n ? dec_width_u64(op >> 4) + 1 : 0;
      const int incl = wave_incl(w, lane);
      if (STORE && k < n) {
        LaneOut<STORE> o{out, pos + incl - w, lim};
        o.num((int64_t)(op >> 4));
        o.ch(c < ntab ? tab[c] : '?');
      }
      pos += __shfl(incl, 63, 64);
    }
  }
  __device__ void bases(const uint8_t* seq, int qb, int qe, bool rev) {
    const int n = qe - qb;
    if (STORE)
      for (int i = lane; i < n; i += 64) {
        const int b = min((int)seq[rev ? qe - 1 - i : qb + i], 4);
        put(pos + i, rev ? "TGCAN"[b] : "ACGTN"[b]);
      }
    pos += n;
  }
  __device__ void quals(const char* q, int qb, int qe, bool rev) {
    const int n = qe - qb;
    if (STORE)
      for (int i = lane; i < n; i += 64) put(pos + i, q[rev ? qe - 1 - i : qb + i]);
    pos += n;
  }
};

// mem_aln_t as mem_reg2aln and mem_sam_pe / mem_reg2sam fill it
struct Rec {
  int64_t pos;
  int rid, is_rev, n_cigar, NM, md_len, mapq, flag, score, sub, alt_sc, is_alt;
  const uint32_t* cig;
  const char* md;
  bool bad;
};

__device__ Rec rec_unmapped() {  // mem_reg2aln(.., 0): bwamem.c:1111-1114
  Rec q{};
  q.rid = -1, q.pos = -1, q.flag = 0x4;
  return q;
}

// the record of region k of the read whose n regions start at base
__device__ Rec rec_of_region(const bwagpu_samtext_t& t, int64_t base, int n, int k) {
  Rec q = rec_unmapped();
  q.bad = true;
  if (k < 0 || k >= n) return q;
  const int job = t.dev_job_of[base + k];
  if (job < 0 || job >= t.job_cap) return q;
  const bwagpu_aln_t a = t.dev_aln[job];
  if (a.status != BWAGPU_ALN_OK || a.rid < 0 || a.rid >= t.n_contigs || a.n_cigar < 0 || a.n_cigar > t.max_ops ||
      a.md_len < 0 || a.md_len >= t.max_md)
    return q;
  const bwagpu_alnreg_t& g = t.dev_regs[base + k];
  q.bad = false, q.flag = 0;
  q.pos = a.pos, q.rid = a.rid, q.is_rev = a.is_rev != 0, q.n_cigar = a.n_cigar, q.NM = a.NM, q.md_len = a.md_len;
  q.cig = t.dev_cigar + (int64_t)job * t.max_ops, q.md = t.dev_md + (int64_t)job * t.max_md;
  q.score = g.score, q.sub = g.sub > g.csub ? g.sub : g.csub;  // bwamem.c:1170-1171
  q.alt_sc = g.alt_sc, q.is_alt = (g.n_comp_is_alt >> 30) != 0;
  return q;
}

__device__ int rec_rlen(const Rec& q, int lane) {  // get_rlen, bwamem.c:813-822
  int l = 0;
  for (int k = lane; k < q.n_cigar; k += 64) {
    const uint32_t op = q.cig[k];
    if ((op & 0xf) == 0 || (op & 0xf) == 2) l += (int)(op >> 4);
  }
  return wave_sum(l, lane);
}

// one read's part of its pair's decision, and the read itself
struct ReadCtx {
  int i;  // 0 / 1 within the pair
  int64_t base;
  int n;
  bool paired;
  int z, alt, mapq_h, flag0;  // h[i]'s region, g[i]'s or -1, h[i]'s mapq, the flag of every record
  int l_seq;
  const uint8_t* seq;
  const char* qual;
};

// the read's record list as region indices: first_rec, next_rec ... -1
__device__ int next_rec(const bwagpu_samtext_t& t, const ReadCtx& c, int k, int lane) {
  if (c.paired) return k < 0 ? c.z : (k == c.z ? c.alt : -1);
  for (int k0 = (k + 1) & ~63; k0 < c.n; k0 += 64) {
    const int j = k0 + lane;
    const uint64_t m = __ballot(j > k && j < c.n && t.dev_out_mapq[c.base + j] >= 0);
    if (m) return k0 + __builtin_ctzll(m);
  }
  return -1;
}
__device__ Rec list_rec(const bwagpu_samtext_t& t, const ReadCtx& c, int k, int which) {
  Rec q = rec_of_region(t, c.base, c.n, k);
  if (c.paired) {
    q.mapq = (k == c.z ? c.mapq_h : t.dev_out_mapq[c.base + k]) & 0xff;
    q.flag |= c.flag0 | (k == c.z ? 0 : 0x800);
  } else {
    q.mapq = t.dev_out_mapq[c.base + k] & 0xff;
    q.flag |= c.flag0 | (which ? 0x800 : 0);
  }
  return q;
}

// the XA / XB field of the record of region key (bwamem_extra.c:120-135, bwamem.c:947-950) -> false: needs the host
template <bool STORE>
__device__ bool sam_xa(const SamTextArgs& g, Emit<STORE>& e, const ReadCtx& c, int key) {
  const bwagpu_samtext_t& t = g.t;
  const bool xb = (t.flags & BWAGPU_MEM_F_XB) != 0;
  bool opened = false;
  for (int j0 = 0; j0 < c.n; j0 += 64) {
    const int j = j0 + e.lane;
    const bool hit = j < c.n && t.dev_xa_of[c.base + j] == key;
    if (!wave_any(hit)) continue;
    Rec q{};
    int64_t nb = 0, ne = 0;
    int w = 0;
    if (hit) {
      q = rec_of_region(t, c.base, c.n, j);
      if (!q.bad) {
        nb = t.dev_contig_off[q.rid], ne = max(t.dev_contig_off[q.rid + 1], nb);
        w = (int)(ne - nb) + 2 + dec_width(q.pos + 1) + 1;
        for (int k = 0; k < q.n_cigar; ++k) w += dec_width_u64(q.cig[k] >> 4) + 1;
        w += 1 + dec_width(q.NM) + (xb ? 1 + dec_width(q.score) : 0) + 1;
      }
    }
    if (wave_any(hit && q.bad)) return false;
    if (!opened) e.lit(xb ? "\tXB:Z:" : "\tXA:Z:", 6), opened = true;
    const int incl = wave_incl(w, e.lane);
    if (STORE && hit) {
      LaneOut<STORE> o{e.out, e.pos + incl - w, e.lim};
      for (int64_t x = nb; x < ne; ++x) o.ch(t.dev_contig_names[x]);
      o.ch(','), o.ch("+-"[q.is_rev]), o.num(q.pos + 1), o.ch(',');
      for (int k = 0; k < q.n_cigar; ++k) {
        const uint32_t op = q.cig[k];
        o.num((int64_t)(op >> 4)), o.ch((op & 0xf) < 6 ? "MIDSHN"[op & 0xf] : '?');
      }
      o.ch(','), o.num(q.NM);
      if (xb) o.ch(','), o.num(q.score);
      o.ch(';');
    }
    e.pos += __shfl(incl, 63, 64);
  }
  return true;
}

template <bool STORE>
__device__ void sam_contig(const bwagpu_samtext_t& t, Emit<STORE>& e, int rid) {
  const int64_t b = t.dev_contig_off[rid];
  e.copy(t.dev_contig_names + b, max(t.dev_contig_off[rid + 1] - b, (int64_t)0));
}

// mem_aln2sam (bwamem.c:837-961) for record `which` (of region k) of the read's list, mate m0 -> false: needs the host
template <bool STORE>
__device__ bool sam_line(const SamTextArgs& g, Emit<STORE>& e, const ReadCtx& c, int r, const Rec& p0, int k, int which,
                         int n_list, const Rec& m0, int m_rlen) {
  const bwagpu_samtext_t& t = g.t;
  Rec p = p0, m = m0;
  SamCoord pc{p.pos, p.rid, p.is_rev, p.n_cigar}, mc{m.pos, m.rid, m.is_rev, m.n_cigar};
  p.flag = sam_flag(p.flag, &pc, &mc);
  p.pos = pc.pos, p.rid = pc.rid, p.is_rev = pc.is_rev, p.n_cigar = pc.n_cigar;
  m.pos = mc.pos, m.rid = mc.rid, m.is_rev = mc.is_rev, m.n_cigar = mc.n_cigar;
  const int p_rlen = p.n_cigar ? rec_rlen(p, e.lane) : 0;

  const int64_t nm_b = t.dev_name_off[r];
  e.copy(t.dev_names + nm_b, max(t.dev_name_off[r + 1] - nm_b, (int64_t)0));
  e.ch('\t');
  e.num(p.flag & 0xffff);
  e.ch('\t');
  if (p.rid >= 0) {
    sam_contig(t, e, p.rid);
    e.ch('\t'), e.num(p.pos + 1), e.ch('\t'), e.num(p.mapq), e.ch('\t');
    if (p.n_cigar) e.cigar(p.cig, p.n_cigar, "MIDSH", 5, sam_clip_rewrite(t.flags, p.is_alt) ? sam_cigar_op(3, true, which) : -1);
    else e.ch('*');
  } else {
    e.lit("*\t0\t0\t*", 7);
  }
  e.ch('\t');
  if (m.rid >= 0) {
    if (p.rid == m.rid) e.ch('=');
    else sam_contig(t, e, m.rid);
    e.ch('\t'), e.num(m.pos + 1), e.ch('\t');
    if (p.rid == m.rid) e.num(sam_tlen(pc, p_rlen, mc, m_rlen));
    else e.ch('0');
  } else {
    e.lit("*\t0\t0", 5);
  }
  e.ch('\t');
  {
    int qb = 0, qe = c.l_seq;
    if (p.n_cigar) {
      sam_seq_range(c.l_seq, which && sam_clip_rewrite(t.flags, p.is_alt), p.is_rev, p.cig[0], p.cig[p.n_cigar - 1], &qb,
                    &qe);
      qb = min(max(qb, 0), c.l_seq), qe = min(max(qe, qb), c.l_seq);
    }
    e.bases(c.seq, qb, qe, p.is_rev);
    e.ch('\t');
    if (c.qual) e.quals(c.qual, qb, qe, p.is_rev);
    else e.ch('*');
  }
  if (p.n_cigar) {
    e.lit("\tNM:i:", 6), e.num(p.NM);
    e.lit("\tMD:Z:", 6), e.copy(p.md, p.md_len);
  }
  if (m.n_cigar) {
    e.lit("\tMC:Z:", 6);
    e.cigar(m.cig, m.n_cigar, "MIDSH", 5, sam_clip_rewrite(t.flags, m.is_alt) ? sam_cigar_op(3, true, which) : -1);
  }
  if (p.score >= 0) e.lit("\tAS:i:", 6), e.num(p.score);
  if (p.sub >= 0) e.lit("\tXS:i:", 6), e.num(p.sub);
  if (g.rg_len) e.lit("\tRG:Z:", 6), e.copy(g.rg, g.rg_len);
  if (n_list > 1) {  // no record carries 0x100, so every other record of the list is printed
    e.lit("\tSA:Z:", 6);
    int w2 = 0;
    for (int k2 = next_rec(t, c, -1, e.lane); k2 >= 0; k2 = next_rec(t, c, k2, e.lane), ++w2) {
      if (w2 == which) continue;
      const Rec q = list_rec(t, c, k2, w2);
      if (q.bad) return false;
      sam_contig(t, e, q.rid);
      e.ch(','), e.num(q.pos + 1), e.ch(','), e.ch("+-"[q.is_rev]), e.ch(',');
      e.cigar(q.cig, q.n_cigar, "MIDSH", 5, -1);
      e.ch(','), e.num(q.mapq), e.ch(','), e.num(q.NM), e.ch(';');
    }
  }
  if (p.alt_sc > 0) {
    bool neg;
    const uint64_t th = pa_thousandths(p.score, p.alt_sc, &neg);
    e.lit("\tpa:f:", 6);
    if (neg) e.ch('-');
    e.num((int64_t)(th / 1000)), e.ch('.');
    e.ch((char)('0' + th / 100 % 10)), e.ch((char)('0' + th / 10 % 10)), e.ch((char)('0' + th % 10));
  }
  if (k >= 0 && !sam_xa(g, e, c, k)) return false;
  if (t.dev_comment_off) {
    const int64_t b = t.dev_comment_off[r], n = t.dev_comment_off[r + 1] - b;
    if (n > 0) e.ch('\t'), e.copy(t.dev_comments + b, n);
  }
  e.ch('\n');
  return true;
}

// every line of read r of a pair with sel.status == BWAGPU_SEL_DONE -> false: the pair needs the host
template <bool STORE>
__device__ bool sam_read(const SamTextArgs& g, int r, Emit<STORE>& e) {
  const bwagpu_samtext_t& t = g.t;
  const bwagpu_pairsel_t s = t.dev_sel[r >> 1];
  ReadCtx c{};
  c.i = r & 1, c.base = t.dev_reg_off[r], c.n = t.dev_n[r];
  c.paired = s.branch == BWAGPU_SEL_PAIRED;
  c.z = s.z[c.i], c.alt = c.paired ? s.alt[c.i] : -1, c.mapq_h = s.mapq[c.i];
  c.flag0 = c.paired ? (0x40 << c.i) | s.extra_flag : s.extra_flag | (c.i ? 0x81 : 0x41);
  const int64_t sb = t.dev_seq_off[r], l = t.dev_seq_off[r + 1] - sb;
  if (c.n < 0 || l < 0 || l > 0x7fffffff || c.alt < -1 || c.alt >= c.n) return false;
  c.l_seq = (int)l, c.seq = t.dev_seq + sb, c.qual = t.dev_qual ? t.dev_qual + sb : nullptr;
  // the mate record h[!i]: region z[!i] of the other read (bwamem_pair.c:343, 375-384)
  const int zm = s.z[!c.i];
  if (c.paired ? (c.z < 0 || c.z >= c.n || zm < 0) : zm < -1) return false;
  const int nm = t.dev_n[r ^ 1];
  const Rec m = zm >= 0 ? rec_of_region(t, t.dev_reg_off[r ^ 1], nm, zm) : rec_unmapped();
  if (m.bad) return false;
  const int m_rlen = m.n_cigar ? rec_rlen(m, e.lane) : 0;

  int n_list = 0;
  if (c.paired) {
    n_list = 1 + (c.alt >= 0);
  } else {
    for (int k0 = 0; k0 < c.n; k0 += 64) {
      const int j = k0 + e.lane;
      n_list += __popcll(__ballot(j < c.n && t.dev_out_mapq[c.base + j] >= 0));
    }
  }
  if (n_list == 0) {  // mem_reg2sam's unaligned record (bwamem.c:1048-1052)
    Rec p = rec_unmapped();
    p.flag |= c.flag0;
    return sam_line(g, e, c, r, p, -1, 0, 1, m, m_rlen);
  }
  int which = 0;
  for (int k = next_rec(t, c, -1, e.lane); k >= 0; k = next_rec(t, c, k, e.lane), ++which) {
    const Rec p = list_rec(t, c, k, which);
    if (p.bad || !sam_line(g, e, c, r, p, k, which, n_list, m, m_rlen)) return false;
  }
  return true;
}

}  // namespace

__global__ void sam_rg_kernel(SamRgBytes rg, char* dst) { dst[threadIdx.x] = rg.c[threadIdx.x]; }

// step 1: len[r] = the bytes of read r's lines, status[pair]; a pair with a status has no bytes
__global__ void __launch_bounds__(64 * kSamReadsPerBlock) sam_count_kernel(SamTextArgs g) {
  __shared__ int s_st[kSamReadsPerBlock];
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  const int64_t r64 = (int64_t)blockIdx.x * kSamReadsPerBlock + w;
  const bool live = r64 < g.n_reads;
  const int r = live ? (int)r64 : 0;
  int st = BWAGPU_SAM_DONE;
  int64_t len = 0;
  if (live) {
    if (g.t.dev_sel[r >> 1].status != BWAGPU_SEL_DONE) {
      st = BWAGPU_SAM_SKIPPED;
    } else {
      Emit<false> e{nullptr, 0, 0, lane};
      if (!sam_read<false>(g, r, e) || e.pos > 0x7fffffff) st = BWAGPU_SAM_NEEDS_HOST;
      len = e.pos;
    }
  }
  if (lane == 0) s_st[w] = st;
  __syncthreads();
  st = max(st, s_st[w ^ 1]);  // reads 2i and 2i+1 are waves w and w ^ 1 of one workgroup
  if (live && lane == 0) {
    g.len[r] = st ? 0 : (int32_t)len;
    if (!(r & 1)) g.t.dev_status[r >> 1] = st;
  }
}

// step 2a: per 256 reads the sum of their lengths
__global__ void __launch_bounds__(256) sam_sums_kernel(SamTextArgs g) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t total = 0;
  (void)block_excl_scan<int64_t>(r < g.n_reads ? g.len[r] : 0, &total);
  if (threadIdx.x == 0) g.sums[blockIdx.x] = total;
}

// step 2b, one workgroup: the sums -> their exclusive prefix in place; text_n[1] = the bytes
// needed, text_n[0] = the bytes written: all of them, or the start of the first pair whose end
// passes text_cap (pairs do not straddle a group of 256 reads)
__global__ void __launch_bounds__(256) sam_scan_kernel(SamTextArgs g, int n_blocks) {
  __shared__ int s_grp;
  __shared__ int64_t s_start;
  const int64_t cap = g.t.text_cap;
  if (threadIdx.x == 0) s_grp = -1;
  int64_t carry = 0;
  for (int x0 = 0; x0 < n_blocks; x0 += 256) {
    const int x = x0 + (int)threadIdx.x;
    const int64_t v = x < n_blocks ? g.sums[x] : 0;
    int64_t total = 0;
    const int64_t ex = carry + block_excl_scan<int64_t>(v, &total);
    if (x < n_blocks) {
      g.sums[x] = ex;
      if (ex <= cap && cap < ex + v) s_grp = x, s_start = ex;
    }
    carry += total;
  }
  __syncthreads();
  const int grp = s_grp;
  if (grp < 0) {
    if (threadIdx.x == 0) g.t.dev_text_n[0] = g.t.dev_text_n[1] = carry;
    return;
  }
  const int64_t r = (int64_t)grp * 256 + threadIdx.x;
  const int64_t v = r < g.n_reads ? g.len[r] : 0;
  int64_t total = 0;
  const int64_t at = s_start + block_excl_scan<int64_t>(v, &total);
  const int64_t v1 = __shfl_down(v, 1, 64);  // the odd read of an even lane's pair
  if (!(threadIdx.x & 1) && at <= cap && cap < at + v + v1) g.t.dev_text_n[0] = at;
  if (threadIdx.x == 0) g.t.dev_text_n[1] = carry;
}

// step 3: text_off and the text
__global__ void __launch_bounds__(64 * kSamReadsPerBlock) sam_write_kernel(SamTextArgs g) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t r64 = (int64_t)blockIdx.x * kSamReadsPerBlock + (threadIdx.x >> 6);
  if (r64 >= g.n_reads) return;
  const int r = (int)r64, g0 = r & ~255;
  int64_t sum = 0;  // the lengths before this read within its 256
  for (int x = g0 + lane; x < r; x += 64) sum += g.len[x];
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  const int64_t at = g.sums[r >> 8] + sum;
  const int len = g.len[r], len_pair = len + g.len[r ^ 1];
  const int64_t pair_end = (r & 1) ? at + len : at + len_pair;
  const int64_t written = g.t.dev_text_n[0];
  const bool room = pair_end <= g.t.text_cap;
  if (lane == 0) {
    g.t.dev_text_off[r] = min(at, written);
    if (r == g.n_reads - 1) g.t.dev_text_off[g.n_reads] = written;
    if (!room && !(r & 1) && len_pair > 0) g.t.dev_status[r >> 1] = BWAGPU_SAM_NO_ROOM;
  }
  if (!room || len == 0) return;
  Emit<true> e{g.t.dev_text, at, at + len, lane};
  (void)sam_read<true>(g, r, e);
}

static SamTextArgs sam_args(const bwagpu_samtext_t& t, int32_t n_reads, int32_t rg_len, void* scratch) {
  SamTextArgs a{};
  a.t = t, a.n_reads = n_reads, a.rg_len = rg_len;
  char* p = (char*)scratch;
  a.rg = p;
  a.sums = (int64_t*)(p + 256);
  a.len = (int32_t*)(p + 256 + sizeof(int64_t) * (((size_t)n_reads + 255) / 256));
  return a;
}

hipError_t launch_sam_text_step(int step, const bwagpu_samtext_t& t, int32_t n_reads, const SamRgBytes& rg,
                                int32_t rg_len, void* scratch, hipStream_t st) {
  const SamTextArgs a = sam_args(t, n_reads, rg_len, scratch);
  const unsigned nb = (unsigned)(((int64_t)n_reads + kSamReadsPerBlock - 1) / kSamReadsPerBlock);
  const int ns = (int)(((int64_t)n_reads + 255) / 256);
  if (step == 0) {
    hipLaunchKernelGGL(sam_rg_kernel, dim3(1), dim3(BWAGPU_SAM_MAX_RG + 1), 0, st, rg, (char*)scratch);
    hipLaunchKernelGGL(sam_count_kernel, dim3(nb), dim3(64 * kSamReadsPerBlock), 0, st, a);
  }
  if (step == 1) {
    hipLaunchKernelGGL(sam_sums_kernel, dim3(ns), dim3(256), 0, st, a);
    hipLaunchKernelGGL(sam_scan_kernel, dim3(1), dim3(256), 0, st, a, ns);
  }
  if (step == 2) hipLaunchKernelGGL(sam_write_kernel, dim3(nb), dim3(64 * kSamReadsPerBlock), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_sam_text(const bwagpu_samtext_t& t, int32_t n_reads, const SamRgBytes& rg, int32_t rg_len,
                           void* scratch, hipStream_t st) {
  for (int step = 0; step < 3; ++step)
    if (hipError_t e = launch_sam_text_step(step, t, n_reads, rg, rg_len, scratch, st)) return e;
  return hipGetLastError();
}

}  // namespace bwagpu
