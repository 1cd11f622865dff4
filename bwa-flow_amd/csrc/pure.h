// pure.h — the scoring options, kernel tables and arithmetic that the kernels'
// launchers and the host-side plans (task_host.h) share.  Plain C++: compiles
// without HIP.  engine.h, align2.h and reg2aln.h include it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bwagpu.h"

#ifdef __HIPCC__
#define BWAGPU_HD __host__ __device__
#else
#define BWAGPU_HD
#endif

namespace bwagpu {

// Scoring parameters in the form the kernels use (from bwagpu_opt_t).
struct DevOpt {
  int a, o_del, e_del, o_ins, e_ins, oe_del, oe_ins;
  int pen_clip5, pen_clip3, w, zdrop, max_mat;
  int row_bound;  // extend_quad ends a call once no later row can change its outputs
  int8_t mat[28];
  // query profile words: qprof[q] byte t = mat[t*5 + q] (t = target base 0..3),
  // qprof4[q] = mat[20 + q] (target N; only bare task lists can hold one —
  // targets fetched from the pac are 0..3).  Kernel arguments, so the DP picks
  // its scores with register selects instead of loads.
  uint32_t qprof[5];
  int32_t qprof4[5];
};

// Kernel variants: G lanes per read ("group"), C = max DP columns per lane.
// A read of length l needs G*C >= l (+1 column for eh[qlen], qlen <= l-1).
enum { VK_FAST = 0, VK_GENERIC = 1 };
struct Variant {
  int G, C;
  int kind;  // VK_FAST: chain2aln_fast_kernel (wave per read), VK_GENERIC: chain2aln_kernel
  BWAGPU_HD constexpr int max_len() const { return G * C; }
};
// bare ksw_extend2 task lists (bwagpu_extend_batch): wave kernels by columns
constexpr int kNumExtVariants = 3;
inline constexpr Variant kExtVariants[kNumExtVariants] = {{64, 3, VK_FAST}, {64, 4, VK_FAST}, {64, 16, VK_GENERIC}};
constexpr int kBlock = 256;  // threads per workgroup (4 waves)

// rows a task can touch: the band is empty once i - w >= qlen (ksw.c:417-419),
// so rows i <= qlen + w are the most ever read (the last one only to break)
BWAGPU_HD inline int band_cap(int qlen, int max_mat, int end_bonus, int o, int e) {
  int l = (int)((double)(qlen * max_mat + end_bonus - o) / e + 1.);
  return l > 1 ? l : 1;
}

// LDS row-buffer bytes per group for reads up to lq_max (see rows_needed)
inline int tb_bytes_for(const DevOpt& o, int lq_max) {
  const int eb = std::max(o.pen_clip5, o.pen_clip3);
  const int cap = std::max(band_cap(lq_max, o.max_mat, eb, o.o_ins, o.e_ins),
                           band_cap(lq_max, o.max_mat, eb, o.o_del, o.e_del));
  const int we = std::min(o.w << 1, cap);
  const int n = lq_max + we + 2;
  return (n + 15) & ~15;
}

// the 32-bit kernels (extend_wave, extend_pair): a row's maximum and its last
// column are one reduction of the int key H << 10 | j (ksw_dev.h), exact while
// every H of the call is below 2^21.  mem_chain2aln stays far below (a <= 127,
// reads <= 1023); a bare task's h0 is the caller's (extend_plan refuses it).
inline bool wave_bound_ok(long hb) { return hb < (1L << 21); }  // hb: a bound on every H of the call

// the packed ranges (extend_quad) for reads up to lq: H <= lq * max(mat) < 4096
// (the row-max key H << KS | c is an unsigned 16-bit value: KS = 1..4 in-lane
// column bits for CPL <= 2 / 4 / 8 / 16 columns per lane, so H < 2^12 at
// KS = 4; it passes 32767 from H = 2048 on there, which the unsigned reduction
// takes), H * 2^sk + 128 < 2^15 (2^sk > max(mat); M' is a signed minimum), and
// the scan values H + 33 * CPL * e_ins < 2^15 (CPL <= 8 with 32 lanes, 16 with 16)
inline bool quad_bound_ok(const DevOpt& o, long hb) {  // hb: a bound on every H of the call
  if (o.max_mat < 1 || o.max_mat > 15) return false;
  const int sk = 32 - __builtin_clz((unsigned)o.max_mat);
  for (int k = 0; k < 25; ++k)
    if (o.mat[k] < -127 || o.mat[k] > 127) return false;
  return hb < 4096 && (hb << sk) + 128 < 32768 && hb + 33L * 8 * o.e_ins < 32768 && o.o_del + 128L < 32768 &&
         o.oe_ins + 128L < 32768 && o.e_del < 32768;
}
inline bool quad_scores_ok(const DevOpt& o, int lq) { return quad_bound_ok(o, (long)lq * o.max_mat); }
// the 8-bit-column row-max key (extend_quad<.., true>): every H of reads up to lq < 256
inline bool quad_key8_ok(const DevOpt& o, int lq) { return (long)lq * o.max_mat <= 255; }
// the packed row-end state for calls of up to `rows` target rows: i, |i - j|
// and the z-drop term max((di - dj) e_del, (dj - di) e_ins) (di <= rows,
// dj <= 256) within 16 bits beside H < 4096
inline bool quad_rows_ok(const DevOpt& o, long rows) {
  return rows >= 0 && rows < 16384 && (rows + 256) * std::max(o.e_del, o.e_ins) < 28672;
}

// ksw_align2 (align2.hip).  Segment-count buckets: one compiled kernel per
// (bucket, u8/i16).  A task's bucket is that of its first pass
// (p*ceil(qlen/p) columns over 64 lanes); its reverse pass has fewer columns
// and reuses the same body.
constexpr int kA2Buckets = 8;
inline constexpr int kA2CD[kA2Buckets] = {1, 2, 3, 4, 6, 8, 12, 16};
constexpr int kA2Bins = 2 * kA2Buckets;  // bins [0, 8): i16, [8, 16): u8

BWAGPU_HD inline int a2_bin_of(int qlen, bool u8) {
  const int p = u8 ? 16 : 8;
  const int ncol = (qlen + p - 1) / p * p;
  const int cd = ncol > 64 ? (ncol + 63) / 64 : 1;
  const int b = cd <= 4 ? cd - 1 : cd <= 6 ? 4 : cd <= 8 ? 5 : cd <= 12 ? 6 : 7;
  return (u8 ? kA2Buckets : 0) + b;
}

// scoring limits of the align2 kernels (reasons are the E_UNSUPPORTED text).
// The reference holds e_del, e_ins, o_del + e_del and o_ins + e_ins in SIMD
// lanes of the pass's width and keeps their low bits only: 16 in ksw_i16
// (_mm_set1_epi16, ksw.c:252-255), 8 in ksw_u8 (_mm_set1_epi8, ksw.c:132-135).
// The kernels compute with the untruncated values, so a penalty the reference
// would truncate is refused, not emulated (the closed-form F of align2.hip is
// proved for o_ins > 0 only, and a truncated o_ins + e_ins can fall to e_ins or
// below).  The word limit holds for every task, the byte limit for tasks that
// carry BWAGPU_KSW_XBYTE; these two functions are the only place either is written.
inline constexpr const char* kA2WordWhy =
    "ksw_align2 with o_del + e_del or o_ins + e_ins > 65535: the reference keeps 16 bits of them "
    "(_mm_set1_epi16, ksw.c:252-255)";
inline constexpr const char* kA2ByteWhy =
    "ksw_align2 XBYTE task with e_del, e_ins, o_del + e_del or o_ins + e_ins > 255: the reference's 8-bit pass "
    "keeps 8 bits of them (_mm_set1_epi8, ksw.c:132-135)";
inline constexpr const char* kA2ByteRescueWhy =
    "mate rescue with e_del, e_ins, o_del + e_del or o_ins + e_ins > 255: whether a read is short enough for "
    "ksw_align2's 8-bit pass (l_ms * a < 250) is known only on the device, and that pass keeps 8 bits of them "
    "(_mm_set1_epi8, ksw.c:132-135)";
inline const char* align2_opt_unsupported(const DevOpt& o) {
  if (o.o_ins <= 0)
    return "ksw_align2 with o_ins == 0: the reference's lazy-F early exit (ksw.c:180) then depends on "
           "its SIMD lane order; run it on the CPU";
  if (o.max_mat <= 0) return "ksw_align2 needs a positive match score (ksw.c:216 divides by it)";
  if (o.o_ins > 65535 || o.e_ins > 65535 || o.o_del > 65535 || o.e_del > 65535) return "gap penalty > 65535";
  if (o.oe_del > 65535 || o.oe_ins > 65535) return kA2WordWhy;
  return nullptr;
}
BWAGPU_HD inline bool align2_byte_ok(const DevOpt& o) {
  return o.e_del <= 255 && o.e_ins <= 255 && o.oe_del <= 255 && o.oe_ins <= 255;
}
// a word task whose 16-bit scores could saturate (ksw_i16 clamps at 32767)
BWAGPU_HD inline bool align2_word_fits(int qlen, int max_mat) { return (int64_t)qlen * max_mat <= 32767; }

// mem_reg2aln's CIGAR (reg2aln.hip).  Query-length buckets: one compiled
// kernel per strided segment count CD (eh[] slots 0..qlen over 64 lanes:
// qlen + 1 <= 64 * CD)
constexpr int kR2Buckets = 6;
inline constexpr int kR2CD[kR2Buckets] = {1, 2, 3, 4, 8, 16};
BWAGPU_HD inline int r2_bucket_of(int qlen) {
  const int cd = (qlen + 64) >> 6;
  return cd <= 4 ? cd - 1 : (cd <= 8 ? 4 : 5);
}
// a job's direction matrix (ksw_global2's z, ncol x tlen bytes, ksw.c:511-512)
// sits in LDS up to kR2ZSmall / kR2ZLarge bytes and in a per-wave HBM slice beyond
constexpr int kR2ZSmall = 8 * 1024, kR2ZLarge = 24 * 1024;
constexpr int kR2MaxRef = 8192;  // reference window bytes per job (LDS)

// bwagpu_reg2aln_device: one job's place among the kernel's bins, by the
// arithmetic of bwagpu_reg2aln_batch's validation loop (capi_tasks.hip).  On
// every job this accepts, lq / rl / zb / bucket / cls are what that loop
// computes; a job that loop refuses with an error code is R2_REFUSED here.
// Two bounds are this function's own: truesc within [-2^24, 2^24] and w within
// [0, 2^24] (no real score reaches them: a <= 127, reads <= 1023 bp).  With
// them, lq <= 1023, rl <= 8192 and the context's option ranges (make_opt) no
// 32-bit expression of the band inference wraps, here or in reg2aln_kernel's
// infer_bw_dev: the kernel trusts its bin's LDS capacities, so a job whose
// real band is wider than the one that sized zb would write past its wave's LDS.
enum { R2_ACCEPTED = 0, R2_REFUSED = 1 };
constexpr int kR2Bins = kR2Buckets * 3;  // bin = bucket * 3 + cls
constexpr int kR2CostClasses = 8;        // inside a bin, 0 = the largest matrices
constexpr int kR2ScoreBound = 1 << 24;
constexpr int kR2LdsPerBlock = 160 * 1024;
struct R2Class {
  int verdict;  // R2_*
  int lq, rl;   // 0 for a job that gets no DP (unmapped, no CIGAR)
  int64_t zb;   // bytes of the widest try's direction matrix
  int bucket, cls;
};

// per-wave LDS bytes of a bin whose longest query is qmax, longest window rmax
BWAGPU_HD inline int r2_lds_per_wave(int qmax, int rmax, int cls, int* qcap, int* rcap, int* ocap) {
  *qcap = (qmax + 16) & ~15;
  *rcap = (rmax + 16) & ~15;
  *ocap = *qcap + *rcap + 4;
  int lpw = *qcap + *rcap + 4 * *ocap;
  if (cls < 2) lpw += cls == 0 ? kR2ZSmall : kR2ZLarge;
  return (lpw + 15) & ~15;
}

BWAGPU_HD inline int r2_infer_bw(int lq, int rl, int a, int truesc, int q_, int r_) {  // infer_bw, bwamem.c:801-808
  if (lq == rl && lq * a - truesc < (q_ + r_ - a) * 2) return 0;
  const int w = (int)((double)((lq < rl ? lq : rl) * a - truesc - q_) / r_ + 2.);
  const int d = lq > rl ? lq - rl : rl - lq;
  return w > d ? w : d;
}

BWAGPU_HD inline R2Class r2_classify(const DevOpt& o, int64_t l_pac, int64_t qpool_len,
                                     const bwagpu_reg2aln_task_t& t) {
  R2Class c{R2_REFUSED, 0, 0, 0, 0, 0};
  if (t.l_seq < 0 || t.qoff < 0 || t.qoff > qpool_len - t.l_seq) return c;  // read outside the pool
  if (t.truesc < -kR2ScoreBound || t.truesc > kR2ScoreBound || t.w < 0 || t.w > kR2ScoreBound) return c;
  const int64_t two = l_pac << 1;
  if (t.rb >= 0 && t.re >= 0) {
    const int64_t beg = t.rb, end = t.re > two ? two : t.re;
    const bool ok = t.qe > t.qb && t.rb < t.re && !(t.rb < l_pac && t.re > l_pac) &&
                    (beg >= l_pac || end <= l_pac) && end - beg == t.re - t.rb;
    if (ok) {
      if (t.qb < 0 || t.qe > t.l_seq) return c;                     // qb/qe outside the read
      if ((int64_t)t.qe - t.qb > BWAGPU_MAX_READ_LEN) return c;
      if (t.re - t.rb > kR2MaxRef) return c;
      const int lq = t.qe - t.qb, rl = (int)(t.re - t.rb);
      // the widest band any try can use: the first try's w2 (bwamem.c:1123-1126)
      // doubled at most twice (1132), capped at opt->w << 2, then bwa.c:152-159
      const int wmax = o.w << 2;
      int w2 = r2_infer_bw(lq, rl, o.a, t.truesc, o.o_del, o.e_del);
      const int w2i = r2_infer_bw(lq, rl, o.a, t.truesc, o.o_ins, o.e_ins);
      if (w2i > w2) w2 = w2i;
      if (w2 > o.w) w2 = w2 < t.w ? w2 : t.w;
      if (w2 > wmax) w2 = wmax;
      const int64_t w24 = (int64_t)w2 * 4;
      const int w2max = (int)(w24 < wmax ? w24 : wmax);
      const int half = (lq + 1) >> 1;
      const int mi = (int)((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
      const int mdl = (int)((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
      int mg = mi > mdl ? mi : mdl;
      if (mg < 1) mg = 1;
      const int dl = rl > lq ? rl - lq : lq - rl;
      int wb = (mg + dl + 1) >> 1;
      if (wb > w2max) wb = w2max;
      if (wb < dl + 3) wb = dl + 3;
      c.lq = lq, c.rl = rl;
      c.zb = (int64_t)(lq < 2 * wb + 1 ? lq : 2 * wb + 1) * rl;
      c.cls = c.zb <= kR2ZSmall ? 0 : (c.zb <= kR2ZLarge ? 1 : 2);
      // a single-job batch of the host form: its bin's LDS must fit a workgroup
      int qc, rc, oc;
      if ((c.cls == 1 ? 1 : 4) * r2_lds_per_wave(lq, rl, c.cls, &qc, &rc, &oc) > kR2LdsPerBlock) return c;
    }
  }
  c.bucket = r2_bucket_of(c.lq);
  c.verdict = R2_ACCEPTED;
  return c;
}

// the coarse order inside a bin: 0 holds the largest zb + lq + rl.  Steps of 512
// in the small LDS class (they part the jobs whose first try is the ungapped
// shortcut, zb = 7 rl and most regions of a real batch, from the narrowest
// banded ones at 100, 150 and 250 bp; everything from 3584 up runs first),
// steps of 4096 in the large one, octaves in the HBM class.  Finer classes were
// measured and bring nothing.
BWAGPU_HD inline int r2_cost_class(int cls, int64_t cost) {
  int64_t s = cls == 0 ? cost >> 9 : (cls == 1 ? (cost - kR2ZSmall) >> 12 : 0);
  if (cls == 2)
    for (int64_t v = cost >> 15; v > 0; v >>= 1) ++s;
  if (s < 0) s = 0;
  return s >= kR2CostClasses ? 0 : kR2CostClasses - 1 - (int)s;
}

// mem_gen_alt's selection (samtext.hip).  get_pri_idx (bwa/bwamem_extra.c:90-95)
// on a read's n regions: the region whose XA string region i would join, or -1.
// The reference hands its float option to a double parameter, so the product is
// a double one: 0.8f is 0.800000011920929, and a hit of 80 under a primary of 100
// is dropped.  A secondary_all outside the read (the reference would read past
// its array) joins nothing.
BWAGPU_HD inline int xa_pri_idx(double drop_ratio, const bwagpu_alnreg_t* a, int n, int i) {
  const int k = a[i].secondary_all;
  if (k >= 0 && k < n && a[i].score >= a[k].score * drop_ratio) return k;
  return -1;
}
// the two caps (bwamem_extra.c:118): cnt hits joined the string, has_alt = one of them is an ALT hit
BWAGPU_HD inline bool xa_over_cap(int cnt, bool has_alt, int max_hits, int max_hits_alt) {
  return cnt > max_hits_alt || (!has_alt && cnt > max_hits);
}

// ---- the arithmetic of mem_aln2sam (bwa/bwamem.c:824-961) behind bwagpu_sam_text_device ----

// characters kputw / kputl print for v: its decimal digits and the sign
BWAGPU_HD inline int dec_width_u64(uint64_t v) {
  int w = 1;
  while (v >= 10) v /= 10, ++w;
  return w;
}
BWAGPU_HD inline uint64_t dec_mag(int64_t v) { return v < 0 ? 0 - (uint64_t)v : (uint64_t)v; }
BWAGPU_HD inline int dec_width(int64_t v) { return dec_width_u64(dec_mag(v)) + (v < 0); }
// the k-th digit of v from the right (k = 0: the ones)
BWAGPU_HD inline int dec_digit(uint64_t v, int k) {
  for (; k > 0; --k) v /= 10;
  return (int)(v % 10);
}

// "pa:f:%.3f" of (double)score / alt_sc (bwamem.c:945): the thousandths that printf
// prints, which rounds the quotient's exact binary value half-to-even, taken in
// integers from the double's mantissa.  x = M * 2^-s with M < 2^53, so M * 1000
// fits 63 bits; a quotient under 2^-11 (s > 63) rounds to zero.  *neg: the
// quotient's sign bit, which printf prints in front of a zero as well.
BWAGPU_HD inline uint64_t pa_thousandths(int score, int alt_sc, bool* neg) {
  const double x = (double)score / alt_sc;
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  *neg = (b >> 63) != 0;
  const int ex = (int)((b >> 52) & 0x7ff);
  if (ex == 0) return 0;  // +-0 (two ints give no denormal)
  const uint64_t p = ((b & ((1ull << 52) - 1)) | (1ull << 52)) * 1000;
  const int s = 1075 - ex;  // x = mantissa * 2^-s
  if (s <= 0) return p << -s;  // |x| >= 2^52: not a quotient of two ints
  if (s > 63) return 0;
  const uint64_t q = p >> s, rem = p & ((1ull << s) - 1), half = 1ull << (s - 1);
  return q + (rem > half || (rem == half && (q & 1)));
}

// a record's or a mate's coordinates as mem_aln2sam rewrites them
struct SamCoord {
  int64_t pos;
  int32_t rid, is_rev, n_cigar;
};
// bwamem.c:844-852 on copies p and m of the record and its mate (mem_sam_pe always
// passes one): the line's flag bits, and the coordinates an unmapped end takes over
BWAGPU_HD inline int sam_flag(int flag, SamCoord* p, SamCoord* m) {
  flag |= 0x1;
  flag |= p->rid < 0 ? 0x4 : 0;
  flag |= m->rid < 0 ? 0x8 : 0;
  if (p->rid < 0 && m->rid >= 0) p->rid = m->rid, p->pos = m->pos, p->is_rev = m->is_rev, p->n_cigar = 0;
  if (m->rid < 0 && p->rid >= 0) m->rid = p->rid, m->pos = p->pos, m->is_rev = p->is_rev, m->n_cigar = 0;
  flag |= p->is_rev ? 0x10 : 0;
  flag |= m->is_rev ? 0x20 : 0;
  return flag;
}
// TLEN where p->rid == m->rid (bwamem.c:874-877); rlen = get_rlen of each CIGAR
BWAGPU_HD inline int64_t sam_tlen(const SamCoord& p, int p_rlen, const SamCoord& m, int m_rlen) {
  if (m.n_cigar == 0 || p.n_cigar == 0) return 0;
  const int64_t p0 = p.pos + (p.is_rev ? p_rlen - 1 : 0);
  const int64_t p1 = m.pos + (m.is_rev ? m_rlen - 1 : 0);
  return -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
}
// the clip rules.  Clips turn hard on a line with which > 0, without MEM_F_SOFTCLIP,
// of a non-ALT record (bwamem.c:830, 887, 901); add_cigar then prints which ? 'H' : 'S'
// for op 3 and 4 alike
BWAGPU_HD inline bool sam_clip_rewrite(int opt_flag, int is_alt) { return !(opt_flag & 0x200) && !is_alt; }
BWAGPU_HD inline int sam_cigar_op(int c, bool rewrite, int which) {
  return rewrite && (c == 3 || c == 4) ? (which ? 4 : 3) : c;
}
// SEQ / QUAL of a line are the read's [qb, qe), cut by the first and last op when
// they are clips and the line hard-clips (bwamem.c:886-890, 900-904); the two ends
// swap on the reverse strand.  n_cigar > 0.
BWAGPU_HD inline void sam_seq_range(int l_seq, bool cut, int is_rev, uint32_t first_op, uint32_t last_op, int* qb,
                                    int* qe) {
  int b = 0, e = l_seq;
  if (cut) {
    const int c5 = ((first_op & 0xf) == 4 || (first_op & 0xf) == 3) ? (int)(first_op >> 4) : 0;
    const int c3 = ((last_op & 0xf) == 4 || (last_op & 0xf) == 3) ? (int)(last_op >> 4) : 0;
    if (!is_rev) b += c5, e -= c3;
    else e -= c5, b += c3;
  }
  *qb = b, *qe = e;
}

}  // namespace bwagpu
