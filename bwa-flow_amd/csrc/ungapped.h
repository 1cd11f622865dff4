// ungapped.h — ksw_extend2 calls that need no DP.  Plain C++,
// host and device in the way pure.h is: compiles without HIP.
//
// A seed is a maximal exact match, so a side usually begins with the mismatch
// that ended the seed and then matches to the end of the read.  Let s_i be the
// diagonal scores mat[t_i][q_i], i < qlen, c_i their running sum and
// P = sum (max_mat - s_i) the diagonal's deficit.  If P < oe_min =
// min(o_del + e_del, o_ins + e_ins), a cell (i, j) off the diagonal has at most
// min(i, j) + 1 aligned pairs and has paid a gap open, so it is strictly below
// the diagonal cell of its row: every row's maximum is its diagonal cell, with
// no tie, and no row past the query reaches the maximum or gscore.  Every
// output then follows from the c_i (ungapped_result).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BWAGPU_UNG_HD __host__ __device__
#else
#define BWAGPU_UNG_HD
#endif

namespace bwagpu {

// what a certified side leaves: everything but h0, which only shifts the scores
struct UngappedSide {
  int32_t M;   // max(0, max_i c_i)
  int32_t am;  // the first i with c_i = M, plus 1 (0 if M = 0): qle and tle
  int32_t cl;  // c_{qlen - 1}
};

// ksw_extend2's six outputs for a certified call that starts from h0
struct UngappedOut {
  int32_t score, qle, tle, gtle, gscore, max_off;
};

BWAGPU_UNG_HD inline int ungapped_oe_min(int o_del, int e_del, int o_ins, int e_ins) {
  const int d = o_del + e_del, i = o_ins + e_ins;
  return d < i ? d : i;
}

// the conditions on the call's parameters (the diagonal's own is ungapped_scan):
// the target covers the query; h0 and a positive z-drop are at least the
// cheapest gap (no diagonal cell falls to 0, no row that lags the maximum by
// P ends the call); a positive match score, so that c_i bounds what an
// off-diagonal cell can have collected
BWAGPU_UNG_HD inline bool ungapped_call_ok(int qlen, int tlen, int h0, int w, int zdrop, int max_mat, int oe_min) {
  return qlen >= 1 && tlen >= qlen && max_mat >= 1 && oe_min >= 1 && h0 >= oe_min && w >= 0 &&
         (zdrop <= 0 || zdrop >= oe_min);
}
// mem_chain2aln's band retry (MAX_BAND_TRY) ends after a first call with
// max_off = 0 only if the test max_off < (w >> 1) + (w >> 2) can hold
BWAGPU_UNG_HD inline bool ungapped_band_ok(int w) { return (w >> 1) + (w >> 2) > 0; }

// the diagonal, one base at a time: step(i, mat[t_i][q_i]) for i = 0 .. qlen - 1.
// P never falls (max_mat is the matrix's maximum), so `dead` may be looked at
// after any number of steps; a dead scan's side is not certified.
struct UngappedScan {
  int c = 0, P = 0, M = 0, am = 0;
  BWAGPU_UNG_HD void step(int i, int s, int max_mat) {
    P += max_mat - s;
    c += s;
    if (c > M) {
      M = c;
      am = i + 1;
    }
  }
  BWAGPU_UNG_HD bool dead(int oe_min) const { return P >= oe_min; }
  BWAGPU_UNG_HD UngappedSide side() const { return UngappedSide{M, am, c}; }
};

// score(i) = mat[t_i][q_i].  false as soon as P >= oe_min.
template <class Score>
BWAGPU_UNG_HD inline bool ungapped_scan(int qlen, int max_mat, int oe_min, Score score, UngappedSide* u) {
  UngappedScan sc;
  for (int i = 0; i < qlen; ++i) {
    sc.step(i, score(i), max_mat);
    if (sc.dead(oe_min)) return false;
  }
  *u = sc.side();
  return true;
}

// The same diagonal in pieces.  A segment is a run of n
// consecutive bases: c their score sum, P their deficit, M = max(0, the
// largest prefix sum inside the segment) and am the first index inside it that
// reaches M, plus 1 (0 if M = 0).  combine(a, b) is the segment a followed by
// b; it is associative and the empty segment is its identity, so a side's
// bases may be summarised sixteen at a time by different lanes and folded in
// order afterwards.  b's prefix sums start from a.c; its maximum replaces a's
// only where it is strictly larger, so the first index wins a tie as it does
// in UngappedScan::step.  A fold over the side's bases one at a time is that
// scan.  P adds and never falls: a dead prefix makes the whole side dead.
struct UngSeg {
  int32_t n = 0, c = 0, P = 0, M = 0, am = 0;
  BWAGPU_UNG_HD bool dead(int oe_min) const { return P >= oe_min; }
  BWAGPU_UNG_HD UngappedSide side() const { return UngappedSide{M, am, c}; }
};
BWAGPU_UNG_HD inline UngSeg ungseg_base(int s, int max_mat) {
  UngSeg g;
  g.n = 1;
  g.c = s;
  g.P = max_mat - s;
  g.M = s > 0 ? s : 0;
  g.am = s > 0 ? 1 : 0;
  return g;
}
BWAGPU_UNG_HD inline UngSeg ungseg_combine(const UngSeg& a, const UngSeg& b) {
  UngSeg g;
  g.n = a.n + b.n;
  g.c = a.c + b.c;
  g.P = a.P + b.P;
  const bool later = a.c + b.M > a.M;
  g.M = later ? a.c + b.M : a.M;
  g.am = later ? a.n + b.am : a.am;
  return g;
}

BWAGPU_UNG_HD inline UngappedOut ungapped_result(int h0, int qlen, const UngappedSide& u) {
  UngappedOut x;
  x.score = h0 + u.M;
  x.qle = x.tle = u.am;
  x.gscore = h0 + u.cl;
  x.gtle = qlen;
  x.max_off = 0;
  return x;
}

}  // namespace bwagpu
