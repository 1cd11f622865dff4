// global_dp.h — ksw_global2 (bwa/ksw.c:504-606) on one wave, shared by the
// CIGAR step (reg2aln.hip: with the direction matrix) and the region
// post-processing (regpost.hip: mem_patch_reg's score-only call, DIR = false).
#pragma once
#include <hip/hip_runtime.h>

#include "engine.h"
#include "wave_ops.h"

namespace bwagpu {
namespace {

constexpr int R2_NEG = -0x40000000;        // ksw.c:489 MINUS_INF
constexpr int R2_SENT = -(3 << 29);        // below every reachable scan value

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)((uint64_t)hi << 32 | lo);
}
__device__ __forceinline__ int wave_sum(int v) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return uni(v);
}
// query profile of base q: byte t = mat[t*5 + q] (t = reference base 0..3)
__device__ __forceinline__ uint32_t prof_word(const DevOpt& o, int q) {
  uint32_t p0 = o.qprof[0], p1 = o.qprof[1], p2 = o.qprof[2], p3 = o.qprof[3], p4 = o.qprof[4];
  asm volatile("" : "+s"(p0), "+s"(p1), "+s"(p2), "+s"(p3), "+s"(p4));
  uint32_t v = p0;
  v = q == 1 ? p1 : v;
  v = q == 2 ? p2 : v;
  v = q == 3 ? p3 : v;
  v = q == 4 ? p4 : v;
  return v;
}
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ksw_global2's DP over the wave (see the file comment); returns eh[qlen].h
template <int CD, bool DIR = true>
__device__ int global_dp(const DevOpt& o, int ql, const uint8_t* q, int tl, const uint8_t* r, int w, int ncol,
                         uint8_t* z, int64_t& cells) {
  const int lane = (int)(threadIdx.x & 63);
  const int e_del = o.e_del, e_ins = o.e_ins, oe_del = o.oe_del, oe_ins = o.oe_ins;
  int Hs[CD], Es[CD];
  uint32_t pf[CD];
#pragma unroll
  for (int c = 0; c < CD; ++c) {
    const int j = 64 * c + lane;
    pf[c] = prof_word(o, j < ql ? q[j] : 0);
    Hs[c] = j == 0 ? 0 : (j <= ql && j <= w ? -(o.o_ins + e_ins * j) : R2_NEG);
    Es[c] = R2_NEG;
  }
  int64_t ncells = 0;
  for (int i = 0; i < tl; ++i) {
    const int lo = i > w ? i - w : 0, hi = i + w + 1 < ql ? i + w + 1 : ql;
    const int sh = (r[i] & 3) << 3;
    const int h1init = lo == 0 ? -(o.o_del + e_del * (i + 1)) : R2_NEG;
    const int fdecay = R2_NEG + lo * e_ins;  // + (-j e_ins): F's start value decayed to column j
    uint8_t* zi = z + (size_t)i * ncol - lo;
    int M[CD], EX[CD];
    bool inb[CD];
    int carry = R2_SENT;
#pragma unroll
    for (int c = 0; c < CD; ++c) {
      const int j = 64 * c + lane;
      inb[c] = j >= lo && j < hi;
      M[c] = Hs[c] + __builtin_amdgcn_sbfe((int)pf[c], sh, 8);
      const int u = inb[c] ? M[c] - oe_ins + j * e_ins : R2_SENT;
      int x = c == 0 ? u : max(u, carry);
      x = max_bc31(max_bc15(max_shr8(max_shr4(max_shr2(max_shr1(x))))));
      EX[c] = dpp<DPP_WAVE_SHR1>(carry, x);
      if (c + 1 < CD) carry = __builtin_amdgcn_readlane(x, 63);
    }
    int prev63 = h1init;
#pragma unroll
    for (int c = 0; c < CD; ++c) {
      const int j = 64 * c + lane;
      const int m = M[c], e = Es[c];
      const int f = max(fdecay - j * e_ins, EX[c] - (j - 1) * e_ins);
      uint32_t d = m >= e ? 0u : 1u;
      int h = m >= e ? m : e;
      d = h >= f ? d : 2u;
      h = h >= f ? h : f;
      const int te = m - oe_del, ed = e - e_del;
      d |= ed > te ? 4u : 0u;
      const int tf = m - oe_ins, fd = f - e_ins;
      d |= fd > tf ? 32u : 0u;
      if (DIR && inb[c]) zi[j] = (uint8_t)d;
      // H(i, j-1) into slot j: lane 0 of segment 0 (and slot lo) takes h1init
      const int hsh = dpp<DPP_WAVE_SHR1>(prev63, h);
      if (c + 1 < CD) prev63 = __builtin_amdgcn_readlane(h, 63);
      const bool upd = (j >= lo && j <= hi) || j == hi;
      Hs[c] = upd ? (j <= lo ? h1init : hsh) : Hs[c];
      Es[c] = inb[c] ? (ed > te ? ed : te) : (j == hi ? R2_NEG : Es[c]);
    }
    ncells += hi > lo ? hi - lo : 0;
  }
  cells += ncells;
  // eh[qlen].h: slot ql lives in lane ql & 63 of segment ql >> 6
  int s = 0;
#pragma unroll
  for (int c = 0; c < CD; ++c) s = (ql >> 6) == c ? Hs[c] : s;
  return __builtin_amdgcn_readlane(s, ql & 63);
}

// The same DP in the BAND frame, for bands of 2w+1 <= 64 CDB columns: lane
// position p (segment c, p = 64c + lane) holds column j = i - w + p of row
// i, so the band never moves relative to the lanes.  Per row:
//  * M(i,j) needs H(i-1, j-1), which sits at the same position p of the
//    previous row: no shift; the query base of a position changes every row
//    (one LDS byte per lane);
//  * E(i,j) is the E written at column j by row i-1, one position up (p+1):
//    a one-lane shift down of the new E values, NEG entering at the top
//    (eh[end].e = MINUS_INF, ksw.c:569);
//  * eh[j+1].h for the next row is H(i, j) at the same position, except the
//    row's first slot, which takes h1 (ksw.c:533-534);
//  * eh[qlen].h, the score, is followed as a uniform value.
template <int CDB, bool DIR = true>
__device__ int band_dp(const DevOpt& o, int ql, const uint8_t* q, int tl, const uint8_t* r, int w, int ncol,
                       uint8_t* z, int64_t& cells) {
  const int lane = (int)(threadIdx.x & 63);
  const int e_del = o.e_del, e_ins = o.e_ins, oe_del = o.oe_del, oe_ins = o.oe_ins;
  int EH[CDB], EE[CDB];
#pragma unroll
  for (int c = 0; c < CDB; ++c) {
    const int j = 64 * c + lane - w;  // row 0
    EH[c] = j == 0 ? 0 : (j >= 1 && j <= ql && j <= w ? -(o.o_ins + e_ins * j) : R2_NEG);
    EE[c] = R2_NEG;
  }
  int sc = ql == 0 ? 0 : (ql <= w ? -(o.o_ins + e_ins * ql) : R2_NEG);  // eh[qlen].h
  int64_t ncells = 0;
  for (int i = 0; i < tl; ++i) {
    const int lo = i > w ? i - w : 0, hi = i + w + 1 < ql ? i + w + 1 : ql;
    const int sh = (r[i] & 3) << 3;
    const int h1init = lo == 0 ? -(o.o_del + e_del * (i + 1)) : R2_NEG;
    const int fdecay = R2_NEG + lo * e_ins;
    uint8_t* zi = z + (size_t)i * ncol - lo;
    int M[CDB], EX[CDB], J[CDB];
    bool inb[CDB];
    int carry = R2_SENT;
#pragma unroll
    for (int c = 0; c < CDB; ++c) {
      const int j = i - w + 64 * c + lane;
      J[c] = j;
      inb[c] = j >= lo && j < hi;
      const int qb = inb[c] ? q[j] : 0;
      M[c] = EH[c] + __builtin_amdgcn_sbfe((int)prof_word(o, qb), sh, 8);
      const int u = inb[c] ? M[c] - oe_ins + j * e_ins : R2_SENT;
      int x = c == 0 ? u : max(u, carry);
      x = max_bc31(max_bc15(max_shr8(max_shr4(max_shr2(max_shr1(x))))));
      EX[c] = dpp<DPP_WAVE_SHR1>(carry, x);
      if (c + 1 < CDB) carry = __builtin_amdgcn_readlane(x, 63);
    }
    int En[CDB], Hn[CDB];
#pragma unroll
    for (int c = 0; c < CDB; ++c) {
      const int j = J[c];
      const int m = M[c], e = EE[c];
      const int f = max(fdecay - j * e_ins, EX[c] - (j - 1) * e_ins);
      uint32_t d = m >= e ? 0u : 1u;
      int h = m >= e ? m : e;
      d = h >= f ? d : 2u;
      h = h >= f ? h : f;
      const int te = m - oe_del, ed = e - e_del;
      d |= ed > te ? 4u : 0u;
      const int tf = m - oe_ins, fd = f - e_ins;
      d |= fd > tf ? 32u : 0u;
      if (DIR && inb[c]) zi[j] = (uint8_t)d;
      Hn[c] = h;
      En[c] = inb[c] ? (ed > te ? ed : te) : R2_NEG;
    }
    // eh[qlen].h after this row (ksw.c:568): H(i, ql-1), or h1 when the band is empty
    if (hi == ql) {
      const int pq = ql - 1 - i + w;  // position of column ql-1
      int v = 0;
#pragma unroll
      for (int c = 0; c < CDB; ++c) v = (pq >> 6) == c ? Hn[c] : v;
      sc = lo < hi ? __builtin_amdgcn_readlane(v, pq & 63) : h1init;
    }
    // next row's frame: EH at the same position (h1 at column lo-1), EE one position down
    int nxt = R2_NEG;
#pragma unroll
    for (int c = CDB - 1; c >= 0; --c) {
      EH[c] = J[c] == lo - 1 ? h1init : Hn[c];
      const int dn = __builtin_amdgcn_mov_dpp(En[c], 0x130, 0xF, 0xF, false);  // wave_shl:1 (lane l <- l+1)
      EE[c] = lane == 63 ? nxt : dn;
      if (c > 0) nxt = __builtin_amdgcn_readlane(En[c], 0);
    }
    ncells += hi > lo ? hi - lo : 0;
  }
  cells += ncells;
  return sc;
}

}  // namespace
}  // namespace bwagpu
