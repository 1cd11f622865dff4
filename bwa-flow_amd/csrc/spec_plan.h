// spec_plan.h — which extension kernel each length bin of the speculative
// mem_chain2aln runs (spec.hip's launch_ext_round), decided in one place.
// Plain C++: compiles without HIP (tests/cpp/ext_plan_asan.cpp).  engine.h
// includes it.
#pragma once
#include <stddef.h>

#include <algorithm>

#include "pure.h"

namespace bwagpu {

// extension task lists: 3 length classes (kernel columns per lane) x 3 rounds
constexpr int kSpecBins = 3;  // lq <= 160 / <= 256 / <= 1023
// (160: the pair kernel's first bin needs CPL <= 5 = 160 / 32; 2x150 reads all fall in it)
constexpr int kSpecBinLen[kSpecBins] = {160, 256, 1023};

constexpr int kSideLds = 96;  // LDS bytes of one parked SideTask (spec.hip)
// the short phase's groups and columns: eight lanes, queries up to 63
constexpr int kShortG = 8, kShortPmax = 8, kShortQMax = kShortG * kShortPmax - 1;

// LDS of one wave of the side kernel: 64 / g groups of two target row buffers,
// two states and two query buffers
inline size_t side4_wave_lds(int tb_bytes, int g, int pmax) {
  return (size_t)(64 / g) * (2 * (size_t)tb_bytes + 2 * kSideLds + 2 * (size_t)pmax * g);
}

// the threshold a launch runs with: 0 where the short run's buffers (rows for
// queries up to short_q, as tb_bytes_for sizes them) would not fit the block's
// LDS; -> the LDS bytes of one wave, the larger of the two runs' needs
inline int side_short_plan(const DevOpt& o, int tb_bytes, int g, int pmax, int short_q, int* tb_short,
                           size_t* wave_lds) {
  const size_t w1 = side4_wave_lds(tb_bytes, g, pmax);
  *tb_short = 0;
  *wave_lds = w1;
  short_q = std::min(std::max(short_q, 0), kShortQMax);
  if (short_q == 0) return 0;
  const int tbs = tb_bytes_for(o, short_q);
  const size_t w2 = (side4_wave_lds(tbs, kShortG, kShortPmax) + 15) & ~(size_t)15;
  if ((size_t)(kBlock / 64) * std::max(w1, w2) > 64 * 1024) return 0;
  *tb_short = tbs;
  *wave_lds = std::max(w1, w2);
  return short_q;
}

// The first two length bins' extension kernels for a context of extension form
// `form` (bwagpu_ctx_ext_form: 0 = default, 1 = two seeds per wave, 2 = four
// per wave), target row buffers of tb_bytes and the short-side threshold
// short_q (bwagpu_ctx_ext_short).  quad: every score of both bins fits the
// packed 16-bit DP (extend_quad); key8: the first bin's fit its 8-bit row-max key.
//
//   bin  condition              kernel                        code
//   0    quad, key8, form 0     spec_side4_kernel<16,10,true>   18
//   0    quad, key8, form 2     spec_side4_kernel<32,5,true>    14
//   0    quad, not key8         spec_side4_kernel<32,8,false>   15
//   0    not quad               spec_ext2_kernel<5>              2
//   1    quad, form 0           spec_ext4_kernel<16,16,false>
//   1    quad, form 2           spec_ext4_kernel<32,8,false>
//   1    not quad               spec_ext2_kernel<8>
//
// EXT2: two seeds per wave, 32-bit DP.  EXT4: 128 / G seeds per wave, both
// sides of a seed by one task state machine.  SIDE4: phased, every left call
// then every right call (two launches), 128 / G calls per wave.  The third bin
// (reads over 256 bp) always runs spec_ext_kernel<16>.  `code` is what
// bwagpu_debug_ext_kernel reports (the first bin only; Engine.EXT_KERNELS
// names it).  The second bin stays on the task state machine: its calls run
// ~250 rows, so the tail of each side launch cost more than the phasing saved
// (DESIGN.md §3 round 6).
enum ExtFamily { EXT2 = 0, EXT4 = 1, SIDE4 = 2 };
struct ExtBin {
  int family, G, PMAX;
  bool K8;
  int code;     // 0: none (the second bin)
  bool phased;  // its list is sorted one per side by query length (spec_sort2_*), else in pair order (spec_sort_*)
};
struct ExtPlan {
  bool quad;
  ExtBin bin[2];
  // the first bin's side launches (SIDE4): the short phase's effective threshold
  // (0: off; only the eight-per-wave form has one), its target row bytes, and
  // the LDS bytes of one wave
  int short_q, tb_short;
  size_t wave_lds;
};

inline ExtPlan ext_plan(const DevOpt& o, int form, int tb_bytes, int short_q) {
  ExtPlan p{};
  p.quad = form != 1 && quad_scores_ok(o, kSpecBinLen[1]) && quad_rows_ok(o, tb_bytes);
  if (!p.quad) {
    p.bin[0] = {EXT2, 32, kSpecBinLen[0] / 32, false, 2, false};
    p.bin[1] = {EXT2, 32, kSpecBinLen[1] / 32, false, 0, false};
    return p;
  }
  if (!quad_key8_ok(o, kSpecBinLen[0])) p.bin[0] = {SIDE4, 32, kSpecBinLen[1] / 32, false, 15, true};
  else if (form == 0) p.bin[0] = {SIDE4, 16, kSpecBinLen[0] / 16, true, 18, true};
  else p.bin[0] = {SIDE4, 32, kSpecBinLen[0] / 32, true, 14, true};
  if (form == 0) p.bin[1] = {EXT4, 16, kSpecBinLen[1] / 16, false, 0, false};
  else p.bin[1] = {EXT4, 32, kSpecBinLen[1] / 32, false, 0, false};
  const ExtBin& s = p.bin[0];
  p.short_q = side_short_plan(o, tb_bytes, s.G, s.PMAX, s.G == 16 && s.K8 ? short_q : 0, &p.tb_short, &p.wave_lds);
  return p;
}

}  // namespace bwagpu
