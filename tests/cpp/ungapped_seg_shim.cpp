// ungapped_seg_shim.cpp — the segment form of the ungapped certificate's
// diagonal scan (UngSeg / ungseg_combine in bwa-flow_amd/csrc/ungapped.h,
// DESIGN.md §26) behind C entries.  Plain C++: no HIP.
// tests/test_ungapped_seg.py builds it as a shared object and loads it with
// ctypes; tests/cpp/ungapped_seg_asan.cpp includes it.
#include <stdint.h>

#include <vector>

#include "bwagpu.h"
#include "ungapped.h"

// the serial scan of the scores s[0 .. n): out = {c, P, M, am}
extern "C" void ungseg_serial(const int32_t* s, int32_t n, int32_t max_mat, int32_t* out) {
  bwagpu::UngappedScan sc;
  for (int i = 0; i < n; ++i) sc.step(i, s[i], max_mat);
  out[0] = sc.c, out[1] = sc.P, out[2] = sc.M, out[3] = sc.am;
}

// the same scores cut into segments at cuts[0] < cuts[1] < ... (each in 1 ..
// n - 1), each segment folded from its bases, then the segments folded
// left-nested ((a b) c) d (order 0) or right-nested a (b (c d)) (order 1):
// out = {n, c, P, M, am}
extern "C" void ungseg_fold(const int32_t* s, int32_t n, int32_t max_mat, const int32_t* cuts, int32_t n_cuts,
                            int32_t order, int32_t* out) {
  using namespace bwagpu;
  std::vector<UngSeg> segs;
  int at = 0;
  for (int k = 0; k <= n_cuts; ++k) {
    const int end = k < n_cuts ? cuts[k] : n;
    UngSeg g;
    for (; at < end; ++at) g = ungseg_combine(g, ungseg_base(s[at], max_mat));
    segs.push_back(g);
  }
  UngSeg g;  // the empty segment: the identity on either side
  if (order == 0)
    for (size_t k = 0; k < segs.size(); ++k) g = ungseg_combine(g, segs[k]);
  else
    for (size_t k = segs.size(); k-- > 0;) g = ungseg_combine(segs[k], g);
  out[0] = g.n, out[1] = g.c, out[2] = g.P, out[3] = g.M, out[4] = g.am;
}

// ungapped_batch (ungapped_shim.cpp) with the diagonal summarised sixteen
// bases at a time and the summaries folded right-nested: certified[k] and
// res[k] as there.  -> the number of certified tasks
extern "C" int32_t ungseg_batch(const bwagpu_opt_t* opt, int32_t n_tasks, const bwagpu_ext_task_t* tasks,
                                const uint8_t* qpool, const uint8_t* tpool, bwagpu_ext_result_t* res,
                                uint8_t* certified) {
  using namespace bwagpu;
  int max_mat = 0;  // ksw.c:397-398: the maximum over the matrix, from 0
  for (int i = 0; i < 25; ++i) max_mat = opt->mat[i] > max_mat ? opt->mat[i] : max_mat;
  const int oe_min = ungapped_oe_min(opt->o_del, opt->e_del, opt->o_ins, opt->e_ins);
  int32_t n = 0;
  for (int32_t k = 0; k < n_tasks; ++k) {
    const bwagpu_ext_task_t& t = tasks[k];
    certified[k] = 0;
    if (!ungapped_call_ok(t.qlen, t.tlen, t.h0, t.w, t.zdrop, max_mat, oe_min)) continue;
    const uint8_t* q = qpool + t.qoff;
    const uint8_t* tg = tpool + t.toff;
    std::vector<UngSeg> segs;
    for (int base = 0; base < t.qlen; base += 16) {
      UngSeg g;
      for (int i = base; i < t.qlen && i < base + 16; ++i) g = ungseg_combine(g, ungseg_base(opt->mat[tg[i] * 5 + q[i]], max_mat));
      segs.push_back(g);
    }
    UngSeg g;
    for (size_t j = segs.size(); j-- > 0;) g = ungseg_combine(segs[j], g);
    if (g.dead(oe_min)) continue;
    const UngappedOut x = ungapped_result(t.h0, t.qlen, g.side());
    res[k].score = x.score;
    res[k].qle = x.qle;
    res[k].tle = x.tle;
    res[k].gtle = x.gtle;
    res[k].gscore = x.gscore;
    res[k].max_off = x.max_off;
    certified[k] = 1;
    ++n;
  }
  return n;
}
