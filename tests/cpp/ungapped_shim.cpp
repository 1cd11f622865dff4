// ungapped_shim.cpp — the ungapped certificate (bwa-flow_amd/csrc/ungapped.h)
// over bare ksw_extend2 task lists, behind one C entry.  Plain C++: no HIP.
// tests/test_ungapped_cert.py builds it as a shared object and loads it with
// ctypes; tests/cpp/ungapped_asan.cpp includes it.
#include <stdint.h>

#include "bwagpu.h"
#include "ungapped.h"

// certified[k] = 1 and res[k] = the six outputs where task k holds the
// certificate (the call's own w, zdrop and h0; the band retry is
// mem_chain2aln's and no part of a bare call), else certified[k] = 0 and
// res[k] untouched.  -> the number of certified tasks
extern "C" int32_t ungapped_batch(const bwagpu_opt_t* opt, int32_t n_tasks, const bwagpu_ext_task_t* tasks,
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
    UngappedSide u;
    if (!ungapped_scan(t.qlen, max_mat, oe_min, [&](int i) { return (int)opt->mat[tg[i] * 5 + q[i]]; }, &u)) continue;
    const UngappedOut x = ungapped_result(t.h0, t.qlen, u);
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
