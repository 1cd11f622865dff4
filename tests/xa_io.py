"""Loader of tests/golden/xa_select.npz (tools_dev/gen_xa_fixture.py: the number
of hits in the XA:Z field of every record the reference's own mem_sam_pe prints,
on the pair sets and on hand-built cases), and mem_gen_alt's selection
(bwa/bwamem_extra.c:90-118) restated in numpy, which the generator pins against
those strings hit by hit."""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_io as G
import pair_io as P
from bwagpu import abi

SETS = ["rep", "rep_sw2", "mixed", "ends"]
CASES = ["at_cap", "over_cap", "alt_lifts_cap", "ratio_80_81", "primary_below_T", "two_strings"]
COVERAGE_KEYS = ("lines_with_xa", "hits", "strings_over_cap", "strings_alt_lifted", "hits_under_ratio",
                 "strings_unprinted")
FLOORS = dict(lines_with_xa=50, hits=100, strings_over_cap=5, strings_alt_lifted=10, hits_under_ratio=20,
              strings_unprinted=1)


def xa_read(a, om, done, mate, xopt):
    """one read: regions a, out_mapq om -> (xa_of, job_select, events)"""
    n = len(a)
    ratio = float(np.float32(xopt.XA_drop_ratio))  # the float option in a double parameter
    sa, sc = a["secondary_all"].astype(np.int64), a["score"].astype(np.int64)
    alt = (a["n_comp_is_alt"] >> np.uint32(30)) != 0
    pri = np.full(n, -1, np.int64)
    ev = dict.fromkeys(COVERAGE_KEYS, 0)
    xa_of, job = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    if not done:
        return xa_of, job, ev
    for i in range(n):
        k = int(sa[i])
        if 0 <= k < n:
            if float(sc[i]) >= float(sc[k]) * ratio:
                pri[i] = k
            else:
                ev["hits_under_ratio"] += 1
    for r in np.unique(pri[pri >= 0]):
        members = np.nonzero(pri == r)[0]
        cnt, has_alt = len(members), bool(alt[members].any())
        if cnt > xopt.max_XA_hits_alt or (not has_alt and cnt > xopt.max_XA_hits):
            ev["strings_over_cap"] += 1
            continue
        ev["strings_alt_lifted"] += cnt > xopt.max_XA_hits
        if om[r] < 0:
            ev["strings_unprinted"] += 1
            continue
        xa_of[members] = r
        ev["lines_with_xa"] += 1
        ev["hits"] += cnt
    job[(om >= 0) | (xa_of >= 0)] = 0
    if 0 <= mate < n:
        job[mate] = 0
    return xa_of, job, ev


def xa_model(off, regs, n, sel, out_mapq, xopt=None):
    """-> xa_of, job_select parallel to regs (-1 outside the reads' spans too), summed events"""
    xopt = abi.default_samopt() if xopt is None else xopt
    xa_of, job = np.full(len(regs), -1, np.int32), np.full(len(regs), -1, np.int32)
    tot = dict.fromkeys(COVERAGE_KEYS, 0)
    for r in range(len(n)):
        s = sel[r >> 1]
        done = int(s["status"]) == abi.SEL_DONE
        mate = int(s["z"][r & 1]) if done and int(s["branch"]) == abi.SEL_NO_PAIRING else -1
        lo, hi = int(off[r]), int(off[r]) + int(n[r])
        xa_of[lo:hi], job[lo:hi], ev = xa_read(regs[lo:hi], out_mapq[lo:hi], done, mate, xopt)
        for k in COVERAGE_KEYS:
            tot[k] += int(ev[k])
    return xa_of, job, tot


class XaData:
    """one batch: the regions as the selection leaves them, sel and out_mapq by mode (0 pairing,
    1 MEM_F_NOPAIRING), and xa_cnt by mode: parallel to the regions, the number of hits in the
    reference's XA:Z field of the region's record, -1 for a region without a record"""

    def __init__(self, name, n, regs, sel, out_mapq, xa_cnt, genome, opt, alt):
        self.name, self.n, self.regs, self.sel, self.out_mapq, self.xa_cnt = name, n, regs, sel, out_mapq, xa_cnt
        self.off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if len(n) else np.zeros(0, np.int64)
        self.genome, self.opt, self.alt = genome, opt, alt

    @property
    def n_reads(self):
        return len(self.n)


def _file():
    return np.load(os.path.join(G.GOLD, "xa_select.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def coverage() -> dict:
    return dict(zip(COVERAGE_KEYS, _file()["coverage"].tolist()))


@functools.lru_cache(maxsize=None)
def load(name) -> XaData:
    z, d = _file(), P.load(name)
    cnt = {0: z[name + "_xa_cnt"].astype(np.int32), 1: z[name + "_xa_cnt_nopair"].astype(np.int32)}
    return XaData(name, d.n, {0: d.final, 1: d.marked}, d.sel, d.out_mapq, cnt, d.genome, d.opt, d.alt)


@functools.lru_cache(maxsize=None)
def load_cases() -> XaData:
    """the hand-built pairs as one batch; pair p is CASES[p]"""
    z = _file()
    assert [str(k) for k in z["case_names"]] == CASES
    pre = "cases_"
    return XaData("cases", z[pre + "n"].astype(np.int32),
                  {0: z[pre + "final"].astype(abi.ALNREG_DTYPE), 1: z[pre + "marked"].astype(abi.ALNREG_DTYPE)},
                  {0: z[pre + "sel"].astype(abi.PAIRSEL_DTYPE), 1: z[pre + "sel_nopair"].astype(abi.PAIRSEL_DTYPE)},
                  {0: z[pre + "out_mapq"].astype(np.int32), 1: z[pre + "out_mapq_nopair"].astype(np.int32)},
                  {0: z[pre + "xa_cnt"].astype(np.int32), 1: z[pre + "xa_cnt_nopair"].astype(np.int32)},
                  G.load_ref(), G.opt_of(z), z["alt"])
