"""Loader of tests/golden/rescue_<set>.npz and rescue_pestat_cases.npz
(tools_dev/gen_rescue_fixture.py: the reference's own mem_pestat and mem_matesw
over simulated paired-end libraries; reads 2i and 2i+1 are pair i)."""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_io as G
from bwagpu import abi
from golden_io import dense, offsets  # noqa: F401  (R.dense, R.offsets of the tests and the generators)

RESCUE_SETS = ["fr", "mixed", "shift", "ends", "rep", "rep_sw2"]
COVERAGE_KEYS = ("pairs_sw", "regs_added", "regs_added_rev", "regs_added_to_empty", "sw_no_region", "dedup_removed",
                 "windows_changed", "windows_rejected", "pairs_multi_cand", "calls_cut", "pairs_multi_orient",
                 "spec_ignored", "reads_over_17", "needed_not_speculated")
# the floors the generator enforces over all sets together (needed_not_speculated has none)
FLOORS = dict(pairs_sw=200, regs_added=100, regs_added_rev=30, regs_added_to_empty=30, sw_no_region=20,
              dedup_removed=10, windows_changed=10, windows_rejected=5, pairs_multi_cand=20, calls_cut=5,
              pairs_multi_orient=20, spec_ignored=5, reads_over_17=1)
PESTAT_CASES = ["all_under_min_cnt", "exactly_10", "failed_by_ratio", "two_alive", "is_zero", "over_max_ins",
                "low_clamped", "cal_sub", "other_contig", "odd_n_reads", "n_reads_0", "no_regions"]


def pairopt_of(z, max_rounds=3) -> abi.PairOpt:
    i, m = z["pairopt_int"], z["pairopt_mask"]
    return abi.PairOpt(int(i[0]), int(i[1]), int(i[2]), int(i[3]), int(i[4]), float(m[0]), float(m[1]), max_rounds)


class RescueSet:
    def __init__(self, name):
        z = np.load(os.path.join(G.GOLD, f"rescue_{name}.npz"), allow_pickle=False)
        self.name = name
        self.opt = G.opt_of(z)
        self._z_pairopt = dict(pairopt_int=z["pairopt_int"].copy(), pairopt_mask=z["pairopt_mask"].copy())
        self.genome_id = int(z["genome"][0])  # 0: tests/golden/ref.npz, 2: the set's own genome (g_*)
        if self.genome_id == 0:
            self.genome = G.load_ref()
        else:
            self.genome = dict(l_pac=int(z["g_l_pac"][0]), ann_offset=z["g_ann_offset"], ann_len=z["g_ann_len"],
                               pac=z["g_pac"])
        self.alt = z["alt"]
        self.seq_off, self.seq = z["seq_off"], z["seq"]
        self.n = z["reg_n"].astype(np.int32)
        self.regs = z["regs"].astype(abi.ALNREG_DTYPE)
        self.off = offsets(self.n)
        self.pes = z["pes"].astype(abi.PESTAT_DTYPE)
        self.out_n = z["out_n"].astype(np.int32)
        self.out_regs = z["out_regs"].astype(abi.ALNREG_DTYPE)
        self.n_sw = z["n_sw"].astype(np.int32)
        self.peak_n = z["peak_n"].astype(np.int32)  # the longest a read's vector gets (before a dedup)
        self.coverage = dict(zip(COVERAGE_KEYS, z["coverage"].tolist()))

    @property
    def n_reads(self):
        return len(self.n)

    def pairopt(self, max_rounds=3) -> abi.PairOpt:
        return pairopt_of(self._z_pairopt, max_rounds)

    def out_off(self, headroom):
        """output spans of n + headroom regions per read -> int64[n_reads + 1]"""
        return np.concatenate([[0], np.cumsum(self.n.astype(np.int64) + headroom)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def load(name) -> RescueSet:
    return RescueSet(name)


@functools.lru_cache(maxsize=None)
def load_cases():
    """-> (opt, PairOpt, {name: (n int32[n_reads], regs, pes PESTAT_DTYPE[4])})"""
    z = np.load(os.path.join(G.GOLD, "rescue_pestat_cases.npz"), allow_pickle=False)
    cases = {str(k): (z[f"{k}_n"].astype(np.int32), z[f"{k}_regs"].astype(abi.ALNREG_DTYPE),
                      z[f"{k}_pes"].astype(abi.PESTAT_DTYPE)) for k in z["names"]}
    return G.opt_of(z), pairopt_of(z), cases
