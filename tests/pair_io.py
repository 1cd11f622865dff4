"""Loader of tests/golden/pair_<set>.npz and pair_cases.npz
(tools_dev/gen_pair_fixture.py: the reference's own mem_mark_primary_se,
mem_pair and mem_approx_mapq_se over the post-rescue regions of the rescue
sets and over one library simulated at the level of regions, `split`; reads 2i
and 2i+1 are pair i)."""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_io as G
import rescue_io as R
from bwagpu import abi

PAIR_SETS = R.RESCUE_SETS + ["split"]
COVERAGE_KEYS = ("proper", "no_primary", "is_multi", "unpaired_preferred", "pair0_with_primaries", "z_nonzero",
                 "switched", "n_sub_pos", "csub_over_sub", "hash_ties", "alt_emitted", "reads_mixed_alt",
                 "reads_over_17", "two_live")
# the floors the generator enforces over all sets together
FLOORS = dict(is_multi=20, unpaired_preferred=20, pair0_with_primaries=20, z_nonzero=100, switched=100, hash_ties=10,
              alt_emitted=10, reads_mixed_alt=50, two_live=1)
CASES = ["n0_n0", "n0_n1", "n1_n1", "n2_n1", "n2_n2", "only_alt", "n16", "n17", "n64", "n65", "n_cap", "n_cap_plus_1",
         "pri_cap_plus_1", "all_failed", "dist_at_low_high", "score_0", "sub_ge_score", "two_live_rf"]


def selopt_of(z, flags=0) -> abi.SelOpt:
    i, f = z["selopt_int"], z["selopt_f"]
    return abi.SelOpt(int(i[0]), int(i[1]), int(i[2]), float(f[0]), int(i[3]), float(f[1]), float(f[2]), int(flags))


class PairData:
    """one batch of pairs: the unmarked regions, the marked ones, and the selection with and without MEM_F_NOPAIRING"""

    def __init__(self, name, z, pre, regs, pes, opt, genome, genome_id, alt):
        self.name, self.opt, self.genome, self.genome_id, self.alt = name, opt, genome, genome_id, alt
        self._sel = dict(selopt_int=z["selopt_int"].copy(), selopt_f=z["selopt_f"].copy())
        self.pair_id0 = int(z["pair_id0"][0])
        self.pes = pes.astype(abi.PESTAT_DTYPE)
        self.n = z[pre + "n"].astype(np.int32)
        self.off = R.offsets(self.n)
        self.regs = regs.astype(abi.ALNREG_DTYPE)              # as the rescue leaves them
        self.n_pri = z[pre + "n_pri"].astype(np.int32)
        self.marked = z[pre + "marked"].astype(abi.ALNREG_DTYPE)  # after mem_mark_primary_se, id = 2 * pair id + r
        self.final = z[pre + "final"].astype(abi.ALNREG_DTYPE)    # after the selection (NOPAIRING leaves `marked`)
        self.sel = {0: z[pre + "sel"].astype(abi.PAIRSEL_DTYPE), 1: z[pre + "sel_nopair"].astype(abi.PAIRSEL_DTYPE)}
        self.out_mapq = {0: z[pre + "out_mapq"].astype(np.int32), 1: z[pre + "out_mapq_nopair"].astype(np.int32)}

    @property
    def n_reads(self):
        return len(self.n)

    def selopt(self, flags=0) -> abi.SelOpt:
        return selopt_of(self._sel, flags)


@functools.lru_cache(maxsize=None)
def load(name) -> PairData:
    z = np.load(os.path.join(G.GOLD, f"pair_{name}.npz"), allow_pickle=False)
    if name == "split":
        d = PairData(name, z, "", z["in_regs"], z["pes"], G.opt_of(z), G.load_ref(), 0, z["alt"])
    else:
        s = R.load(name)
        d = PairData(name, z, "", R.dense(s.out_regs, R.offsets(s.out_n), s.out_n), s.pes, s.opt, s.genome,
                     s.genome_id, s.alt)
        assert np.array_equal(d.n, s.out_n)
    d.coverage = dict(zip(COVERAGE_KEYS, z["coverage"].tolist()))
    return d


@functools.lru_cache(maxsize=None)
def load_cases() -> dict:
    z = np.load(os.path.join(G.GOLD, "pair_cases.npz"), allow_pickle=False)
    assert [str(k) for k in z["names"]] == CASES
    return {k: PairData(k, z, k + "_", z[k + "_regs"], z[k + "_pes"], G.opt_of(z), G.load_ref(), 0, z["alt"])
            for k in CASES}
