"""Loader of tests/golden/post_<set>.npz (tools_dev/gen_post_fixture.py: the
reference's own mem_sort_dedup_patch / mem_mark_primary_se per read)."""
from __future__ import annotations

import functools
import os

import numpy as np

import golden_io as G
from bwagpu import abi
from bwagpu.engine import Batch
from golden_io import dense  # noqa: F401  (P.dense of the tests)

POST_SETS = ["c1_default", "c5_mixed", "opt1_scoring", "opt2_band", "chain_rep", "rep_redun1", "sv", "c5_refseed"]
COVERAGE_KEYS = ("reads_lost_to_redundancy", "regs_patched", "regs_patched_rev", "pairs_gated_not_merged",
                 "reads_over_17", "reads_over_17_tied_re", "reads_identical_dropped", "reads_mixed_alt",
                 "regs_secondary")
# the floors the generator enforces over all fixtures together
FLOORS = dict(reads_lost_to_redundancy=20, regs_patched=20, regs_patched_rev=5, pairs_gated_not_merged=5,
              reads_over_17=5, reads_over_17_tied_re=1, reads_identical_dropped=5, reads_mixed_alt=10,
              regs_secondary=20)


class PostSet:
    def __init__(self, name):
        z = np.load(os.path.join(G.GOLD, f"post_{name}.npz"), allow_pickle=False)
        self.name = name
        self.opt = G.opt_of(z)
        self.popt = abi.PostOpt(int(z["popt_gap"][0]), float(z["popt_mask"][0]), float(z["popt_mask"][1]), 0)
        self.genome = int(z["genome"][0])  # 0: tests/golden/ref.npz, 1: the chr21-sized golden genome
        self.alt = z["alt"]
        self.id0 = int(z["id0"][0])
        self.seq_off, self.seq = z["seq_off"], z["seq"]
        self.n = z["reg_n"].astype(np.int32)
        self.regs = z["regs"].astype(abi.ALNREG_DTYPE)
        self.off = G.offsets(self.n)
        # expected results by flags
        self.want = {3: (z["out3_regs"].astype(abi.ALNREG_DTYPE), z["out3_n"].astype(np.int32)),
                     7: (z["out7_regs"].astype(abi.ALNREG_DTYPE), z["out7_n"].astype(np.int32))}
        self.coverage = dict(zip(COVERAGE_KEYS, z["coverage"].tolist()))
        self.batch = None
        if "seeds" in z.files:
            self.batch = Batch(self.seq_off, self.seq, z["read_chain_off"], z["chain_seed_off"], z["chain_rid"],
                               z["chain_frac_rep"], z["seeds"].astype(abi.SEED_DTYPE))


@functools.lru_cache(maxsize=None)
def load(name) -> PostSet:
    return PostSet(name)


@functools.lru_cache(maxsize=None)
def genome(kind: int) -> dict:
    """l_pac / ann_offset / ann_len / pac of a fixture's genome"""
    if kind == 0:
        return G.load_ref()
    from bwagpu import workload
    _, ref, _ = workload.load_fixture(workload.C5_FIXTURE)
    return dict(l_pac=int(ref.l_pac), ann_offset=ref.ann_offset, ann_len=ref.ann_len, pac=ref.pac)
