"""The post / rescue / pair fixtures in the GRCh38 regime (tests/golden/grch_*.npz,
tools_dev/gen_grch_pair_fixture.py): the sets of post_io / rescue_io / pair_io on
tests/golden/ref.npz translated into "ref.npz's genome, 195 GRCh38-shaped contigs,
ref.npz's genome again" (workload.GoldenInGrch38, 201 contigs, l_pac 3.1e9), with the
reference's own answers there.

Even pairs go to copy A (contigs 0-2: forward coordinates unchanged, the reverse
strand past 2^32), odd pairs to copy B (contigs 198-200: both strands between 2^31
and 2^32); both mates of a pair land in the same copy.  Reads, offsets, pair ids and
every other field stay as they are.  The fixtures hold the digest of the genome's pac
and of the translated inputs they were made from, and the loaders refuse when what is
regenerated here differs."""
from __future__ import annotations

import copy
import functools
import hashlib
import os

import numpy as np

import golden_io as G
import pair_io as P
import post_io as PO
import rescue_io as R
from bwagpu import abi

GENOME_ID = 38  # the genome key of the translated sets (0-2 are the small genomes)
POST_SETS = ["sv", "chain_rep", "c1_default"]
RESCUE_SETS = ["fr", "mixed", "ends", "shift"]
PAIR_SETS = RESCUE_SETS + ["split"]
CROSS = "cross"
N_CROSS, CROSS_PAIR_ID0 = 64, 31
ALN_SET, ALN_MAX_OPS, ALN_MAX_MD = "ends", 64, 512
COVERAGE_KEYS = ("in_rb_ge_2^32", "in_rb_2^31_to_2^32", "added_rb_ge_2^32", "added_rb_2^31_to_2^32", "patched_copy_a",
                 "patched_copy_b", "patched_rev", "windows_changed_copy_a", "windows_changed_copy_b", "proper_copy_a",
                 "proper_copy_b", "differ_from_translation")
# over all sets together (differ_from_translation is recorded, it has no floor)
FLOORS = {"in_rb_ge_2^32": 500, "in_rb_2^31_to_2^32": 500, "added_rb_ge_2^32": 30, "added_rb_2^31_to_2^32": 30,
          "patched_copy_a": 15, "patched_copy_b": 15, "patched_rev": 10, "windows_changed_copy_a": 3,
          "windows_changed_copy_b": 3, "proper_copy_a": 300, "proper_copy_b": 300}
MIN_CONTIGS = 5  # distinct rid over all inputs, from both ends of the contig table


class Composite:
    """the composite genome as the engines and the generators take it"""

    def __init__(self):
        from bwagpu import workload
        from bwagpu.synth import Grch38Ref
        small = G.load_ref()
        g = workload.GoldenInGrch38(Grch38Ref(38), as_object(small))
        self.l_small, self.l_pac, self.off_b, self.rid_b = int(g.lg), int(g.l_pac), int(g.off_b), int(g.rid_b)
        self.n_small = len(small["ann_len"])
        self.genome = dict(l_pac=self.l_pac, ann_offset=g.ann_offset, ann_len=g.ann_len, pac=g.pac)
        self.pac_sha256 = hashlib.sha256(g.pac).digest()

    def alt(self, alt_small):
        """[alt, zeros(195), alt]"""
        a = np.asarray(alt_small, np.uint8)
        return np.concatenate([a, np.zeros(self.rid_b - self.n_small, np.uint8), a])

    def copy_b(self, n):
        """per region: does its read's pair go to copy B"""
        return np.repeat(((np.arange(len(n)) >> 1) & 1).astype(bool), np.asarray(n, np.int64))

    def translate(self, regs, in_b):
        """regions on the small genome -> the same regions here; in_b per region (or one bool)"""
        out = np.array(regs, abi.ALNREG_DTYPE)
        rb = out["rb"].astype(np.int64)
        # the strand of rb chooses the shift of both ends: re == l_small of a forward region stays an end
        shift = np.where(in_b, self.off_b, np.where(rb >= self.l_small, 2 * (self.l_pac - self.l_small), 0))
        out["rb"] = rb + shift
        out["re"] = out["re"].astype(np.int64) + shift
        out["rid"] = np.where(np.asarray(in_b) & (out["rid"] >= 0), out["rid"] + self.rid_b, out["rid"])
        return out


def as_object(refd):
    """ref.npz's dict as the object with l_pac / ann_offset / ann_len / pac that GoldenInGrch38 reads"""
    class Small:
        pass
    s = Small()
    s.l_pac, s.ann_offset, s.ann_len, s.pac = refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"]
    return s


@functools.lru_cache(maxsize=None)
def composite() -> Composite:
    """built once per session (0.78 GB of pac)"""
    return Composite()


def digest(*arrays) -> bytes:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
    return h.digest()


# ---------------------------------------------------------------- translated inputs (no fixture needed)
def post_input(name):
    """post_<name> translated: its PostSet with regs, alt and genome replaced (the expected results are not)"""
    c = composite()
    s = copy.copy(PO.load(name))
    s.regs = c.translate(s.regs, c.copy_b(s.n))
    s.alt, s.genome, s.want = c.alt(s.alt), GENOME_ID, None
    s.in_sha256 = digest(s.seq_off, s.seq, s.n, s.regs, s.alt)
    return s


def rescue_input(name):
    """rescue_<name> translated (or the hand-built `cross`): a RescueSet without expected results"""
    c = composite()
    if name == CROSS:
        return cross_input()
    s = copy.copy(R.load(name))
    assert s.genome_id == 0
    s.small = R.load(name)
    s.regs = c.translate(s.regs, c.copy_b(s.n))
    s.alt, s.genome, s.genome_id = c.alt(s.alt), c.genome, GENOME_ID
    s.pes = s.out_n = s.out_regs = s.n_sw = s.peak_n = None
    s.in_sha256 = digest(s.seq_off, s.seq, s.n, s.regs, s.alt)
    return s


def cross_input():
    """64 pairs whose mates lie 3.1e9 bases apart: read 1 is `fr` pair k's first read in copy A, read 2 the
    second read of `fr` pair k + 64 in copy B (another fragment: nothing to rescue beside read 1 either).
    Their rid differ and their distance exceeds 2^31."""
    c = composite()
    fr = R.load("fr")
    both = (fr.n[0::2] > 0) & (fr.n[1::2] > 0)
    ks = [k for k in range(len(both) - N_CROSS) if both[k] and both[k + N_CROSS]][:N_CROSS]
    assert len(ks) == N_CROSS
    reads = [r for k in ks for r in (2 * k, 2 * (k + N_CROSS) + 1)]
    s = copy.copy(fr)
    s.name, s.small = CROSS, None
    s.n = fr.n[reads]
    s.off = R.offsets(s.n)
    s.seq_off = np.concatenate([[0], np.cumsum([fr.seq_off[r + 1] - fr.seq_off[r] for r in reads])]).astype(np.int64)
    s.seq = np.concatenate([fr.seq[fr.seq_off[r]:fr.seq_off[r + 1]] for r in reads])
    regs = np.concatenate([fr.regs[fr.off[r]:fr.off[r] + fr.n[r]] for r in reads])
    s.regs = c.translate(regs, np.repeat((np.arange(len(reads)) & 1).astype(bool), s.n))
    s.alt, s.genome, s.genome_id = c.alt(fr.alt), c.genome, GENOME_ID
    s.pes = s.out_n = s.out_regs = s.n_sw = s.peak_n = None
    s.in_sha256 = digest(s.seq_off, s.seq, s.n, s.regs, s.alt)
    return s


def split_input():
    """pair_split's unmarked regions translated -> (regs, n, pes, alt)"""
    c = composite()
    d = P.load("split")
    return c.translate(d.regs, c.copy_b(d.n)), d.n, d.pes, c.alt(d.alt)


# ---------------------------------------------------------------- fixtures
def _npz(kind, name):
    path = os.path.join(G.GOLD, f"grch_{kind}_{name}.npz")
    z = np.load(path, allow_pickle=False)
    if z["pac_sha256"].tobytes() != composite().pac_sha256:
        raise RuntimeError(f"{os.path.basename(path)}: the regenerated composite genome differs from the fixture's")
    return z


def _check_input(z, kind, name, sha):
    if z["in_sha256"].tobytes() != sha:
        raise RuntimeError(f"grch_{kind}_{name}.npz: the translated inputs differ from the ones the reference ran on")


def coverage_of(z) -> dict:
    return dict(zip(COVERAGE_KEYS, z["coverage"].tolist()))


@functools.lru_cache(maxsize=None)
def load_post(name):
    s = post_input(name)
    z = _npz("post", name)
    _check_input(z, "post", name, s.in_sha256)
    s.want = {3: (z["out3_regs"].astype(abi.ALNREG_DTYPE), z["out3_n"].astype(np.int32)),
              7: (z["out7_regs"].astype(abi.ALNREG_DTYPE), z["out7_n"].astype(np.int32))}
    s.coverage = coverage_of(z)
    return s


@functools.lru_cache(maxsize=None)
def load_rescue(name):
    """`cross` carries two statistics: pes_own, mem_pestat's answer on the set itself (every orientation
    failed), and pes, the translated `fr` library's, under which its rescue and its selection ran"""
    s = rescue_input(name)
    z = _npz("rescue", name)
    _check_input(z, "rescue", name, s.in_sha256)
    s.pes = z["pes"].astype(abi.PESTAT_DTYPE)
    s.pes_own = z["pes_own"].astype(abi.PESTAT_DTYPE)
    s.out_n = z["out_n"].astype(np.int32)
    s.out_regs = z["out_regs"].astype(abi.ALNREG_DTYPE)
    s.n_sw, s.peak_n = z["n_sw"].astype(np.int32), z["peak_n"].astype(np.int32)
    s.coverage = coverage_of(z)
    return s


def pair_input(name):
    """-> (unmarked regions, n, pes, alt, opt, pair_id0, the small set's PairData or None)"""
    if name == "split":
        regs, n, pes, alt = split_input()
        d = P.load("split")
        return regs, n, pes, alt, d.opt, d.pair_id0, d
    s = load_rescue(name)
    regs = R.dense(s.out_regs, R.offsets(s.out_n), s.out_n)
    if name == CROSS:
        return regs, s.out_n, s.pes, s.alt, s.opt, CROSS_PAIR_ID0, None
    d = P.load(name)
    return regs, s.out_n, s.pes, s.alt, s.opt, d.pair_id0, d


@functools.lru_cache(maxsize=None)
def load_pair(name) -> P.PairData:
    regs, n, pes, alt, opt, pid0, _ = pair_input(name)
    z = _npz("pair", name)
    _check_input(z, "pair", name, digest(n, regs, pes, alt))
    assert int(z["pair_id0"][0]) == pid0 and np.array_equal(z["n"], n)
    d = P.PairData(name, z, "", regs, pes, opt, composite().genome, GENOME_ID, alt)
    d.coverage = coverage_of(z)
    return d


@functools.lru_cache(maxsize=None)
def load_aln():
    """the reference's mem_reg2aln on the regions the selection of `ends` emits (out_mapq >= 0, read order)
    -> (jobs, records, CIGAR ops per job, MD bytes per job)"""
    z = _npz("aln", ALN_SET)
    d, s = load_pair(ALN_SET), load_rescue(ALN_SET)
    jobs = aln_jobs(d.off, d.final, d.n, d.out_mapq[0], s.seq_off)
    _check_input(z, "aln", ALN_SET, digest(jobs, s.seq))
    exp = z["exp"].astype(abi.ALN_DTYPE)
    ops = [z["cig_ops"][o:o + k] for o, k in zip(G.offsets(exp["n_cigar"]), exp["n_cigar"])]
    mds = [bytes(z["md"][o:o + k]) for o, k in zip(G.offsets(exp["md_len"]), exp["md_len"])]
    return jobs, exp, ops, mds


def aln_jobs(off, regs, n, select, seq_off):
    """the mem_reg2aln jobs of a selection: one per region with select >= 0, in read order"""
    rd = np.repeat(np.arange(len(n)), np.asarray(n, np.int64))
    c = R.dense(regs, off, n)
    keep = R.dense(select, off, n) >= 0
    c, rd = c[keep], rd[keep]
    jobs = np.zeros(len(c), abi.REG2ALN_TASK_DTYPE)
    for f in ("rb", "re", "qb", "qe", "truesc", "w"):
        jobs[f] = c[f]
    jobs["qoff"] = np.asarray(seq_off)[rd]
    jobs["l_seq"] = np.asarray(seq_off)[rd + 1] - np.asarray(seq_off)[rd]
    return jobs


def all_files():
    return [f"grch_post_{n}.npz" for n in POST_SETS] + [f"grch_rescue_{n}.npz" for n in RESCUE_SETS + [CROSS]] + \
        [f"grch_pair_{n}.npz" for n in PAIR_SETS + [CROSS]] + [f"grch_aln_{ALN_SET}.npz"]


def all_rids() -> set:
    """every contig an input region of a fixture lies in"""
    rids = set()
    for f in all_files():
        rids.update(np.load(os.path.join(G.GOLD, f), allow_pickle=False)["rids"].tolist())
    return rids


def contigs_ok(rids) -> bool:
    c = composite()
    return len(rids) >= MIN_CONTIGS and min(rids) < c.n_small and max(rids) >= c.rid_b
