#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/post_<set>.npz, the expected results
of bwagpu_regs_post, made by the reference's own mem_sort_dedup_patch and
mem_mark_primary_se (oracle/_ref/libbwaref.so, loaded through ctypes).

    make -C oracle ref && python tools_dev/gen_post_fixture.py

Inputs: the raw regions (mem_chain2aln's output) of the chain sets c1_default,
c5_mixed, opt1_scoring, opt2_band, of a slice of the c5_refseed batch, of
chain_rep's reads (their chains extended by the reference's mem_chain2aln),
and of one new set, post_sv: 100/150/250 bp reads on both strands with 3-80 bp
deletions and insertions plus 600/1000 bp reads built so that mem_patch_reg
succeeds (sim_sv_reads says why the short ones cannot), seeded and extended by
the reference's own code against a bwa index of the golden genome built here
in a temporary directory.  post_rep_redun1 repeats chain_rep's heavy reads with
mask_level_redun = 1, the setting under which the second pass's identical hits
(bwamem.c:488-496) exist at all: at the default 0.95 two hits with the same
score, rb and qb always overlap by more than 95 % and the walk removes one.

Every fixture holds the options, the reads, the input regions per read, id0,
the ALT table, and the reference's output once for flags 1|2 and once for
1|2|4 (RegionsToSam::compute, src/Pipeline.cpp:560-575 and :612; the is_alt
loop of :570-574 is restated here, it is not in bwa).  Coverage counts come
from a walk of bwamem.c:450-497 in this script that calls the reference's own
sorts and mem_patch_reg and is checked against mem_sort_dedup_patch's result
for every read.  The script exits non-zero unless the floors below are met
over all fixtures together.
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import golden_io as G  # noqa: E402
import oracle  # noqa: E402
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Batch, compact  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
COVERAGE_KEYS = ("reads_lost_to_redundancy", "regs_patched", "regs_patched_rev", "pairs_gated_not_merged",
                 "reads_over_17", "reads_over_17_tied_re", "reads_identical_dropped", "reads_mixed_alt",
                 "regs_secondary")
FLOORS = dict(reads_lost_to_redundancy=20, regs_patched=20, regs_patched_rev=5, pairs_gated_not_merged=5,
              reads_over_17=5, reads_over_17_tied_re=1, reads_identical_dropped=5, reads_mixed_alt=10,
              regs_secondary=20)
MAX_BYTES = 1 << 20


class MemOpt(C.Structure):  # mem_opt_t, bwa/bwamem.h:26-58
    _fields_ = [("a", C.c_int), ("b", C.c_int), ("o_del", C.c_int), ("e_del", C.c_int), ("o_ins", C.c_int),
                ("e_ins", C.c_int), ("pen_unpaired", C.c_int), ("pen_clip5", C.c_int), ("pen_clip3", C.c_int),
                ("w", C.c_int), ("zdrop", C.c_int), ("max_mem_intv", C.c_uint64), ("T", C.c_int), ("flag", C.c_int),
                ("min_seed_len", C.c_int), ("min_chain_weight", C.c_int), ("max_chain_extend", C.c_int),
                ("split_factor", C.c_float), ("split_width", C.c_int), ("max_occ", C.c_int),
                ("max_chain_gap", C.c_int), ("n_threads", C.c_int), ("chunk_size", C.c_int),
                ("mask_level", C.c_float), ("drop_ratio", C.c_float), ("XA_drop_ratio", C.c_float),
                ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int),
                ("max_ins", C.c_int), ("max_matesw", C.c_int), ("max_XA_hits", C.c_int),
                ("max_XA_hits_alt", C.c_int), ("mat", C.c_int8 * 25)]


class BntAnn(C.Structure):  # bntann1_t, bwa/bntseq.h:36-45
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32),
                ("is_alt", C.c_int32), ("name", C.c_char_p), ("anno", C.c_char_p)]


class BntSeq(C.Structure):  # bntseq_t, bwa/bntseq.h:55-66
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(BntAnn)),
                ("n_holes", C.c_int32), ("ambs", C.c_void_p), ("fp_pac", C.c_void_p)]


class RefPost:
    """the reference's post-processing of one read, and the counting walk"""

    def __init__(self, opt: dict, popt, refd, alt):
        self.lib = lib = oracle.ref_lib()
        if lib is None:
            raise SystemExit("oracle/_ref/libbwaref.so missing: make -C oracle ref")
        lib.mem_opt_init.restype = C.POINTER(MemOpt)
        self.o = o = lib.mem_opt_init().contents
        for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_clip5", "pen_clip3", "w", "zdrop"):
            setattr(o, k, int(opt[k]))
        for i in range(25):
            o.mat[i] = int(opt["mat"][i])
        o.max_chain_gap, o.mask_level_redun, o.mask_level = int(popt[0]), float(popt[1]), float(popt[2])
        self.popt = (int(o.max_chain_gap), np.float32(o.mask_level_redun), np.float32(o.mask_level))
        self.l_pac = int(refd["l_pac"])
        self.pac = np.ascontiguousarray(refd["pac"], np.uint8)
        n = len(refd["ann_offset"])
        self.anns = (BntAnn * n)()
        for i in range(n):
            self.anns[i].offset, self.anns[i].len = int(refd["ann_offset"][i]), int(refd["ann_len"][i])
            self.anns[i].is_alt = int(alt[i])
            self.anns[i].name = b"c%d" % i
        self.bns = BntSeq(self.l_pac, n, 0, self.anns, 0, None, None)
        self.alt = np.asarray(alt, np.uint8)
        vp = C.c_void_p
        lib.mem_sort_dedup_patch.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, vp, C.c_int, vp]
        lib.mem_sort_dedup_patch.restype = C.c_int
        lib.mem_mark_primary_se.argtypes = [C.POINTER(MemOpt), C.c_int, vp, C.c_int64]
        lib.mem_mark_primary_se.restype = C.c_int
        lib.mem_patch_reg.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, vp, vp, vp, C.POINTER(C.c_int)]
        lib.mem_patch_reg.restype = C.c_int
        for f in ("ks_introsort_mem_ars2", "ks_introsort_mem_ars"):
            getattr(lib, f).argtypes = [C.c_size_t, vp]
            getattr(lib, f).restype = None

    def run(self, query, regs, rid_read, primary):
        """-> the reference's output regions of one read (Pipeline.cpp:562-574, then :612)"""
        a = np.array(regs, abi.ALNREG_DTYPE, order="C")
        q = np.array(query, np.uint8, order="C")
        m = len(a)
        if m:
            m = self.lib.mem_sort_dedup_patch(C.byref(self.o), C.byref(self.bns), self.pac.ctypes.data,
                                              q.ctypes.data, m, a.ctypes.data)
        assert np.array_equal(q, query), "the reference left the read reversed"
        a = a[:m].copy()
        for j in range(m):
            if a["rid"][j] >= 0 and self.alt[a["rid"][j]]:
                a["n_comp_is_alt"][j] = (a["n_comp_is_alt"][j] & np.uint32(0x3fffffff)) | np.uint32(1 << 30)
        if primary and m:
            self.lib.mem_mark_primary_se(C.byref(self.o), m, a.ctypes.data, int(rid_read))
        return a

    def gates(self, x, y):
        """mem_patch_reg's tests before the DP (bwamem.c:421-432), in Python"""
        if x["rb"] < self.l_pac <= y["rb"]:
            return False
        if x["qb"] >= y["qb"] or x["qe"] >= y["qe"] or x["re"] >= y["re"]:
            return False
        w = abs(int(x["re"] - y["rb"]) - int(x["qe"] - y["qb"]))
        r = abs(float(int(x["re"] - y["rb"])) / float(int(y["re"] - x["rb"]))
                - float(int(x["qe"] - y["qb"])) / float(int(y["qe"] - x["qb"])))
        ow = int(self.o.w)
        if x["re"] < y["rb"] or x["qe"] < y["qb"]:
            return not (w > ow << 1 or r >= float(np.float32(0.05)))
        return not (w > ow << 2 or r >= float(np.float32(0.05) * np.float32(2)))

    def walk(self, query, regs, want):
        """bwamem.c:450-497 with the reference's sorts and mem_patch_reg; -> event counts.
        `want`: mem_sort_dedup_patch's own result, which the walk must reproduce"""
        ev = dict(redundant=0, patched=0, gated_not_merged=0, identical=0, tied_re=0)
        n = len(regs)
        if n <= 1:
            return ev
        gap, red, _ = self.popt
        a = np.array(regs, abi.ALNREG_DTYPE, order="C")
        q = np.array(query, np.uint8, order="C")
        self.lib.ks_introsort_mem_ars2(n, a.ctypes.data)
        ev["tied_re"] = int(len(np.unique(a["re"])) < n)
        a["n_comp_is_alt"] = (a["n_comp_is_alt"] & np.uint32(0xc0000000)) | np.uint32(1)
        for i in range(1, n):
            p = a[i:i + 1]
            if p["rid"][0] != a["rid"][i - 1] or p["rb"][0] >= a["re"][i - 1] + gap:
                continue
            j = i - 1
            while j >= 0 and p["rid"][0] == a["rid"][j] and p["rb"][0] < a["re"][j] + gap:
                qq = a[j:j + 1]
                j -= 1
                if qq["qe"][0] == qq["qb"][0]:
                    continue
                P, Q = p[0], qq[0]
                orr = int(Q["re"] - P["rb"])
                oq = int(Q["qe"] - P["qb"]) if Q["qb"] < P["qb"] else int(P["qe"] - Q["qb"])
                mr = min(int(Q["re"] - Q["rb"]), int(P["re"] - P["rb"]))
                mq = min(int(Q["qe"] - Q["qb"]), int(P["qe"] - P["qb"]))
                if np.float32(orr) > red * np.float32(mr) and np.float32(oq) > red * np.float32(mq):
                    ev["redundant"] += 1
                    if P["score"] < Q["score"]:
                        p["qe"] = P["qb"]
                        break
                    qq["qe"] = Q["qb"]
                elif Q["rb"] < P["rb"]:
                    gated = self.gates(Q, P)
                    w = C.c_int(0)
                    sc = self.lib.mem_patch_reg(C.byref(self.o), C.byref(self.bns), self.pac.ctypes.data,
                                                q.ctypes.data, qq.ctypes.data, p.ctypes.data, C.byref(w))
                    assert gated or sc == 0, "a pair failed the gates in Python and merged in C"
                    if sc > 0:
                        ev["patched"] += 1
                        pc, qc = int(P["n_comp_is_alt"]), int(Q["n_comp_is_alt"])
                        p["n_comp_is_alt"] = (pc & 0xc0000000) | ((pc + (qc & 0x3fffffff) + 1) & 0x3fffffff)
                        p["seedcov"] = max(P["seedcov"], Q["seedcov"])
                        p["sub"] = max(P["sub"], Q["sub"])
                        p["csub"] = max(P["csub"], Q["csub"])
                        p["qb"], p["rb"] = Q["qb"], Q["rb"]
                        p["truesc"] = p["score"] = sc
                        p["w"] = w.value
                        qq["qb"] = Q["qe"]
                    elif gated:
                        ev["gated_not_merged"] += 1
        a = np.ascontiguousarray(a[a["qe"] > a["qb"]])
        m = len(a)
        self.lib.ks_introsort_mem_ars(m, a.ctypes.data)
        keep = np.ones(m, bool)
        for i in range(1, m):
            if a["score"][i] == a["score"][i - 1] and a["rb"][i] == a["rb"][i - 1] and a["qb"][i] == a["qb"][i - 1]:
                keep[i] = False
        ev["identical"] = int(m - keep.sum())
        a = a[keep]
        bad = G.region_mismatch(a, want)
        assert bad is None, "the counting walk differs from mem_sort_dedup_patch: " + bad
        return ev


def make_fixture(name, opt, popt, refd, genome, alt, seq_off, seq, regs_in, n_in, id0, out_dir, batch=None):
    """run the reference over every read; -> the fixture's coverage counts"""
    rp = RefPost(opt, popt, refd, alt)
    seq_off = np.asarray(seq_off, np.int64)
    n_in = np.asarray(n_in, np.int32)
    off = np.concatenate([[0], np.cumsum(n_in)]).astype(np.int64)
    cov = dict.fromkeys(COVERAGE_KEYS, 0)
    out3, out7, n3, n7 = [], [], [], []
    for r in range(len(n_in)):
        q = seq[seq_off[r]:seq_off[r + 1]]
        a = regs_in[off[r]:off[r + 1]]
        o3 = rp.run(q, a, id0 + r, False)
        o7 = rp.run(q, a, id0 + r, True)
        assert len(o3) == len(o7)
        out3.append(o3)
        out7.append(o7)
        n3.append(len(o3))
        n7.append(len(o7))
        want = o3.copy()  # mem_sort_dedup_patch's result: o3 without the ALT bit
        want["n_comp_is_alt"] &= np.uint32(0x3fffffff)
        ev = rp.walk(q, a, want)
        comp = o3["n_comp_is_alt"] & np.uint32(0x3fffffff)
        cov["reads_lost_to_redundancy"] += ev["redundant"] > 0
        cov["regs_patched"] += int((comp > 1).sum())
        cov["regs_patched_rev"] += int(((comp > 1) & (o3["rb"] >= rp.l_pac)).sum())
        cov["pairs_gated_not_merged"] += ev["gated_not_merged"]
        cov["reads_over_17"] += len(a) > 17
        cov["reads_over_17_tied_re"] += len(a) > 17 and ev["tied_re"]
        cov["reads_identical_dropped"] += ev["identical"] > 0
        n_alt = int((o7["n_comp_is_alt"] >> np.uint32(30) != 0).sum())
        cov["reads_mixed_alt"] += 0 < n_alt < len(o7)
        cov["regs_secondary"] += int((o7["secondary"] >= 0).sum())
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, abi.ALNREG_DTYPE)  # noqa: E731
    path = os.path.join(out_dir, f"post_{name}.npz")
    extra = {} if batch is None else dict(  # the chains the regions came from (the device entry's input)
        read_chain_off=batch.read_chain_off, chain_seed_off=batch.chain_seed_off, chain_rid=batch.chain_rid,
        chain_frac_rep=batch.chain_frac_rep, seeds=batch.seeds)
    np.savez_compressed(
        path, **extra, opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32), opt_mat=np.asarray(opt["mat"], np.int8),
        popt_gap=np.array([popt[0]], np.int32), popt_mask=np.array([popt[1], popt[2]], np.float32),
        genome=np.array([genome], np.int32), alt=np.asarray(alt, np.uint8), id0=np.array([id0], np.int64),
        flags=np.array([3, 7], np.int32), seq_off=seq_off, seq=np.asarray(seq, np.uint8), reg_n=n_in,
        regs=np.asarray(regs_in, abi.ALNREG_DTYPE), out3_n=np.array(n3, np.int32), out3_regs=cat(out3),
        out7_n=np.array(n7, np.int32), out7_regs=cat(out7),
        coverage=np.array([int(cov[k]) for k in COVERAGE_KEYS], np.int64))
    size = os.path.getsize(path)
    print(f"[gen_post] post_{name}: {len(n_in)} reads, {int(n_in.sum())} -> {sum(n3)} regions, {size} bytes, "
          f"{ {k: int(v) for k, v in cov.items()} }")
    if size > MAX_BYTES:
        raise SystemExit(f"post_{name}.npz is {size} bytes (> {MAX_BYTES})")
    return cov


def take_reads(batch: Batch, regs, n, reads):
    """(seq_off, seq, compact regions, counts) of a subset of a batch's reads"""
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    so = batch.seq_off
    seq = np.concatenate([batch.seq[so[r]:so[r + 1]] for r in reads])
    seq_off = np.concatenate([[0], np.cumsum([so[r + 1] - so[r] for r in reads])])
    rr = np.concatenate([regs[off[r]:off[r + 1]] for r in reads]) if len(reads) else regs[:0]
    return seq_off, seq, rr, np.asarray(n)[reads]


def genome_bases(refd):
    l_pac = int(refd["l_pac"])
    x = np.arange(l_pac, dtype=np.int64)
    return (refd["pac"][x >> 2] >> ((~x & 3) << 1).astype(np.uint8)) & 3


def build_index(refd, d):
    """the golden genome as FASTA and its bwa index (the reference's bwa_idx_build) -> prefix"""
    g = genome_bases(refd)
    fa = os.path.join(d, "ref.fa")
    with open(fa, "w") as f:
        for i, (o, ln) in enumerate(zip(refd["ann_offset"], refd["ann_len"])):
            s = np.array(list("ACGT"))[g[int(o):int(o) + int(ln)]]
            f.write(f">c{i}\n" + "".join(s.tolist()) + "\n")
    lib = oracle.ref_lib()
    lib.bwa_idx_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    lib.bwa_idx_build.restype = C.c_int
    lib.bwa_idx_build(fa.encode(), fa.encode(), 0, 10000000)
    pac = np.fromfile(fa + ".pac", np.uint8)
    if not np.array_equal(pac[:len(refd["pac"]) - 1], refd["pac"][:len(refd["pac"]) - 1]):
        raise SystemExit("the index built here is of another genome than tests/golden/ref.npz")
    return fa


def sim_sv_reads(refd, rng, n_reads, alt_contig):
    """post_sv's reads: windows of the golden genome on both strands with one deletion or
    insertion and 1 % substitutions, a third of them on the ALT contig.
    100/150/250 bp reads carry a 3-80 bp indel anywhere: the extension crosses the short
    ones from both sides (redundant hits) and the long ones fail mem_patch_reg's gates or
    its score ratio.  A patch that succeeds needs the indel to cost under 10 % of the
    predicted score, to stay under 5 % of the span (bwamem.c:431, 441) and a far piece too
    short for the extension to cross to it; no read of 250 bp can have all three, so every
    third read is 600 or 1000 bp with a 20-45 bp indel 19..d-1 bases from one end."""
    g = genome_bases(refd)
    seqs = []
    for k in range(n_reads):
        long_read = k % 3 == 1
        L = int(rng.choice([600, 1000])) if long_read else int(rng.choice([100, 150, 250]))
        c = alt_contig if k % 3 == 0 else int(rng.integers(0, len(refd["ann_len"])))
        if long_read:
            d = int(rng.integers(20, 29 if L == 600 else 46))
            f = int(rng.integers(19, d))
            a = L - f if rng.random() < 0.5 else f
        else:
            d = int(rng.choice([3, 8, 15, 20, 25, 30, 40, 50, 60, 80]))
            a = int(rng.integers(30, L - 30))
        p0 = int(refd["ann_offset"][c]) + int(rng.integers(0, int(refd["ann_len"][c]) - L - 100))
        if rng.random() < 0.6:  # deletion in the read
            read = np.concatenate([g[p0:p0 + a], g[p0 + a + d:p0 + d + L]])
        else:  # insertion
            if not long_read:
                d = min(d, L - a - 25)
            read = np.concatenate([g[p0:p0 + a], rng.integers(0, 4, d).astype(np.uint8), g[p0 + a:p0 + L - d]])
        read = read.astype(np.uint8).copy()
        sub = rng.random(len(read)) < (0.002 if long_read else 0.01)
        read[sub] = (read[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        if rng.random() < 0.5:
            read = (3 - read[::-1]).astype(np.uint8)
        seqs.append(read)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return seq_off, np.concatenate(seqs)


def main():
    out_dir = GOLD
    refd = G.load_ref()
    oref = oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])
    dflt = (10000, 0.95, 0.50)  # mem_opt_init, bwamem.c:62-72
    n_seqs = len(refd["ann_len"])
    total = dict.fromkeys(COVERAGE_KEYS, 0)

    def add(cov):
        for k in COVERAGE_KEYS:
            total[k] += int(cov[k])

    # the chain sets' own raw regions (golden genome), ALT contig rotating
    for i, name in enumerate(G.CHAIN_SETS):
        opt, b, regs, n = G.load_chain_set(name)
        alt = np.zeros(n_seqs, np.uint8)
        alt[i % n_seqs] = 1
        reads = np.arange(b.n_reads)
        add(make_fixture(name, opt, dflt, refd, 0, alt, *take_reads(b, regs, n, reads), 1000 * i, out_dir))

    # chain_rep: the reference's chains of repetitive reads, extended by its mem_chain2aln
    cg = G.load_chain_gold("rep")
    rco, chn, frac, sd = cg["final"]
    seeds = np.zeros(len(sd), abi.SEED_DTYPE)
    seeds["rbeg"], seeds["qbeg"], seeds["len"], seeds["score"] = sd[:, 0], sd[:, 1], sd[:, 2], sd[:, 3]
    cso = np.concatenate([[0], np.cumsum(chn[:, 2])])
    b = Batch(cg["seq_off"], cg["seq"], rco, cso, chn[:, 1], frac, seeds)
    regs, n, _ = oracle.chain2aln("ref", cg["opt"], oref, b)
    alt = np.zeros(n_seqs, np.uint8)
    alt[1] = 1
    popt = (cg["copt"]["max_chain_gap"], 0.95, cg["copt"]["mask_level"])
    add(make_fixture("chain_rep", cg["opt"], popt, refd, 0, alt,
                     *take_reads(b, compact(b, regs, n), n, np.arange(b.n_reads)), 77, out_dir))
    # the same reads with mask_level_redun = 1: hits of equal extent (or == mr) are then not
    # redundant in the walk, and the second sort's identical hits reach bwamem.c:488-496
    heavy = np.nonzero(n > 4)[0][:250]
    add(make_fixture("rep_redun1", cg["opt"], (popt[0], 1.0, popt[2]), refd, 0, alt,
                     *take_reads(b, compact(b, regs, n), n, heavy), 5, out_dir))

    # post_sv: simulated reads, seeded and extended by the reference
    rng = np.random.default_rng(20240611)
    with tempfile.TemporaryDirectory() as d:
        prefix = build_index(refd, d)
        seq_off, seq = sim_sv_reads(refd, rng, 900, 2)
        rco, rid, fr, cso, sd = oracle.ref_seqs2chains(prefix, seq_off, seq)
    b = Batch(seq_off, seq, rco, cso, rid, fr, sd)
    opt = abi.default_opt()
    regs, n, _ = oracle.chain2aln("ref", opt, oref, b)
    alt = np.zeros(n_seqs, np.uint8)
    alt[2] = 1
    add(make_fixture("sv", opt, dflt, refd, 0, alt, *take_reads(b, compact(b, regs, n), n, np.arange(b.n_reads)),
                     123456789, out_dir, batch=b))

    # c5_refseed: the reads of the mixed batch with the most regions (the chr21-sized genome)
    opt, gref, bs = workload.load_fixture(workload.C5_FIXTURE)
    b = bs[0].batch
    g = oracle.Ref(gref.l_pac, gref.ann_offset, gref.ann_len, gref.pac)
    regs, n, _ = oracle.chain2aln("ref", opt, g, b, n_threads=16)
    reads = np.sort(np.argsort(-n.astype(np.int64), kind="stable")[:1500])
    alt = np.zeros(len(gref.ann_len), np.uint8)
    alt[1] = 1
    gd = dict(l_pac=gref.l_pac, ann_offset=gref.ann_offset, ann_len=gref.ann_len, pac=gref.pac)
    add(make_fixture("c5_refseed", opt, dflt, gd, 1, alt, *take_reads(b, compact(b, regs, n), n, reads), 60000,
                     out_dir))

    print("[gen_post] coverage over all fixtures:", total)
    short = {k: (total[k], FLOORS[k]) for k in COVERAGE_KEYS if total[k] < FLOORS[k]}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")


if __name__ == "__main__":
    main()
