#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/grch_<stage>_<set>.npz, the expected
results of the region post-processing, mate rescue, pair selection and alignment
records at GRCh38 coordinates, made by the reference's own functions
(oracle/_ref/libbwaref.so through ctypes: RefPost / RefPair / RefSel of the three
small-genome generators).

    make -C oracle ref && python tools_dev/gen_grch_pair_fixture.py

The inputs are the small-genome fixtures' (post_*, rescue_*, pair_split on
tests/golden/ref.npz) translated by tests/grch_io.py into the composite genome
"ref.npz's genome, 195 GRCh38-shaped contigs, ref.npz's genome again": even
pairs in copy A (reverse strand past 2^32), odd pairs in copy B (both strands
between 2^31 and 2^32).  The reference's functions need the contig table and the
0.78 GB pac only, no index.  The observing walk of mem_matesw reads its windows
through LazyStrands; the two strands of 3.1 Gbases are never materialised.

Per set the file holds the digests of the pac and of the translated inputs, and
the expected outputs as full records.  `cross` is hand-built (grch_io.cross_input):
64 pairs with read 1 in copy A and read 2 in copy B.  The pair stage of every
rescue set runs on the reference's post-rescue regions here, as gen_pair_fixture
does on the small genome.

The script counts, per set, how many pairs' answers differ from the plain
translation of the small-genome fixture's answers (the reference's answer stands),
asserts that mem_pestat's statistics equal the small-genome ones, and exits
non-zero unless grch_io.FLOORS are met over all sets together."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"), HERE):
    sys.path.insert(0, p)

import golden_io as G  # noqa: E402
import grch_io as GI  # noqa: E402
import oracle  # noqa: E402
import pair_io as P  # noqa: E402
import post_io as PO  # noqa: E402
import rescue_io as R  # noqa: E402
from bwagpu import abi  # noqa: E402
from gen_pair_fixture import SELOPT_KEYS_F, SELOPT_KEYS_I, RefSel, select_pairs  # noqa: E402
from gen_post_fixture import RefPost  # noqa: E402
from gen_rescue_fixture import HEADROOM, PAIROPT_KEYS, rescue_pairs  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MAX_BYTES = 1 << 20
CROSS_PAIR_ID0 = GI.CROSS_PAIR_ID0


class LazyStrands:
    """bns_get_seq's two strands of a genome, decoded from the pac one slice [rb:re) at a time"""

    def __init__(self, refd):
        self.pac, self.l_pac = refd["pac"], int(refd["l_pac"])

    def __getitem__(self, s):
        x = np.arange(s.start, s.stop, dtype=np.int64)
        fwd = x < self.l_pac
        p = np.where(fwd, x, 2 * self.l_pac - 1 - x)
        b = (self.pac[p >> 2] >> ((~p & 3) << 1).astype(np.uint8)) & 3
        return np.where(fwd, b, 3 - b).astype(np.uint8)


class GrchSel(RefSel):
    strands = staticmethod(LazyStrands)


def pairopt_dict(s):
    z = s._z_pairopt
    po = dict(zip(PAIROPT_KEYS, [int(x) for x in z["pairopt_int"]]))
    po["mask_level_redun"], po["mask_level"] = float(z["pairopt_mask"][0]), float(z["pairopt_mask"][1])
    return po


def per_read(regs, n):
    off = G.offsets(n)
    return [regs[o:o + k] for o, k in zip(off, n)]


def pairs_differing(n_reads, *columns):
    """how many pairs differ in any of the (got, want, per-read counts or None for per-pair arrays) columns"""
    bad = np.zeros(n_reads // 2, bool)
    for got, want, n in columns:
        if n is None:
            bad |= np.array([got[p].tobytes() != want[p].tobytes() for p in range(n_reads // 2)])
            continue
        off = np.concatenate([G.offsets(n), [int(np.sum(n))]])
        if len(got) != len(want):
            return n_reads // 2
        for p in range(n_reads // 2):
            bad[p] |= got[off[2 * p]:off[2 * p + 2]].tobytes() != want[off[2 * p]:off[2 * p + 2]].tobytes()
    return int(bad.sum())


def input_counts(cov, regs, rids):
    rb = regs["rb"].astype(np.int64)
    cov["in_rb_ge_2^32"] += int((rb >= 1 << 32).sum())
    cov["in_rb_2^31_to_2^32"] += int(((rb >= 1 << 31) & (rb < 1 << 32)).sum())
    rids.update(np.unique(regs["rid"]).tolist())


def save(kind, name, cov, rids, **arrays):
    path = os.path.join(GOLD, f"grch_{kind}_{name}.npz")
    np.savez_compressed(path, pac_sha256=np.frombuffer(GI.composite().pac_sha256, np.uint8),
                        coverage=np.array([int(cov[k]) for k in GI.COVERAGE_KEYS], np.int64),
                        rids=np.array(sorted(rids), np.int32), **arrays)
    size = os.path.getsize(path)
    print(f"[gen_grch] grch_{kind}_{name}: {size} bytes, { {k: int(v) for k, v in cov.items() if v} }", flush=True)
    if size > MAX_BYTES:
        raise SystemExit(f"grch_{kind}_{name}.npz is {size} bytes (> {MAX_BYTES})")
    return cov


def sha(b):
    return np.frombuffer(b, np.uint8)


# ---------------------------------------------------------------- the three stages
def post_expected(s, reads=None):
    """the reference's mem_sort_dedup_patch (+ mem_mark_primary_se) per read of a translated post set"""
    rp = RefPost(s.opt, (s.popt.max_chain_gap, s.popt.mask_level_redun, s.popt.mask_level), GI.composite().genome, s.alt)
    out = {3: [], 7: []}
    for r in range(len(s.n)) if reads is None else reads:
        q = s.seq[s.seq_off[r]:s.seq_off[r + 1]]
        a = s.regs[s.off[r]:s.off[r] + s.n[r]]
        out[3].append(rp.run(q, a, s.id0 + r, False))
        out[7].append(rp.run(q, a, s.id0 + r, True))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, abi.ALNREG_DTYPE)  # noqa: E731
    return {f: (cat(v), np.array([len(a) for a in v], np.int32)) for f, v in out.items()}


def make_post(name):
    c = GI.composite()
    s, small = GI.post_input(name), PO.load(name)
    cov, rids = dict.fromkeys(GI.COVERAGE_KEYS, 0), set()
    input_counts(cov, s.regs, rids)
    want = post_expected(s)
    o3, n3 = want[3]
    patched = (o3["n_comp_is_alt"] & np.uint32(0x3fffffff)) > 1
    in_b = c.copy_b(n3)
    cov["patched_copy_a"], cov["patched_copy_b"] = int((patched & ~in_b).sum()), int((patched & in_b).sum())
    cov["patched_rev"] = int((patched & (o3["rb"] >= c.l_pac)).sum())
    nr = len(s.n) & ~1
    cov["differ_from_translation"] = pairs_differing(
        nr, *[(want[f][0], c.translate(small.want[f][0], c.copy_b(small.want[f][1])), want[f][1]) for f in (3, 7)])
    return save("post", name, cov, rids, in_sha256=sha(s.in_sha256), out3_n=n3, out3_regs=o3, out7_n=want[7][1],
                out7_regs=want[7][0])


def rescue_expected(s, pes, n_pairs=None, per_pair=None):
    """the reference's rescue loop over the first n_pairs pairs (all) of a translated rescue set under pes"""
    po = pairopt_dict(s)
    rs = GrchSel(s.opt, po, s.genome, s.alt)
    nr = s.n_reads if n_pairs is None else 2 * n_pairs
    regs = per_read(s.regs, s.n)[:nr]
    out, out_n, n_sw, peak_n, _ = rescue_pairs(s.name, rs, po, pes, s.seq_off, s.seq, regs, per_pair)
    return np.concatenate(out), np.array(out_n, np.int32), np.array(n_sw, np.int32), np.array(peak_n, np.int32)


def make_rescue(name, fr_pes=None):
    c = GI.composite()
    s = GI.rescue_input(name)
    cov, rids = dict.fromkeys(GI.COVERAGE_KEYS, 0), set()
    input_counts(cov, s.regs, rids)
    rs = GrchSel(s.opt, pairopt_dict(s), s.genome, s.alt)
    pes_own = rs.pestat(per_read(s.regs, s.n))
    if name == GI.CROSS:
        assert (pes_own["failed"] == 1).all(), "mem_pestat counted a pair across the two copies"
        pes = fr_pes
    else:
        assert pes_own.tobytes() == s.small.pes.tobytes(), f"{name}: pes differs from the small genome's"
        pes = pes_own
    ev = []
    out, out_n, n_sw, peak_n = rescue_expected(s, pes, per_pair=ev)
    assert (peak_n - s.n <= HEADROOM).all()
    for p, e in enumerate(ev):  # pair p's copy is p & 1, except in `cross`, whose windows lie beside read 1 and read 2
        if name == GI.CROSS:
            continue
        ab = "b" if p & 1 else "a"
        cov["windows_changed_copy_" + ab] += int(e["windows_changed"])
        cov["added_rb_2^31_to_2^32" if p & 1 else "added_rb_ge_2^32"] += int(e["regs_added"] if p & 1 else e["regs_added_rev"])
    if s.small is not None:
        cov["differ_from_translation"] = pairs_differing(
            s.n_reads, (out, c.translate(s.small.out_regs, c.copy_b(s.small.out_n)), out_n),
            (n_sw, s.small.n_sw, None))
    save("rescue", name, cov, rids, in_sha256=sha(s.in_sha256), pes=pes, pes_own=pes_own, out_n=out_n, out_regs=out,
         n_sw=n_sw, peak_n=peak_n)
    return cov, pes


def make_pair(name):
    c = GI.composite()
    regs, n, pes, alt, opt, pid0, small = GI.pair_input(name)
    cov, rids = dict.fromkeys(GI.COVERAGE_KEYS, 0), set()
    if name == "split":
        input_counts(cov, regs, rids)
        po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
                  mask_level_redun=0.95, mask_level=0.50)
        seqs = [np.random.default_rng(r).integers(0, 4, 150).astype(np.uint8) for r in range(len(n))]
    else:
        s = GI.load_rescue(name)
        po = pairopt_dict(s)
        seqs = [s.seq[s.seq_off[r]:s.seq_off[r + 1]] for r in range(s.n_reads)]
    rs = GrchSel(opt, po, c.genome, alt)
    res, _ = select_pairs(name, rs, pes, seqs, per_read(regs, n), pid0)
    proper = res["sel"]["branch"] == abi.SEL_PAIRED
    if name != GI.CROSS:
        cov["proper_copy_a"], cov["proper_copy_b"] = int(proper[0::2].sum()), int(proper[1::2].sum())
    if small is not None:
        in_b = c.copy_b(small.n)
        cov["differ_from_translation"] = pairs_differing(
            len(n), (res["marked"], c.translate(small.marked, in_b), n), (res["final"], c.translate(small.final, in_b), n),
            (res["sel"], small.sel[0], None), (res["sel_nopair"], small.sel[1], None),
            (res["out_mapq"], small.out_mapq[0], n), (res["out_mapq_nopair"], small.out_mapq[1], n))
    o = rs.o
    return save("pair", name, cov, rids, in_sha256=sha(GI.digest(n, regs, pes, alt)), pair_id0=np.array([pid0], np.int64),
                selopt_int=np.array([getattr(o, k) for k in SELOPT_KEYS_I], np.int32),
                selopt_f=np.array([getattr(o, k) for k in SELOPT_KEYS_F], np.float32), **res)


def make_aln():
    """the reference's mem_reg2aln on every region the selection of `ends` emits"""
    c = GI.composite()
    d, s = GI.load_pair(GI.ALN_SET), GI.load_rescue(GI.ALN_SET)
    jobs = GI.aln_jobs(d.off, d.final, d.n, d.out_mapq[0], s.seq_off)
    g = c.genome
    ref = oracle.Ref(g["l_pac"], g["ann_offset"], g["ann_len"], g["pac"])
    exp, cig, md = oracle.reg2aln("ref", d.opt, ref, jobs, s.seq, GI.ALN_MAX_OPS, GI.ALN_MAX_MD)
    assert (exp["status"] == abi.ALN_OK).sum() > len(jobs) // 2 and (exp["status"] != abi.ALN_OVERFLOW).all()
    cov = dict.fromkeys(GI.COVERAGE_KEYS, 0)
    ops = np.concatenate([cig[k, :exp["n_cigar"][k]] for k in range(len(jobs))])
    mds = np.concatenate([md[k, :exp["md_len"][k]] for k in range(len(jobs))])
    return save("aln", GI.ALN_SET, cov, set(exp["rid"].tolist()), in_sha256=sha(GI.digest(jobs, s.seq)), exp=exp,
                cig_ops=ops, md=mds)


def main():
    total = dict.fromkeys(GI.COVERAGE_KEYS, 0)

    def add(cov):
        for k in GI.COVERAGE_KEYS:
            total[k] += int(cov[k])

    for name in GI.POST_SETS:
        add(make_post(name))
    fr_pes = None
    for name in GI.RESCUE_SETS + [GI.CROSS]:
        cov, pes = make_rescue(name, fr_pes)
        add(cov)
        if name == "fr":
            fr_pes = pes
    GI.load_rescue.cache_clear()
    for name in GI.PAIR_SETS + [GI.CROSS]:
        add(make_pair(name))
    GI.load_pair.cache_clear()
    make_aln()
    rids = GI.all_rids()
    print("[gen_grch] coverage over all sets:", total, "contigs:", sorted(rids))
    short = {k: (total[k], f) for k, f in GI.FLOORS.items() if total[k] < f}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")
    if not GI.contigs_ok(rids):
        raise SystemExit(f"contigs {sorted(rids)}: fewer than {GI.MIN_CONTIGS}, or from one end of the table only")


if __name__ == "__main__":
    main()
