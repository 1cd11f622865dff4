#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/sam_text_<set>.npz, the expected output of
bwagpu_sam_text_device, made by the reference's own mem_sam_pe and mem_aln2sam
(oracle/_ref/libbwaref.so, loaded through ctypes).

    make -C oracle ref && python tools_dev/gen_sam_fixture.py

(a) mem_sam_pe with MEM_F_NO_RESCUE, with and without MEM_F_NOPAIRING, over the
pairs of the sets of tests/xa_io.py (only read) and over hand-built pairs, and
once more over one set and the hand-built pairs under MEM_F_SOFTCLIP | MEM_F_XB.
Read names, qualities, comments, contig names and bwa_rg_id come from the
formulas of tests/sam_io.py, so only the text is stored: whole for as many
leading reads as fit 1 MiB, a 16-byte blake2b digest per read after that.
(b) mem_aln2sam called directly on hand-built mem_aln_t lists for what reads do
not reach (CIGARs of 1 to 200 ops, reads of 1 to 250 bases on both strands,
positions past 2^32, MD of 1 and max_md - 1 bytes, no qualities); stored with
every array that makes the stage build those lists.
The script exits non-zero under the coverage floors of sam_io.FLOORS or when a
file is over 1 MiB.  No line is restated.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"), HERE):
    sys.path.insert(0, p)

import golden_io as G  # noqa: E402
import pair_io as PIO  # noqa: E402
import rescue_io as RIO  # noqa: E402
import sam_io as S  # noqa: E402
import xa_io as X  # noqa: E402
from bwagpu import abi  # noqa: E402
from gen_pair_fixture import (F_NO_RESCUE, F_NOPAIRING, PAIR_ID0, BSeq, MemAln, cat_regs, hand_pes, reg)  # noqa: E402
from gen_post_fixture import BntSeq, MemOpt  # noqa: E402
from gen_rescue_fixture import AlnRegV, libc  # noqa: E402
from gen_xa_fixture import PO, RefXa  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


class KString(C.Structure):
    _fields_ = [("l", C.c_size_t), ("m", C.c_size_t), ("s", C.c_void_p)]


class RefSam(RefXa):
    """the reference with sam_io's contig names and read group"""

    def __init__(self, *a):
        super().__init__(*a)
        self.names = [S.contig_name(i) for i in range(self.rp.bns.n_seqs)]
        for i, nm in enumerate(self.names):
            self.rp.anns[i].name = nm
        rg = (C.c_char * 256).in_dll(self.lib, "bwa_rg_id")
        rg.value = S.RG_ID
        self.lib.mem_aln2sam.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), C.POINTER(KString), C.POINTER(BSeq),
                                         C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.mem_aln2sam.restype = None

    def sam_pair(self, tag, p, seqs, a_raw, pes, pid, mode, flags):
        """mem_sam_pe without rescue on pair p -> the bytes of s[0].sam, s[1].sam"""
        o = self.o
        saved = o.flag
        o.flag = F_NO_RESCUE | (F_NOPAIRING if mode else 0) | flags
        s = (BSeq * 2)()
        keep = []
        v = (AlnRegV * 2)()
        for i in range(2):
            r = 2 * p + i
            q = np.ascontiguousarray(seqs[i], np.uint8)
            ql = C.create_string_buffer(S.read_qual(r, len(q)).tobytes())
            com = S.read_comment(r)
            keep += [q, ql]
            s[i].l_seq, s[i].name, s[i].seq, s[i].qual = len(q), S.pair_name(tag, p), q.ctypes.data, C.addressof(ql)
            s[i].comment = com if com else None
            t = self.to_v(np.ascontiguousarray(a_raw[i]))
            v[i].n, v[i].m, v[i].a = t.n, t.m, t.a
        self.lib.mem_sam_pe(C.byref(o), C.byref(self.rp.bns), self.rp.pac.ctypes.data, pes.ctypes.data, int(pid),
                            C.cast(s, C.c_void_p), C.cast(v, C.c_void_p))
        o.flag = saved
        out = []
        for i in range(2):
            out.append(C.string_at(s[i].sam))
            libc.free(s[i].sam)
            libc.free(v[i].a)
        return out


def pack(texts, n_full):
    off, text = S.blob(texts[:n_full])
    dig = np.frombuffer(b"".join(S.digest(t) for t in texts[n_full:]), np.uint8).reshape(-1, 16)
    return off, text, dig


def save_fitting(path, fixed, runs):
    """runs: key -> the reads' texts.  Whole text for as many leading pairs as fit MAX_BYTES"""
    n_reads = len(next(iter(runs.values())))
    n_full = n_reads
    while True:
        arrays = dict(fixed)
        for key, texts in runs.items():
            off, text, dig = pack(texts, n_full)
            arrays.update({key + "_off": off, key + "_text": text, key + "_digest": dig,
                           key + "_n_lines": np.array([t.count(b"\n") for t in texts], np.int32)})
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        if size <= S.MAX_BYTES:
            print(f"[gen_sam] {os.path.basename(path)}: {size} bytes, whole text for {n_full} of {n_reads} reads",
                  flush=True)
            return
        if n_full == 0:
            raise SystemExit(f"{path} is {size} bytes (> {S.MAX_BYTES}) even without text")
        n_full = int(n_full * 0.85) & ~1


def run_batch(tag, rs, d, seqs, raw, pes, pid0, keys):
    """every key's run over the batch -> ({key: texts}, coverage)"""
    ev = dict.fromkeys(S.COVERAGE_KEYS, 0)
    runs = {}
    for key in keys:
        mode, flags = S.KEYS[key]
        sel, om = d.sel[mode], d.out_mapq[mode]
        texts = []
        for p in range(d.n_reads // 2):
            assert int(sel[p]["status"]) == abi.SEL_DONE, f"{tag} pair {p}"
            both = rs.sam_pair(tag, p, seqs[2 * p:2 * p + 2], raw[2 * p:2 * p + 2], pes, pid0 + p, mode, flags)
            for i, t in enumerate(both):
                r = 2 * p + i
                n_rec = int((om[d.off[r]:d.off[r] + d.n[r]] >= 0).sum())
                assert t.endswith(b"\n") and b"\0" not in t and t.count(b"\n") == max(1, n_rec), f"{tag} read {r}"
                S.line_events(t.decode(), ev)
                if int(sel[p]["branch"]) == abi.SEL_PAIRED:
                    ev["hg_lists"] += int(sel[p]["alt"][i]) >= 0
                elif n_rec >= 2:
                    ev["nopair_multi_lines"] += n_rec
            texts += both
        runs[key] = texts
    return runs, ev


def make_cases(refd):
    """the hand-built pairs -> regions per read, in sam_io.CASES order"""
    l_pac = int(refd["l_pac"])
    P, ALT = 50000, int(refd["ann_offset"][2]) + 5000
    fwd = lambda pos=P, **kw: reg(l_pac, pos, **kw)  # noqa: E731
    rev_mate = reg(l_pac, P + 250, rev=True)
    none = np.zeros(0, abi.ALNREG_DTYPE)
    cases = {}
    cases["pa_65_80"] = [cat_regs([fwd(score=65), reg(l_pac, ALT, rid=2, score=80, alt=True)]), rev_mate]
    cases["h_g"] = [cat_regs([fwd(score=140), reg(l_pac, ALT, rid=2, score=150, alt=True)]),
                    cat_regs([reg(l_pac, P + 250, rev=True, score=120), reg(l_pac, ALT + 300, rid=2, score=150, alt=True,
                                                                            rev=True)])]
    cases["supp_mate_clipped"] = [cat_regs([fwd(score=75, qb=0, qe=75), fwd(P + 40000, score=70, qb=75, qe=150)]),
                                  reg(l_pac, P + 260, rev=True, score=130, qb=12, qe=143)]
    cases["unaligned_rev_mate"] = [none, rev_mate]
    cases["unaligned_fwd_mate"] = [fwd(), none]
    cases["both_unaligned"] = [none, none]
    cases["two_strings"] = [cat_regs([fwd(score=75, qb=0, qe=75), fwd(P + 40000, score=70, qb=75, qe=150),
                                      fwd(P + 9000, score=70, qb=0, qe=75), fwd(P + 18000, score=66, qb=0, qe=75),
                                      fwd(P + 60000, score=65, qb=75, qe=150)]), rev_mate]
    assert list(cases) == S.CASES
    return [a.copy() for pair in cases.values() for a in pair]


def run_cases(refd, opt, alt):
    rng = np.random.default_rng(29)
    reads = make_cases(refd)
    seqs = [rng.integers(0, 5 if k % 4 == 3 else 4, 150).astype(np.uint8) for k in range(len(reads))]
    rs = RefSam(opt, PO, refd, alt)
    pes, pid0 = hand_pes(), 40
    marked, fin, sels, oms = [], [], {0: [], 1: []}, {0: [], 1: []}
    for p in range(len(reads) // 2):
        m, npri = zip(*[rs.mark(reads[2 * p + i], 2 * (pid0 + p) + i) for i in range(2)])
        marked += list(m)
        for nopair in (0, 1):
            rec, om, a = rs.select(list(m), list(npri), pes, pid0 + p, bool(nopair), dict.fromkeys(PIO.COVERAGE_KEYS, 0))
            if nopair == 0:
                fin += a
            sels[nopair].append(rec)
            oms[nopair] += om
    n = np.array([len(a) for a in reads], np.int32)
    d = X.XaData("sam_cases", n, {0: cat_regs(fin), 1: cat_regs(marked)},
                 {k: np.array(sels[k], abi.PAIRSEL_DTYPE) for k in (0, 1)},
                 {k: np.concatenate(oms[k]).astype(np.int32) for k in (0, 1)}, None, refd, opt, alt)
    runs, ev = run_batch("cases", rs, d, seqs, reads, pes, pid0, ["pair", "nopair", "other"])
    seq_off, seq = S.blob([x.tobytes() for x in seqs])
    pre = "cases_"
    fixed = {pre + "n": n, pre + "final": d.regs[0], pre + "marked": d.regs[1], pre + "sel": d.sel[0],
             pre + "sel_nopair": d.sel[1], pre + "out_mapq": d.out_mapq[0], pre + "out_mapq_nopair": d.out_mapq[1],
             "seq_off": seq_off, "seq": seq, "alt": alt, "case_names": np.array(S.CASES),
             "opt_int": np.array([opt[k] for k in G.OPT_KEYS], np.int32), "opt_mat": np.asarray(opt["mat"], np.int8),
             "coverage": np.array([ev[k] for k in S.COVERAGE_KEYS], np.int64)}
    for p, name in enumerate(S.CASES):
        print(f"[gen_sam] case {name}:", flush=True)
        for key in runs:
            for i in range(2):
                print(f"    {key} read {i}: {runs[key][2 * p + i].decode()!r}"[:400], flush=True)
    save_fitting(os.path.join(GOLD, "sam_text_cases.npz"), fixed, runs)
    return ev


# ---------------------------------------------------------------- (b) mem_aln2sam on hand-built lists
def aln_cigar(k_case, l_seq, n_ops, clipped):
    """n_ops ops with lengths of one to four digits; a clipped record starts and ends in a clip inside the read"""
    ops = [((1 + (k * 37 + k_case) % (10 ** (1 + k % 4))) << 4) | (0, 1, 2)[k % 3] for k in range(n_ops)]
    if clipped and n_ops >= 2 and l_seq >= 4:
        ops[0] = (l_seq // 4) << 4 | 3
        ops[-1] = (l_seq // 3) << 4 | (4 if k_case % 4 == 1 else 3)
    return np.array(ops, np.uint32)


def run_aln(refd, opt, alt):
    rs = RefSam(opt, PO, refd, alt)
    rng = np.random.default_rng(31)
    MO, MM = S.ALN_MAX_OPS, S.ALN_MAX_MD
    md_pool = (b"0123456789ACGT^" * 8)
    n, regs, out_mapq, recs, cigs, mds, seqs, sel = [], [], [], [], [], [], [], []
    lists = []  # per read: (list of mem_aln_t field dicts, mate dict)

    def record(k_case, j, l_seq, rev, n_ops, pos, md_len, clipped, is_alt):
        return dict(pos=pos, rid=(k_case + j) % 3, is_rev=rev, is_alt=is_alt, mapq=(k_case * 17 + j * 5) % 61,
                    NM=(k_case * 3 + j) % 40, cigar=aln_cigar(k_case + j, l_seq, n_ops, clipped),
                    md=md_pool[j:j + md_len], score=30 + k_case + j, sub=(k_case % 5) * 7, csub=(k_case % 4) * 9,
                    alt_sc=80 if k_case % 3 == 0 else 0)

    def unmapped():
        return dict(pos=-1, rid=-1, is_rev=0, is_alt=0, mapq=0, NM=0, cigar=np.zeros(0, np.uint32), md=b"", score=0,
                    sub=0, csub=0, alt_sc=0, flag=4)

    lens, opsn = [1, 63, 64, 65, 250], [1, 63, 64, 65, 200]
    poss, mdl = [0, 4999999998, 123456], [1, MM - 1, 7]
    for k_case, (l_seq, rev) in enumerate(itertools.product(lens, (0, 1))):
        n_rec = 1 + k_case % 2
        own = [record(k_case, j, l_seq, rev ^ (j & 1), opsn[(k_case + j) % 5], poss[(k_case + j) % 3],
                      mdl[(k_case + j) % 3], j > 0, int(k_case % 5 == 4 and j > 0)) for j in range(n_rec)]
        mate_mapped = k_case % 4 != 3
        mate = record(k_case + 50, 0, 100, 1 - rev, 3, poss[(k_case + 1) % 3] + 200, 5, True, int(k_case % 6 == 5))
        mate["rid"] = own[0]["rid"] if k_case % 2 == 0 else mate["rid"]
        for j, a in enumerate(own):
            a["flag"] = 0x41 | (0x800 if j else 0)
        mate["flag"] = 0x81
        um = unmapped()
        um["flag"] |= 0x81
        seqs += [rng.integers(0, 5 if k_case % 3 == 2 else 4, l_seq).astype(np.uint8),
                 rng.integers(0, 4, 100).astype(np.uint8)]
        lists += [(own, mate if mate_mapped else unmapped()), ([mate] if mate_mapped else [um], own[0])]
        for read in (own, [mate] if mate_mapped else []):
            n.append(len(read))
            for a in read:
                g = np.zeros(1, abi.ALNREG_DTYPE)
                g["score"], g["sub"], g["csub"], g["alt_sc"], g["rid"] = a["score"], a["sub"], a["csub"], a["alt_sc"], a["rid"]
                g["secondary"] = g["secondary_all"] = -1
                g["n_comp_is_alt"] = 1 | (a["is_alt"] << 30)
                regs.append(g)
                out_mapq.append(a["mapq"])
                rec = np.zeros(1, abi.ALN_DTYPE)
                rec["pos"], rec["rid"], rec["is_rev"], rec["n_cigar"] = a["pos"], a["rid"], a["is_rev"], len(a["cigar"])
                rec["NM"], rec["md_len"], rec["score"], rec["status"] = a["NM"], len(a["md"]), 999, abi.ALN_OK
                recs.append(rec)
                slot = np.full(MO, 0xA5A5A5A5, np.uint32)
                slot[:len(a["cigar"])] = a["cigar"]
                cigs.append(slot)
                m = np.full(MM, 0x5A, np.uint8)
                m[:len(a["md"])] = np.frombuffer(a["md"], np.uint8)
                m[len(a["md"])] = 0
                mds.append(m)
        s = np.zeros(1, abi.PAIRSEL_DTYPE)
        s["status"], s["branch"], s["z"] = abi.SEL_DONE, abi.SEL_NO_PAIRING, [[0, 0 if mate_mapped else -1]]
        s["alt"] = -1
        sel.append(s)

    def c_list(items, keep):
        arr = (MemAln * len(items))()
        for x, a in zip(arr, items):
            buf = np.zeros(4 * len(a["cigar"]) + len(a["md"]) + 1, np.uint8)
            buf[:4 * len(a["cigar"])] = a["cigar"].view(np.uint8)
            buf[4 * len(a["cigar"]):-1] = np.frombuffer(a["md"], np.uint8)
            keep.append(buf)
            x.pos, x.rid, x.flag, x.n_cigar = a["pos"], a["rid"], a["flag"] if "flag" in a else 0, len(a["cigar"])
            x.bits = a["is_rev"] | a["is_alt"] << 1 | a["mapq"] << 2 | a["NM"] << 10
            x.cigar, x.XA = buf.ctypes.data, None
            x.score, x.sub, x.alt_sc = a["score"], max(a["sub"], a["csub"]), a["alt_sc"]
        return arr

    def text_of(with_qual):
        texts = []
        for r, (own, mate) in enumerate(lists):
            keep = []
            q = np.ascontiguousarray(seqs[r])
            ql = C.create_string_buffer(S.read_qual(r, len(q)).tobytes())
            s = BSeq()
            com = S.read_comment(r)
            s.l_seq, s.name, s.seq, s.comment = len(q), S.pair_name("aln", r >> 1), q.ctypes.data, com if com else None
            s.qual = C.addressof(ql) if with_qual else None
            arr, m = c_list(own, keep), c_list([mate], keep)
            ks = KString(0, 0, None)
            for which in range(len(own)):
                rs.lib.mem_aln2sam(C.byref(rs.o), C.byref(rs.rp.bns), C.byref(ks), C.byref(s), len(own),
                                   C.cast(arr, C.c_void_p), which, C.cast(m, C.c_void_p))
            texts.append(C.string_at(ks.s, ks.l))
            libc.free(ks.s)
        return texts

    saved = rs.o.flag
    rs.o.flag = 0
    runs = {"q": text_of(True), "nq": text_of(False)}
    rs.o.flag = saved
    seq_off, seq = S.blob([x.tobytes() for x in seqs])
    n = np.array(n, np.int32)
    assert len(n) == len(lists)
    fixed = dict(n=n, regs=cat_regs(regs), sel=np.concatenate(sel), out_mapq=np.array(out_mapq, np.int32),
                 xa_of=np.full(len(regs), -1, np.int32), job_of=np.arange(len(regs), dtype=np.int32),
                 aln=np.concatenate(recs), cigar=np.stack(cigs), md=np.stack(mds), seq_off=seq_off, seq=seq,
                 n_contigs=np.array([rs.rp.bns.n_seqs], np.int32))
    ev = dict.fromkeys(S.COVERAGE_KEYS, 0)
    for t in runs["q"]:
        S.line_events(t.decode(), ev)
    print(f"[gen_sam] aln: {len(lists)} reads, {len(regs)} records, events {ev}", flush=True)
    for r in (0, 1, 2, 3):
        print(f"    read {r}: {runs['q'][r].decode()!r}"[:300], flush=True)
    save_fitting(os.path.join(GOLD, "sam_text_aln.npz"), fixed, runs)


def main():
    refd = G.load_ref()
    opt = abi.default_opt()
    alt2 = np.zeros(len(refd["ann_len"]), np.uint8)
    alt2[2] = 1
    tot = run_cases(refd, opt, alt2)
    print(f"[gen_sam] cases: {tot}", flush=True)
    run_aln(refd, opt, alt2)
    for name in S.SETS:
        s, d = RIO.load(name), X.load(name)
        rs = RefSam(s.opt, dict(PO, max_matesw=int(s.pairopt().max_matesw)), s.genome, s.alt)
        off = RIO.offsets(s.out_n)
        raw = [s.out_regs[o:o + k] for o, k in zip(off, s.out_n)]
        seqs = [s.seq[s.seq_off[r]:s.seq_off[r + 1]] for r in range(s.n_reads)]
        runs, ev = run_batch(name, rs, d, seqs, raw, s.pes, PAIR_ID0[name], S.keys_of(name))
        print(f"[gen_sam] {name}: {d.n_reads // 2} pairs, {ev}", flush=True)
        save_fitting(os.path.join(GOLD, f"sam_text_{name}.npz"),
                     {"coverage": np.array([ev[k] for k in S.COVERAGE_KEYS], np.int64)}, runs)
        for k in tot:
            tot[k] += ev[k]
    print(f"[gen_sam] coverage over the sets and the hand-built pairs: {tot}")
    short = {k: (tot[k], S.FLOORS[k]) for k in S.FLOORS if tot[k] < S.FLOORS[k]}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")


if __name__ == "__main__":
    main()
