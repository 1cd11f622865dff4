#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/xa_select.npz, the expected result of
bwagpu_xa_select_device, made by the reference's own mem_sam_pe
(oracle/_ref/libbwaref.so, loaded through ctypes).

    make -C oracle ref && python tools_dev/gen_xa_fixture.py

Inputs are the pair sets of tests/golden/pair_<set>.npz with the reads of
rescue_<set>.npz (both only read), and a few hand-built pairs.  For every pair,
with and without MEM_F_NOPAIRING, mem_sam_pe runs with MEM_F_NO_RESCUE on the
unmarked regions, as gen_pair_fixture.py's pin runs it, and the XA:Z field of
every line it prints is taken apart.  Stored per region: the number of hits in
the field of the region's record (0 without a field, -1 for a region without a
record).  No line is restated.

The selection restated in numpy (tests/xa_io.py) is pinned on the way: for every
record its hits, in index order, must be the field's hits one by one: contig,
strand and position as the reference's mem_reg2aln gives them for that region.
The script exits non-zero unless the floors of xa_io.FLOORS hold over all sets.
"""
import ctypes as C
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
import xa_io as X  # noqa: E402
from bwagpu import abi  # noqa: E402
from gen_pair_fixture import (F_NO_RESCUE, F_NOPAIRING, PAIR_ID0, BSeq, RefSel, cat_regs, hand_pes, reg)  # noqa: E402
from gen_rescue_fixture import AlnRegV, libc  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MAX_BYTES = 1 << 20
PO = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
          mask_level_redun=0.95, mask_level=0.50)


class RefXa(RefSel):
    def sam_text(self, seqs, a_raw, pes, pid, nopair):
        """the reference's mem_sam_pe without rescue -> s[0].sam, s[1].sam"""
        o = self.o
        saved = o.flag
        o.flag = F_NO_RESCUE | (F_NOPAIRING if nopair else 0)
        s = (BSeq * 2)()
        keep = [np.ascontiguousarray(x, np.uint8) for x in seqs]
        v = (AlnRegV * 2)()
        for i in range(2):
            s[i].l_seq, s[i].name, s[i].seq = len(keep[i]), b"r", keep[i].ctypes.data
            t = self.to_v(np.ascontiguousarray(a_raw[i]))
            v[i].n, v[i].m, v[i].a = t.n, t.m, t.a
        self.lib.mem_sam_pe(C.byref(o), C.byref(self.rp.bns), self.rp.pac.ctypes.data, pes.ctypes.data, int(pid),
                            C.cast(s, C.c_void_p), C.cast(v, C.c_void_p))
        o.flag = saved
        out = []
        for i in range(2):
            out.append(C.string_at(s[i].sam).decode())
            libc.free(s[i].sam)
            libc.free(v[i].a)
        return out

    def xopt(self):
        return abi.SamOpt(0, float(self.o.XA_drop_ratio), int(self.o.max_XA_hits), int(self.o.max_XA_hits_alt))


def xa_hits(line):
    """the hits of a SAM line's XA:Z field as (contig, strand, pos) -> list"""
    for f in line.split("\t")[11:]:
        if f.startswith("XA:Z:"):
            hits = [h.split(",") for h in f[5:].split(";") if h]
            return [(h[0], h[1][0], int(h[1][1:])) for h in hits]
    return []


def xa_counts(tag, rs: RefXa, pes, seqs, raw_by_read, d, mode, pair_id0, tot):
    """mem_sam_pe over every pair of one batch in one mode -> xa_cnt parallel to the regions"""
    regs, sel, om = d.regs[mode], d.sel[mode], d.out_mapq[mode]
    xa_of, _, ev = X.xa_model(d.off, regs, d.n, sel, om, rs.xopt())
    cnt = np.full(len(regs), -1, np.int32)
    for p in range(d.n_reads // 2):
        assert int(sel[p]["status"]) == abi.SEL_DONE, f"{tag} pair {p}"
        texts = rs.sam_text(seqs[2 * p:2 * p + 2], raw_by_read[2 * p:2 * p + 2], pes, pair_id0 + p, bool(mode))
        for i in range(2):
            r = 2 * p + i
            lo, n = int(d.off[r]), int(d.n[r])
            a, x = regs[lo:lo + n], xa_of[lo:lo + n]
            lines = texts[i].strip("\n").split("\n")
            emitted = np.nonzero(om[lo:lo + n] >= 0)[0]
            assert len(lines) == max(1, len(emitted)), f"{tag} read {r}: {len(lines)} lines, {len(emitted)} records"
            if len(emitted) == 0:
                assert xa_hits(lines[0]) == [], f"{tag} read {r}"
            for line, k in zip(lines, emitted):
                got = xa_hits(line)
                want = []
                for j in np.nonzero(x == k)[0]:
                    rid, pos, rev, _ = rs.reg2aln(seqs[r], a[j])
                    want.append((f"c{rid}", "+-"[rev], pos + 1))
                assert got == want, f"{tag} read {r} region {k}: XA {got} != restated {want}"
                cnt[lo + k] = len(got)
    for k in X.COVERAGE_KEYS:
        tot[k] += int(ev[k])
    return cnt


def make_cases(refd):
    """the hand-built pairs -> (regions per read, names); the mate is one plain hit in range"""
    l_pac = int(refd["l_pac"])
    P, ALT = 50000, int(refd["ann_offset"][2]) + 5000
    fwd = lambda pos=P, **kw: reg(l_pac, pos, **kw)  # noqa: E731
    mate = reg(l_pac, P + 250, rev=True)
    sec = lambda k, score, **kw: fwd(P + 9000 * (k + 1), score=score, **kw)  # noqa: E731  (overlaps the whole read)
    cases = {}
    cases["at_cap"] = cat_regs([fwd()] + [sec(k, 130 + k) for k in range(5)])
    cases["over_cap"] = cat_regs([fwd()] + [sec(k, 130 + k) for k in range(6)])
    cases["alt_lifts_cap"] = cat_regs([fwd()] + [sec(k, 130 + k) for k in range(5)] +
                                      [reg(l_pac, ALT, rid=2, score=128, alt=True)])
    cases["ratio_80_81"] = cat_regs([fwd(score=100), sec(0, 80), sec(1, 81)])
    cases["primary_below_T"] = cat_regs([fwd(score=29), sec(0, 28), sec(1, 27)])
    cases["two_strings"] = cat_regs([fwd(score=75, qb=0, qe=75), fwd(P + 40000, score=70, qb=75, qe=150),
                                     fwd(P + 9000, score=70, qb=0, qe=75), fwd(P + 18000, score=66, qb=0, qe=75),
                                     fwd(P + 60000, score=65, qb=75, qe=150)])
    assert list(cases) == X.CASES
    reads = []
    for a in cases.values():
        reads += [a, mate.copy()]
    return reads


def run_cases(refd, opt, alt, tot):
    rng = np.random.default_rng(23)
    reads = make_cases(refd)
    seqs = [rng.integers(0, 4, 150).astype(np.uint8) for _ in reads]
    rs = RefXa(opt, PO, refd, alt)
    pes, pid0 = hand_pes(), 40
    marked, n_pri, fin, sels, oms = [], [], [], {0: [], 1: []}, {0: [], 1: []}
    for p in range(len(reads) // 2):
        m, npri = zip(*[rs.mark(reads[2 * p + i], 2 * (pid0 + p) + i) for i in range(2)])
        marked += list(m)
        n_pri += list(npri)
        for nopair in (0, 1):
            rec, om, a = rs.select(list(m), list(npri), pes, pid0 + p, bool(nopair), dict.fromkeys(PIO.COVERAGE_KEYS, 0))
            if nopair == 0:
                fin += a
            sels[nopair].append(rec)
            oms[nopair] += om
    n = np.array([len(a) for a in reads], np.int32)
    d = X.XaData("cases", n, {0: cat_regs(fin), 1: cat_regs(marked)},
                 {k: np.array(sels[k], abi.PAIRSEL_DTYPE) for k in (0, 1)},
                 {k: np.concatenate(oms[k]).astype(np.int32) for k in (0, 1)}, None, refd, opt, alt)
    cnt = {mode: xa_counts("cases", rs, pes, seqs, reads, d, mode, pid0, tot) for mode in (0, 1)}
    pre = "cases_"
    out = {pre + "n": n, pre + "final": d.regs[0], pre + "marked": d.regs[1], pre + "sel": d.sel[0],
           pre + "sel_nopair": d.sel[1], pre + "out_mapq": d.out_mapq[0], pre + "out_mapq_nopair": d.out_mapq[1],
           pre + "xa_cnt": cnt[0], pre + "xa_cnt_nopair": cnt[1], "case_names": np.array(X.CASES)}
    for p, name in enumerate(X.CASES):
        lo, k = int(d.off[2 * p]), int(n[2 * p])
        print(f"[gen_xa] case {name}: branch {int(d.sel[0][p]['branch'])}, xa_cnt {cnt[0][lo:lo + k].tolist()} / "
              f"nopair {cnt[1][lo:lo + k].tolist()}", flush=True)
    return out


def main():
    tot = dict.fromkeys(X.COVERAGE_KEYS, 0)
    refd = G.load_ref()
    opt = abi.default_opt()
    alt2 = np.zeros(len(refd["ann_len"]), np.uint8)
    alt2[2] = 1
    arrays = run_cases(refd, opt, alt2, tot)
    arrays.update(alt=alt2, opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32),
                  opt_mat=np.asarray(opt["mat"], np.int8))
    for name in X.SETS:
        s, pd = RIO.load(name), PIO.load(name)
        rs = RefXa(s.opt, dict(PO, max_matesw=int(s.pairopt().max_matesw)), s.genome, s.alt)
        off = RIO.offsets(s.out_n)
        raw = [s.out_regs[o:o + k] for o, k in zip(off, s.out_n)]
        seqs = [s.seq[s.seq_off[r]:s.seq_off[r + 1]] for r in range(s.n_reads)]
        d = X.XaData(name, pd.n, {0: pd.final, 1: pd.marked}, pd.sel, pd.out_mapq, None, s.genome, s.opt, s.alt)
        before = dict(tot)
        for mode, key in ((0, "_xa_cnt"), (1, "_xa_cnt_nopair")):
            arrays[name + key] = xa_counts(name, rs, s.pes, seqs, raw, d, mode, PAIR_ID0[name], tot)
        print(f"[gen_xa] {name}: {d.n_reads // 2} pairs, {len(pd.final)} regions, "
              f"{ {k: tot[k] - before[k] for k in tot} }", flush=True)
    xo = abi.default_samopt()
    path = os.path.join(GOLD, "xa_select.npz")
    np.savez_compressed(path, **arrays, coverage=np.array([tot[k] for k in X.COVERAGE_KEYS], np.int64),
                        xaopt_f=np.array([xo.XA_drop_ratio], np.float32),
                        xaopt_int=np.array([xo.max_XA_hits, xo.max_XA_hits_alt], np.int32))
    size = os.path.getsize(path)
    print(f"[gen_xa] xa_select.npz: {size} bytes; coverage over all sets: {tot}")
    if size > MAX_BYTES:
        raise SystemExit(f"xa_select.npz is {size} bytes (> {MAX_BYTES})")
    short = {k: (tot[k], X.FLOORS[k]) for k in X.FLOORS if tot[k] < X.FLOORS[k]}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")


if __name__ == "__main__":
    main()
