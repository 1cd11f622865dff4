#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/pair_<set>.npz and pair_cases.npz, the
expected results of bwagpu_mark_primary and bwagpu_pair_select, made by the
reference's own mem_mark_primary_se, mem_pair and mem_approx_mapq_se
(oracle/_ref/libbwaref.so, loaded through ctypes).

    make -C oracle ref && python tools_dev/gen_pair_fixture.py

Inputs of the six sets named after the rescue sets are the post-rescue regions
and pes stored in tests/golden/rescue_<set>.npz (out_regs, out_n, pes: what
gen_rescue_fixture.run_pairs wrote; those files are only read).  The glue of
mem_sam_pe between the three functions (bwamem_pair.c:288-336, :374-390, and
mem_reg2sam's selection, bwamem.c:1030-1047) is restated in RefSel.select.

The restatement is pinned: for every pair the reference's own mem_sam_pe runs
with MEM_F_NO_RESCUE on the same unmarked regions, and (a) the regions it
leaves must equal the restated ones byte for byte, (b) every SAM record's
FLAG, RNAME, POS and MAPQ must equal what the restated selection gives
through the reference's mem_reg2aln and mem_aln2sam's flag rules.

`split` is a library simulated at the level of regions (mem_pair, the marking
and the mapq read nothing else): chimeric reads whose halves lie far apart,
reads from one copy of a diverged duplication whose mate lies beside the other
copy, and pairs on different contigs or far out of range, mixed with ordinary
FR pairs.  Every set is stored with and without MEM_F_NOPAIRING.  The script
exits non-zero unless the floors below are met over all sets together.
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
import rescue_io as RIO  # noqa: E402
from bwagpu import abi  # noqa: E402
from gen_post_fixture import BntSeq, MemOpt  # noqa: E402
from gen_rescue_fixture import AlnRegV, RefPair, infer_dir, libc  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MAX_BYTES = 1 << 20
REG = abi.ALNREG_DTYPE.itemsize
F_NOPAIRING, F_NO_RESCUE = 0x4, 0x20
COVERAGE_KEYS = ("proper", "no_primary", "is_multi", "unpaired_preferred", "pair0_with_primaries", "z_nonzero",
                 "switched", "n_sub_pos", "csub_over_sub", "hash_ties", "alt_emitted", "reads_mixed_alt",
                 "reads_over_17", "two_live")
FLOORS = dict(is_multi=20, unpaired_preferred=20, pair0_with_primaries=20, z_nonzero=100, switched=100, hash_ties=10,
              alt_emitted=10, reads_mixed_alt=50, two_live=1)
SELOPT = dict(T=30, pen_unpaired=17, min_seed_len=19, mapQ_coef_len=50.0, mapQ_coef_fac=3, mask_level=0.5,
              drop_ratio=0.5)
SELOPT_KEYS_I = ("T", "pen_unpaired", "min_seed_len", "mapQ_coef_fac")
SELOPT_KEYS_F = ("mapQ_coef_len", "mask_level", "drop_ratio")
PAIR_ID0 = dict(fr=(1 << 23) - 700, mixed=(1 << 23) - 300, shift=0, ends=123456, rep=1000, rep_sw2=77, split=5000)


class BSeq(C.Structure):  # bseq1_t, bwa/bwa.h:40-46 (USE_STD_BWA)
    _fields_ = [("l_seq", C.c_int), ("id", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p),
                ("seq", C.c_void_p), ("qual", C.c_void_p), ("sam", C.c_void_p)]


class MemAln(C.Structure):  # mem_aln_t, bwa/bwamem.h:88-98
    _fields_ = [("pos", C.c_int64), ("rid", C.c_int), ("flag", C.c_int), ("bits", C.c_uint32), ("n_cigar", C.c_int),
                ("cigar", C.c_void_p), ("XA", C.c_void_p), ("score", C.c_int), ("sub", C.c_int), ("alt_sc", C.c_int)]


def is_alt(a):
    return (a["n_comp_is_alt"] >> np.uint32(30)) != 0


class RefSel(RefPair):
    """the reference's marking, mem_pair and mapq; the restated glue; the pin against mem_sam_pe"""

    def __init__(self, opt, pairopt, refd, alt, selopt=SELOPT):
        super().__init__(opt, pairopt, refd, alt)
        o, lib = self.o, self.lib
        for k in SELOPT_KEYS_I + SELOPT_KEYS_F:
            setattr(o, k, selopt[k])
        self.T, self.pen_unpaired = int(o.T), int(o.pen_unpaired)
        vp, ip = C.c_void_p, C.POINTER(C.c_int)
        lib.mem_pair.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, vp, vp, vp, C.c_int, ip, ip, ip, ip]
        lib.mem_pair.restype = C.c_int
        lib.mem_approx_mapq_se.argtypes = [C.POINTER(MemOpt), vp]
        lib.mem_approx_mapq_se.restype = C.c_int
        lib.mem_sam_pe.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, vp, C.c_uint64, vp, vp]
        lib.mem_sam_pe.restype = C.c_int
        lib.mem_reg2aln.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, C.c_int, vp, vp]
        lib.mem_reg2aln.restype = MemAln

    def mark(self, a, rid):
        a = np.array(a, abi.ALNREG_DTYPE, order="C")
        n_pri = self.lib.mem_mark_primary_se(C.byref(self.o), len(a), a.ctypes.data, int(rid)) if len(a) else 0
        return a, n_pri

    def mapq(self, rec):
        r = np.array(rec, abi.ALNREG_DTYPE, order="C").reshape(1)
        return int(self.lib.mem_approx_mapq_se(C.byref(self.o), r.ctypes.data))

    def pair(self, a, npri, pes, pid):
        v = (AlnRegV * 2)()
        keep = [np.ascontiguousarray(x) for x in a]
        for i in range(2):
            v[i].n = v[i].m = len(keep[i])
            v[i].a = keep[i].ctypes.data if len(keep[i]) else None
        sub, n_sub = C.c_int(0), C.c_int(0)
        z, np_ = (C.c_int * 2)(0, 0), (C.c_int * 2)(int(npri[0]), int(npri[1]))
        id32 = ((int(pid) & 0xffffffff) ^ 0x80000000) - 0x80000000  # mem_sam_pe hands its uint64 id to an int
        o = self.lib.mem_pair(C.byref(self.o), C.byref(self.rp.bns), self.rp.pac.ctypes.data, pes.ctypes.data, None,
                              C.cast(v, C.c_void_p), id32, C.byref(sub), C.byref(n_sub), z, np_)
        return o, sub.value, n_sub.value, [z[0], z[1]]

    def raw_mapq(self, diff):
        return int(6.02 * diff / self.o.a + .499)

    def select(self, a_in, npri, pes, pid, nopair, ev):
        """bwamem_pair.c:286-392 up to the first mem_reg2aln on marked regions ->
        (PAIRSEL_DTYPE record, [out_mapq per read], [regions per read as the reference leaves them])"""
        a = [x.copy() for x in a_in]
        n = [len(x) for x in a]
        T = self.T
        rec = np.zeros((), abi.PAIRSEL_DTYPE)
        rec["n_pri"] = npri
        rec["z"] = rec["alt"] = -1
        extra = 1
        om = [np.full(n[i], -1, np.int32) for i in range(2)]
        called = (not nopair) and npri[0] > 0 and npri[1] > 0
        o = subo = n_sub = 0
        z = [0, 0]
        if called:
            o, subo, n_sub, z = self.pair(a, npri, pes, pid)
            rec["o"], rec["subo"], rec["n_sub"] = o, subo, n_sub
            ev["pair0_with_primaries"] += o == 0
            ev["hash_ties"] += o > 0 and subo == o
        ev["no_primary"] += (not nopair) and not called
        paired = called and o > 0
        if paired:
            multi = [any(a[i]["secondary"][j] < 0 and a[i]["score"][j] >= T for j in range(1, npri[i])) for i in range(2)]
            if multi[0] or multi[1]:
                paired = False
                ev["is_multi"] += 1
        if paired:
            ev["proper"] += 1
            ev["n_sub_pos"] += n_sub > 0
            score_un = int(a[0]["score"][0]) + int(a[1]["score"][0]) - self.pen_unpaired
            subo = max(subo, score_un)
            q_pe = self.raw_mapq(o - subo)
            if n_sub > 0:
                q_pe -= int(4.343 * np.log(n_sub + 1) + .499)
            q_pe = min(max(q_pe, 0), 60)
            fr = np.float32(a[0]["frac_rep"][0]) + np.float32(a[1]["frac_rep"][0])  # float + float
            q_pe = int(q_pe * (1. - .5 * float(fr)) + .499)
            q_se = [0, 0]
            if o > score_un:
                for i in range(2):
                    c = a[i][z[i]:z[i] + 1]
                    if c["secondary"][0] >= 0:
                        c["sub"] = a[i]["score"][c["secondary"][0]]
                        c["secondary"] = -2
                    q = self.mapq(c[0])
                    q = q if q > q_pe else (q_pe if q_pe < q + 40 else q + 40)
                    # h[i].mapq is an 8-bit field: a negative tandem-repeat cap (csub > score) wraps
                    q_se[i] = min(q, self.raw_mapq(int(c["score"][0]) - int(c["csub"][0]))) & 0xff
                    ev["csub_over_sub"] += c["csub"][0] > c["sub"][0]
                extra |= 2
            else:
                ev["unpaired_preferred"] += 1
                z = [0, 0]
                q_se = [self.mapq(a[i][0]) for i in range(2)]
            for i in range(2):
                ev["z_nonzero"] += z[i] != 0
                k = int(a[i]["secondary_all"][z[i]])
                if 0 <= k < npri[i]:
                    assert a[i]["secondary_all"][k] < 0
                    sa = a[i]["secondary_all"]
                    sa[(sa == k) | (np.arange(n[i]) == k)] = z[i]
                    sa[z[i]] = -1
                    ev["switched"] += 1
            rec["branch"] = abi.SEL_PAIRED
            for i in range(2):
                rec["z"][i], rec["mapq"][i] = z[i], q_se[i]
                om[i][z[i]] = q_se[i]
                if npri[i] < n[i]:
                    p = a[i][npri[i]]
                    if not (p["score"] < T or p["secondary"] >= 0 or not is_alt(p)):
                        rec["alt"][i] = npri[i]
                        om[i][npri[i]] = self.mapq(p)
                        ev["alt_emitted"] += 1
        else:
            rid = [-1, -1]
            for i in range(2):
                which = -1
                if n[i]:
                    if a[i]["score"][0] >= T:
                        which = 0
                    elif npri[i] < n[i] and a[i]["score"][npri[i]] >= T:
                        which = npri[i]
                rec["z"][i] = which
                if which >= 0:
                    h = a[i][which]
                    rid[i] = int(h["rid"]) if h["rb"] >= 0 and h["re"] >= 0 else -1
                    rec["mapq"][i] = self.mapq(h) if h["secondary"] < 0 else 0
                cnt = first = 0
                for j in range(n[i]):  # mem_reg2sam, bwamem.c:1030-1047 without MEM_F_ALL
                    p = a[i][j]
                    if p["score"] < T or p["secondary"] >= 0:
                        continue
                    q = self.mapq(p)
                    if cnt and not is_alt(p) and q > first:
                        q = first
                    if not cnt:
                        first = q
                    om[i][j] = q
                    cnt += 1
                    ev["alt_emitted"] += bool(is_alt(p))
            if not nopair and rid[0] == rid[1] and rid[0] >= 0:
                d, dist = infer_dir(self.l_pac, int(a[0]["rb"][0]), int(a[1]["rb"][0]))
                if not pes["failed"][d] and pes["low"][d] <= dist <= pes["high"][d]:
                    extra |= 2
        rec["extra_flag"] = extra
        return rec, om, a

    # ---- the pin
    def reg2aln(self, seq, reg):
        """the reference's mem_reg2aln -> (rid, pos, is_rev, flag)"""
        q = np.ascontiguousarray(seq, np.uint8)
        if reg is None:
            return -1, -1, 0, 4
        r = np.array(reg, abi.ALNREG_DTYPE, order="C").reshape(1)
        m = self.lib.mem_reg2aln(C.byref(self.o), C.byref(self.rp.bns), self.rp.pac.ctypes.data, len(q), q.ctypes.data,
                                 r.ctypes.data)
        if m.cigar:
            libc.free(m.cigar)
        return int(m.rid), int(m.pos), int(m.bits & 1), int(m.flag)

    def expect_sam(self, seqs, a, rec, om):
        """(FLAG, RNAME, POS, MAPQ) of every record the selection stands for, per read
        (bwamem_pair.c:342-362 / mem_reg2sam, and mem_aln2sam's flags, bwamem.c:844-864)"""
        extra = int(rec["extra_flag"])
        h = [self.reg2aln(seqs[i], a[i][rec["z"][i]] if rec["z"][i] >= 0 else None) for i in range(2)]
        out = []
        for i in range(2):
            lst = []
            if rec["branch"] == abi.SEL_PAIRED:
                lst.append((h[i], int(rec["mapq"][i]), 0x40 << i | extra))
                if rec["alt"][i] >= 0:
                    k = int(rec["alt"][i])
                    lst.append((self.reg2aln(seqs[i], a[i][k]), int(om[i][k]), 0x800 | 0x40 << i | extra))
            else:
                for k in np.nonzero(om[i] >= 0)[0]:
                    lst.append((self.reg2aln(seqs[i], a[i][k]), int(om[i][k]),
                                (0x40 << i) | 1 | extra | (0x800 if lst else 0)))
                if not lst:
                    lst.append(((-1, -1, 0, 4), 0, (0x40 << i) | 1 | extra))
            m = h[1 - i]
            recs = []
            for (rid, pos, rev, fl), mapq, add in lst:
                fl |= add | 1 | (4 if rid < 0 else 0) | (8 if m[0] < 0 else 0)
                m_rev = m[2]
                if rid < 0 and m[0] >= 0:
                    rid, pos, rev = m[0], m[1], m[2]
                if m[0] < 0 and rid >= 0:
                    m_rev = rev
                fl |= (0x10 if rev else 0) | (0x20 if m_rev else 0)
                recs.append((fl & 0xffff, f"c{rid}" if rid >= 0 else "*", pos + 1 if rid >= 0 else 0,
                             mapq if rid >= 0 else 0))
            out.append(recs)
        return out

    def sam_pe(self, seqs, a_raw, pes, pid, nopair):
        """the reference's mem_sam_pe without rescue -> ([records per read], [regions per read] as it leaves them)"""
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
        recs, regs = [], []
        for i in range(2):
            text = C.string_at(s[i].sam).decode()
            libc.free(s[i].sam)
            lines = [x.split("\t") for x in text.strip().split("\n")]
            recs.append([(int(f[1]), f[2], int(f[3]), int(f[4])) for f in lines])
            regs.append(self.from_v(v[i]))
            libc.free(v[i].a)
        return recs, regs


def select_pairs(name, rs: RefSel, pes, seqs, regs_by_read, pair_id0):
    """both passes of the reference over every pair -> (the fixture's result arrays, coverage counts)"""
    nr = len(regs_by_read)
    assert nr % 2 == 0
    cov = dict.fromkeys(COVERAGE_KEYS, 0)
    cov["two_live"] = int((pes["failed"] == 0).sum() >= 2)
    marked, n_pri, fin, sel, mapq = [], [], [], {0: [], 1: []}, {0: [], 1: []}
    for p in range(nr // 2):
        pid = pair_id0 + p
        raw = [regs_by_read[2 * p], regs_by_read[2 * p + 1]]
        m, npri = [], []
        for i in range(2):
            x, k = rs.mark(raw[i], 2 * pid + i)
            m.append(x)
            npri.append(k)
            cov["reads_mixed_alt"] += 0 < k < len(x)
            cov["reads_over_17"] += len(x) > 17
        marked += m
        n_pri += npri
        sq = [seqs[2 * p], seqs[2 * p + 1]]
        for nopair in (0, 1):
            ev = dict.fromkeys(COVERAGE_KEYS, 0)
            rec, om, a = rs.select(m, npri, pes, pid, bool(nopair), ev)
            # the pin: the reference's own mem_sam_pe on the unmarked regions
            got, left = rs.sam_pe(sq, raw, pes, pid, bool(nopair))
            for i in range(2):
                bad = G.region_mismatch(a[i], left[i])
                assert bad is None, f"{name} pair {p} nopair={nopair}: regions differ from mem_sam_pe's: {bad}"
            want = rs.expect_sam(sq, a, rec, om)
            assert got == want, f"{name} pair {p} nopair={nopair}: SAM records {got} != restated {want}"
            if nopair == 0:
                fin += a
                for k in COVERAGE_KEYS:
                    if k not in ("reads_mixed_alt", "reads_over_17", "two_live"):
                        cov[k] += int(ev[k])
            else:
                assert all(G.region_mismatch(a[i], m[i]) is None for i in range(2))
            sel[nopair].append(rec)
            mapq[nopair] += om
    cat = lambda v, dt: np.concatenate(v) if len(v) else np.zeros(0, dt)  # noqa: E731
    res = dict(n=np.array([len(a) for a in regs_by_read], np.int32), n_pri=np.array(n_pri, np.int32),
               marked=cat(marked, abi.ALNREG_DTYPE), final=cat(fin, abi.ALNREG_DTYPE),
               sel=np.array(sel[0], abi.PAIRSEL_DTYPE), sel_nopair=np.array(sel[1], abi.PAIRSEL_DTYPE),
               out_mapq=cat(mapq[0], np.int32), out_mapq_nopair=cat(mapq[1], np.int32))
    return res, cov


def run_set(name, rs: RefSel, pes, seqs, regs_by_read, pair_id0, out_dir, extra=None):
    """the reference over every pair, written to pair_<name>.npz -> coverage counts"""
    nr = len(regs_by_read)
    res, cov = select_pairs(name, rs, pes, seqs, regs_by_read, pair_id0)
    o = rs.o
    path = os.path.join(out_dir, f"pair_{name}.npz")
    np.savez_compressed(
        path, **(extra or {}), pair_id0=np.array([pair_id0], np.int64),
        selopt_int=np.array([getattr(o, k) for k in SELOPT_KEYS_I], np.int32),
        selopt_f=np.array([getattr(o, k) for k in SELOPT_KEYS_F], np.float32), **res,
        coverage=np.array([int(cov[k]) for k in COVERAGE_KEYS], np.int64))
    size = os.path.getsize(path)
    print(f"[gen_pair] pair_{name}: {nr // 2} pairs, {sum(len(a) for a in regs_by_read)} regions, {size} bytes, "
          f"{ {k: int(v) for k, v in cov.items()} }", flush=True)
    if size > MAX_BYTES:
        raise SystemExit(f"pair_{name}.npz is {size} bytes (> {MAX_BYTES})")
    return cov


# ---------------------------------------------------------------- synthetic regions (split, cases)
def reg(l_pac, pos, rev=False, rid=0, score=150, qb=0, qe=150, alt=False, csub=0, seedcov=None, frac_rep=0.0):
    """one region of qe - qb bases whose forward-strand leftmost base is pos"""
    a = np.zeros(1, abi.ALNREG_DTYPE)
    ln = qe - qb
    a["rb"] = (l_pac << 1) - (pos + ln) if rev else pos
    a["re"] = a["rb"] + ln
    a["qb"], a["qe"], a["rid"], a["score"], a["truesc"], a["secondary"] = qb, qe, rid, score, score, -1
    a["csub"], a["w"], a["seedcov"], a["seedlen0"] = csub, 100, ln // 2 if seedcov is None else seedcov, 19
    a["frac_rep"] = frac_rep
    a["n_comp_is_alt"] = 1 | (1 << 30 if alt else 0)
    return a


def hand_pes(low=100, high=700, avg=400.0, std=50.0, live=(1,)):
    pes = np.zeros(4, abi.PESTAT_DTYPE)
    pes["failed"] = 1
    for d in live:
        pes[d] = (low, high, 0, 0, avg, std)
    return pes


def cat_regs(parts):
    return np.concatenate(parts) if parts else np.zeros(0, abi.ALNREG_DTYPE)


def split_library(rng, refd, n_pairs):
    """-> regions per read of the `split` library (contig 2 is ALT)"""
    l_pac = int(refd["l_pac"])
    ao, al = [int(x) for x in refd["ann_offset"]], [int(x) for x in refd["ann_len"]]

    def where(c, span=2000):
        return ao[c] + int(rng.integers(1000, al[c] - span - 1000))

    reads = []
    for k in range(n_pairs):
        kind = k % 8
        c = int(rng.integers(0, 2))
        p = where(c)
        isz = int(np.clip(rng.normal(400, 50), 200, 650))
        s1, s2 = int(rng.integers(120, 151)), int(rng.integers(120, 151))
        r1 = [reg(l_pac, p, rid=c, score=s1)]
        r2 = [reg(l_pac, p + isz - 150, rev=True, rid=c, score=s2)]
        if kind == 0:  # chimeric read: its halves lie far apart, the mate beside one of them
            far = where(c)
            r1 = [reg(l_pac, p, rid=c, score=75, qb=0, qe=75), reg(l_pac, far, rid=c, score=int(rng.integers(60, 76)), qb=75, qe=150)]
        elif kind == 1:  # diverged duplication: the read's best hit is copy A, the mate lies beside copy B
            copy_b = p
            copy_a = where(c)
            r1 = [reg(l_pac, copy_a, rid=c, score=s1), reg(l_pac, copy_b, rid=c, score=s1 - int(rng.integers(20, 45)))]
        elif kind == 2:  # different contigs, or far out of range
            if k % 16 == 2:
                r2 = [reg(l_pac, where(1 - c), rev=True, rid=1 - c, score=s2)]
            else:
                r2 = [reg(l_pac, p + 5000 + int(rng.integers(0, 5000)), rev=True, rid=c, score=s2)]
        elif kind == 3:  # a duplication close by: two candidate pairs, often of equal q
            d = int(rng.choice([2, 2, 5, 40]))  # 2: the two insert sizes lie symmetric about the mean
            r2 = [reg(l_pac, p + isz - 150, rev=True, rid=c, score=s2), reg(l_pac, p + 2 * 400 - isz - 150 + d, rev=True, rid=c, score=s2)]
        elif kind == 4:  # an ALT hit beside the primary ones (contig 2)
            r1 = r1 + [reg(l_pac, where(2), rid=2, score=s1 + int(rng.integers(-10, 11)), alt=True)]
        elif kind == 5:  # the mate's better hit is elsewhere: the pair picks the second one (z != 0, switch)
            r2 = [reg(l_pac, where(c), rev=True, rid=c, score=s2 + 3)] + r2
        elif kind == 6:  # a short, low hit only; a read without hits now and then
            r2 = [] if k % 16 == 6 else [reg(l_pac, p + isz - 40, rev=True, rid=c, score=int(rng.integers(20, 40)), qb=0, qe=40)]
        for r in (r1, r2):
            for x in r:
                x["csub"] = int(rng.choice([0, 0, 0, int(x["score"][0]) - 5, int(x["score"][0]) // 2]))
                x["frac_rep"] = float(rng.choice([0.0, 0.0, 0.25]))
                x["sub_n"] = 0
        if rng.random() < 0.5:
            r1, r2 = r2, r1
        reads += [cat_regs(r1), cat_regs(r2)]
    return reads


def rand_read(rng, l_pac, refd, n, n_alt=0, base=150):
    """a read of n regions with random extents on the read, n_alt of them on the ALT contig 2"""
    ao, al = [int(x) for x in refd["ann_offset"]], [int(x) for x in refd["ann_len"]]
    out = []
    for k in range(n):
        qb = int(rng.integers(0, 100))
        qe = int(rng.integers(qb + 25, 151))
        alt = k < n_alt
        c = 2 if alt else int(rng.integers(0, 2))
        pos = ao[c] + int(rng.integers(1000, al[c] - 2000))
        out.append(reg(l_pac, pos, rev=bool(rng.integers(0, 2)), rid=c, score=int(rng.integers(base - 60, base + 1)) * (qe - qb) // 150,
                       qb=qb, qe=qe, alt=alt, csub=int(rng.integers(0, 30))))
    rng.shuffle(out)
    return cat_regs(out)


def make_cases(refd, opt, po, alt, out_dir):
    """pair_cases.npz: hand-built pairs, every case a small batch with its own pes"""
    l_pac = int(refd["l_pac"])
    rng = np.random.default_rng(11)
    P = 50000
    fwd = lambda pos=P, **kw: reg(l_pac, pos, **kw)  # noqa: E731
    rev = lambda pos=P + 250, **kw: reg(l_pac, pos, rev=True, **kw)  # noqa: E731
    none = np.zeros(0, abi.ALNREG_DTYPE)
    cap = abi.SEL_MAX_REGS
    cases = {}
    pes = hand_pes()
    cases["n0_n0"] = (pes, [none, none])
    cases["n0_n1"] = (pes, [none, rev(), fwd(), none])
    cases["n1_n1"] = (pes, [fwd(), rev(), rev(), fwd()])
    cases["n2_n1"] = (pes, [cat_regs([fwd(), fwd(P + 9000, score=140)]), rev(), rev(), cat_regs([fwd(score=120), fwd(P + 9000)])])
    cases["n2_n2"] = (pes, [cat_regs([fwd(), fwd(P + 9000, score=149)]), cat_regs([rev(P + 9250), rev(score=149)])])
    cases["only_alt"] = (pes, [fwd(ao := int(refd["ann_offset"][2]) + 5000, rid=2, alt=True), rev(ao + 250, rid=2, alt=True),
                               cat_regs([fwd(ao, rid=2, alt=True), fwd(ao + 700, rid=2, alt=True, score=140)]), rev()])
    for k in (16, 17, 64, 65):
        cases[f"n{k}"] = (pes, [rand_read(rng, l_pac, refd, k, n_alt=k // 5), rand_read(rng, l_pac, refd, 3),
                                rand_read(rng, l_pac, refd, 2), rand_read(rng, l_pac, refd, k)])
    cases["n_cap"] = (pes, [rand_read(rng, l_pac, refd, cap, n_alt=40), rand_read(rng, l_pac, refd, 2, n_alt=2)])
    cases["n_cap_plus_1"] = (pes, [rand_read(rng, l_pac, refd, cap + 1, n_alt=3), fwd(), fwd(), rev()])
    cases["pri_cap_plus_1"] = (pes, [rand_read(rng, l_pac, refd, cap - 1), rand_read(rng, l_pac, refd, 2), fwd(), rev()])
    cases["all_failed"] = (hand_pes(live=()), [fwd(), rev(), cat_regs([fwd(), fwd(P + 9000, score=100)]), rev()])
    at = lambda d: rev(P + d - 149)  # noqa: E731  (mem_pair's dist to fwd() is d)
    cases["dist_at_low_high"] = (pes, [fwd(), at(100), fwd(), at(700), fwd(), at(99), fwd(), at(701)])
    cases["score_0"] = (pes, [fwd(score=0), rev(), fwd(score=0), rev(score=0)])
    cases["sub_ge_score"] = (pes, [fwd(csub=150), rev(), fwd(csub=200), rev(csub=149),
                                   cat_regs([fwd(score=100, csub=10), fwd(P + 3, score=100, csub=10)]), rev()])
    cases["two_live_rf"] = (hand_pes(live=(1, 2)), [rev(P), fwd(P + 250), fwd(), rev(), rev(P), fwd(P + 250)])
    arrays = dict(names=np.array(list(cases)))
    rs = RefSel(opt, po, refd, alt)
    pid0 = 40
    for name, (pes, reads) in cases.items():
        seqs = [rng.integers(0, 4, 150).astype(np.uint8) for _ in reads]
        big = max(len(a) for a in reads) > 200  # the pin's CIGARs take seconds per read there; the three functions suffice
        marked, n_pri, fin, sels, oms = [], [], [], {0: [], 1: []}, {0: [], 1: []}
        for p in range(len(reads) // 2):
            pid = pid0 + p
            raw = [reads[2 * p], reads[2 * p + 1]]
            m, npri = zip(*[rs.mark(raw[i], 2 * pid + i) for i in range(2)])
            m, npri = list(m), list(npri)
            marked += m
            n_pri += npri
            for nopair in (0, 1):
                ev = dict.fromkeys(COVERAGE_KEYS, 0)
                rec, om, a = rs.select(m, npri, pes, pid, bool(nopair), ev)
                if not big:
                    got, left = rs.sam_pe(seqs[2 * p:2 * p + 2], raw, pes, pid, bool(nopair))
                    assert all(G.region_mismatch(a[i], left[i]) is None for i in range(2)), f"case {name} pair {p}"
                    want = rs.expect_sam(seqs[2 * p:2 * p + 2], a, rec, om)
                    assert got == want, f"case {name} pair {p} nopair={nopair}: {got} != {want}"
                if nopair == 0:
                    fin += a
                sels[nopair].append(rec)
                oms[nopair] += om
        arrays[name + "_pes"] = pes
        arrays[name + "_n"] = np.array([len(a) for a in reads], np.int32)
        arrays[name + "_regs"] = cat_regs(list(reads))
        arrays[name + "_n_pri"] = np.array(n_pri, np.int32)
        arrays[name + "_marked"] = cat_regs(marked)
        arrays[name + "_final"] = cat_regs(fin)
        arrays[name + "_sel"] = np.array(sels[0], abi.PAIRSEL_DTYPE)
        arrays[name + "_sel_nopair"] = np.array(sels[1], abi.PAIRSEL_DTYPE)
        arrays[name + "_out_mapq"] = np.concatenate(oms[0]) if oms[0] else np.zeros(0, np.int32)
        arrays[name + "_out_mapq_nopair"] = np.concatenate(oms[1]) if oms[1] else np.zeros(0, np.int32)
        print(f"[gen_pair] case {name}: {len(reads) // 2} pairs, n {arrays[name + '_n'].tolist()[:8]}, "
              f"branch {[int(s['branch']) for s in sels[0]]}, o {[int(s['o']) for s in sels[0]]}", flush=True)
    o = rs.o
    path = os.path.join(out_dir, "pair_cases.npz")
    np.savez_compressed(path, **arrays, pair_id0=np.array([pid0], np.int64), alt=np.asarray(alt, np.uint8),
                        opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32), opt_mat=np.asarray(opt["mat"], np.int8),
                        selopt_int=np.array([getattr(o, k) for k in SELOPT_KEYS_I], np.int32),
                        selopt_f=np.array([getattr(o, k) for k in SELOPT_KEYS_F], np.float32))
    size = os.path.getsize(path)
    print(f"[gen_pair] pair_cases.npz: {size} bytes")
    if size > MAX_BYTES:
        raise SystemExit(f"pair_cases.npz is {size} bytes (> {MAX_BYTES})")


def main():
    out_dir = GOLD
    total = dict.fromkeys(COVERAGE_KEYS, 0)

    def add(cov):
        for k in COVERAGE_KEYS:
            total[k] += int(cov[k])

    po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
              mask_level_redun=0.95, mask_level=0.50)
    refd = G.load_ref()
    opt = abi.default_opt()
    alt2 = np.zeros(len(refd["ann_len"]), np.uint8)
    alt2[2] = 1
    make_cases(refd, opt, po, alt2, out_dir)

    rng = np.random.default_rng(20240901)
    reads = split_library(rng, refd, 1200)
    seqs = [rng.integers(0, 4, 150).astype(np.uint8) for _ in reads]
    rs = RefSel(opt, po, refd, alt2)
    pes = hand_pes()
    extra = dict(in_regs=cat_regs(reads), pes=pes, alt=alt2, opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32),
                 opt_mat=np.asarray(opt["mat"], np.int8))
    add(run_set("split", rs, pes, seqs, reads, PAIR_ID0["split"], out_dir, extra))

    for name in RIO.RESCUE_SETS:
        s = RIO.load(name)
        rs = RefSel(s.opt, dict(po, max_matesw=int(s.pairopt().max_matesw)), s.genome, s.alt)
        off = RIO.offsets(s.out_n)
        regs = [s.out_regs[o:o + k] for o, k in zip(off, s.out_n)]
        seqs = [s.seq[s.seq_off[r]:s.seq_off[r + 1]] for r in range(s.n_reads)]
        add(run_set(name, rs, s.pes, seqs, regs, PAIR_ID0[name], out_dir))

    print("[gen_pair] coverage over all sets:", total)
    short = {k: (total[k], FLOORS[k]) for k in FLOORS if total[k] < FLOORS[k]}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")


if __name__ == "__main__":
    main()
