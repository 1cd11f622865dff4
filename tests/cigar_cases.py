"""mem_reg2aln job families at the internal boundaries of the CIGAR kernel
(reg2aln_kernel, bwa-flow_amd/csrc/reg2aln.hip with global_dp.h).  Plain numpy,
no GPU.  Every read is a window of the golden genome (golden_io.load_ref())
changed by explicit edits at stated positions; the only random bytes are the
clipped-off read ends (a fixed-seed filler).  Every construction exists on both
strands: the reverse job is the reverse complement of the read on the mirrored
window (tags end in /f and /r).

A family is one option set, 20..150 jobs, the capacities to call with, and per
job what it claims to reach (Family.expect, asserted by tests/test_cigar_cases.py
from the instrumented oracle entry, oracle_reg2aln_batch_extremes):

  ncol, w      DP columns and band of the LAST bwa_gen_cigar2 call
  frame        "band1" (2w+1 <= 64), "band2" (<= 128, kernels with CD >= 2), "col"
  tries, w2s   number of calls and the w2 of each; ungapped: the last call was the shortcut
  run          {op: n}: the longest raw run of op ("M", "I", "D") is exactly n
  diag         (least, largest) diagonal k - i of the cells the last call's backtrack reads; the band is [-w, w]
  first, last  the raw CIGAR's first / last op
  cigar        the final CIGAR string
  md_nums      numbers that stand in the MD; md_dels: lengths of its deletions
  status       the record's status (default ALN_OK)

Band arithmetic (bwa.c:152-159, default scoring, dl = |rl - lq|):
mg = ((lq + 1) >> 1) - 5, w = max(min((mg + dl + 1) >> 1, w2), dl + 3).  With
dl = 0 and a generous w2 that is 63 columns for lq 131..134, 65 for 135..138, 127
for 259..262, 129 for 263..266.  infer_bw (bwamem.c:801-808) for lq == rl gives
w2 = lq - truesc - 4, and 0 below lq - truesc = 12; w2 > opt.w is cut to the
region's w.

Lowest-complexity windows of the golden genome (searched once, period p = the
longest run of seq[i] == seq[i - p]): homopolymer 34 bases at 868921,
dinucleotide repeat 483 bases at 770338, trinucleotide repeat 268 bases at
898878.  The `ties` families put their reads there.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np

import golden_io
from bwagpu import abi

SEG_LQ = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1022, 1023)
RUN_LENS = (63, 64, 65, 127, 128, 129)
END_LENS = (1, 63, 64, 65)
HOMO, DINUC, TRINUC = (868921, 34), (770338, 483), (898878, 268)
OPS = "MIDS"

_REF = golden_io.load_ref()
L_PAC = int(_REF["l_pac"])
_x = np.arange(L_PAC)
SEQ = ((_REF["pac"][_x >> 2] >> ((~_x & 3) << 1)) & 3).astype(np.uint8)
del _x
CONTIGS = [(int(o), int(o) + int(n)) for o, n in zip(_REF["ann_offset"], _REF["ann_len"])]


@dataclass
class Family:
    opt: dict
    tasks: np.ndarray
    qpool: np.ndarray
    tags: list
    expect: list                  # per job: the claims (module docstring)
    reaches: str                  # what the family is for
    calls: list = field(default_factory=lambda: [(64, 512)])   # (max_ops, max_md) of each call
    victims: list = field(default_factory=list)                # capacity: per call (job, overflows, "md" / "ops") or None
    flip_min: int = 0             # ties: at least this many jobs' raw CIGAR changes under oracle.FLIP_ME


def _opt(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100):
    return dict(a=a, b=b, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, pen_clip5=5, pen_clip3=5, w=w,
                zdrop=100, mat=abi.fill_scmat(a, b))


def other(b):
    return (np.asarray(b, np.int64) + 2) & 3


def revcomp(read):
    r = np.asarray(read, np.uint8)[::-1]
    return np.where(r < 4, 3 - r, 4).astype(np.uint8)


def read_of(p, lq, edits=()):
    """a read of lq bases from the window that starts at p -> (read, rl).  edits, in query columns:
    ("X", c) mismatch, ("N", c) an N, ("D", c, n) n window bases skipped before column c (c = lq: after
    the last), ("I", c, n) columns c..c+n-1 are inserted bases (each differs from the window base it
    would meet on the diagonal)"""
    at = {}
    for e in edits:
        at.setdefault(e[1], []).append(e)
    read, t, c = [], p, 0
    while c < lq:
        ins = None
        for e in at.get(c, ()):
            if e[0] == "D":
                t += e[2]
            elif e[0] == "I":
                ins = e[2]
        if ins:
            read += [int((int(SEQ[t + k]) + 1 + k % 3) & 3) for k in range(ins)]
            c += ins
            at.pop(c - ins)
            continue
        b = int(SEQ[t])
        for e in at.get(c, ()):
            b = int(other(b)) if e[0] == "X" else (4 if e[0] == "N" else b)
        read.append(b)
        t += 1
        c += 1
    for e in at.get(lq, ()):
        if e[0] == "D":
            t += e[2]
    assert len(read) == lq, (len(read), lq)
    return np.array(read, np.uint8), t - p


class _Build:
    def __init__(self, seed=5):
        self.rng = np.random.default_rng(seed)   # the clipped-off read ends only
        self.tasks, self.qs, self.qo, self.tags, self.expect = [], [], 0, [], []
        self.p = 1200                            # the next window: contigs 0 and 1, 3000 apart

    def place(self):
        self.p += 3000
        if self.p > 760000:
            self.p = 1200 + 1531
        if 495000 < self.p < 503000:
            self.p = 503000
        return self.p

    def add(self, tag, read, rb, rl, clip5=0, clip3=0, truesc=0, w=400, strands="fr", **expect):
        """read: the aligned query bases on the forward strand over [rb, rb + rl); clip5 / clip3 filler
        bases are put around it"""
        read = np.asarray(read, np.uint8)
        full = np.concatenate([self.rng.integers(0, 4, clip5), read, self.rng.integers(0, 4, clip3)]).astype(np.uint8)
        L, qb, qe = len(full), clip5, clip5 + len(read)
        for s in strands:
            if s == "f":
                job = (rb, rb + rl, self.qo, L, qb, qe, truesc, w, 0)
                q = full
            else:
                job = (2 * L_PAC - (rb + rl), 2 * L_PAC - rb, self.qo, L, L - qe, L - qb, truesc, w, 0)
                q = revcomp(full)
            self.tasks.append(job)
            self.qs.append(q)
            self.qo += L
            self.tags.append(f"{tag}/{s}")
            self.expect.append(dict(expect))

    def edited(self, tag, lq, edits=(), p=None, where=None, **kw):
        """where(p): the window start is moved on until it holds (an indel that could slide along equal bases
        would land wherever the tie order puts it: such claims belong to the `ties` families)"""
        p = self.place() if p is None else p
        while where is not None and not where(p):
            p += 1
        read, rl = read_of(p, lq, edits)
        self.add(tag, read, p, rl, **kw)

    def done(self, opt, reaches, **kw):
        return Family(opt, np.array(self.tasks, abi.REG2ALN_TASK_DTYPE), np.concatenate(self.qs).astype(np.uint8),
                      self.tags, self.expect, reaches, **kw)


def del_fixed(c, n):
    """where(p) for a deletion of n window bases before query column c (no indel before it): it cannot
    slide either way"""
    return lambda p: SEQ[p + c - 1] != SEQ[p + c + n - 1] and SEQ[p + c] != SEQ[p + c + n]


def ins_fixed(t, n):
    """where(p) for n inserted bases (read_of's) in front of window offset t: they cannot slide left (the
    first of them differs from the base at t by construction, so not right either)"""
    return lambda p: SEQ[p + t - 1] != (SEQ[p + t + n - 1] + 1 + (n - 1) % 3) & 3


def frame_of(w, lq):
    return "band1" if 2 * w + 1 <= 64 else ("band2" if 2 * w + 1 <= 128 and lq >= 64 else "col")


def _pair(lq):
    """a 2-base deletion at one third and a 2-base insertion at two thirds: lq == rl"""
    return [("D", lq // 3, 2), ("I", 2 * lq // 3, 2), ("X", lq // 2)] if lq >= 12 else []


def _band_form():
    b = _Build()
    # through lq (dl = 0, w2 = min(lq - 4, region w = 400))
    for lq, ncol in ((130, 61), (131, 63), (134, 63), (135, 65), (138, 65),
                     (258, 125), (259, 127), (262, 127), (263, 129), (266, 129)):
        w = (ncol - 1) // 2
        for name, ed in (("mm", [("X", 5), ("X", lq - 6)]), ("pair", _pair(lq))):
            b.edited(f"lq{lq}_{name}", lq, ed, ncol=ncol, w_=w, frame=frame_of(w, lq), tries=1)
    # a path along the band's own edge columns: an insertion of exactly w bases, 60 matched bases on the top
    # edge (k - i = w, the last lane position of the band frame), a deletion of w back; and the mirror image
    # along the bottom edge (k - i = -w).  A band frame that is one column short loses exactly these.
    for lq, w in ((130, 30), (134, 31), (135, 32), (258, 62), (262, 63), (263, 64), (266, 64)):
        b.edited(f"lq{lq}_top_edge", lq, [("I", 20, w), ("D", 80 + w, w)], ncol=2 * w + 1, w_=w,
                 frame=frame_of(w, lq), tries=1, run={"I": w, "D": w}, diag=(0, w), cigar=f"20M{w}I60M{w}D{lq - 80 - w}M",
                 where=lambda p, w=w: del_fixed(80, w)(p) and ins_fixed(20, w)(p))
        b.edited(f"lq{lq}_bottom_edge", lq, [("D", 20, w), ("I", 80, w)], ncol=2 * w + 1, w_=w,
                 frame=frame_of(w, lq), tries=1, run={"I": w, "D": w}, diag=(-w, 0), cigar=f"20M{w}D60M{w}I{lq - 80 - w}M",
                 where=lambda p, w=w: del_fixed(20, w)(p) and ins_fixed(80 + w, w)(p))
    # through w2 alone: truesc = lq - 4 - w2 on long reads (mg is far larger), inside CD = 16 and CD = 8
    for lq in (1023, 500):
        for w2 in (30, 31, 32, 62, 63, 64):
            for name, ed in (("mm", [("X", 70), ("X", lq - 9)]), ("pair", _pair(lq))):
                b.edited(f"lq{lq}_w2_{w2}_{name}", lq, ed, truesc=lq - 4 - w2, w=400, ncol=2 * w2 + 1, w_=w2,
                         frame=frame_of(w2, lq), tries=1, w2s=(w2,))
    # the CD = 1 kernel: band_dp<1> with ncol = lq, and straight to global_dp<1> past 64 columns
    for lq, rl, w, fr in ((40, 60, 23, "band1"), (40, 80, 43, "col"), (63, 63, 14, "band1"), (63, 91, 31, "band1"),
                          (63, 92, 32, "col"), (63, 95, 35, "col"), (1, 30, 32, "col"), (1, 29, 31, "band1")):
        dl = rl - lq
        ed = ([("D", lq // 2, dl)] if dl else []) + ([("X", 3)] if lq > 8 else [])
        # truesc = -300: the deletion's cost does not start a second call
        b.edited(f"cd1_lq{lq}_rl{rl}", lq, ed, truesc=-300, ncol=min(lq, 2 * w + 1), w_=w, frame=fr, tries=1)
        if dl and lq > 1:
            b.edited(f"cd1_lq{lq}_rl{rl}_tail", lq, [("D", lq, dl)], truesc=-300, ncol=min(lq, 2 * w + 1), w_=w,
                     frame=fr, tries=1)
    for e in b.expect:   # `w` is add()'s region band; the claimed DP band travels as w_
        if "w_" in e:
            e["w"] = e.pop("w_")
    return b.done(_opt(), "last-call band of 61/63/65 and 125/127/129 columns through lq and through w2; CD = 1: "
                  "band frame with ncol = lq, and the column frame past 64 columns")


def _seg_edits(lq):
    """mismatches on both sides of every segment edge and on the last base; a 1-base deletion after
    column 63, a 1-base insertion at column 127, a 1-base deletion before the last column"""
    ed = {}
    for c in (63, 64, 127, 128, 191, 192, 255, 256, 511, 512, lq - 1):
        if 0 <= c < lq:
            ed[c] = ("X", c)
    if lq > 70:
        ed[64] = ("D", 64, 1)
    if lq > 140:
        ed[127] = ("I", 127, 1)
    if lq > 200:
        ed[lq - 2] = ("D", lq - 2, 1)
    return list(ed.values())


def _segments():
    b = _Build()
    for lq in SEG_LQ:
        cd = (lq + 64) >> 6
        # narrow: the region's w = 10 cuts a w2 above opt.w; short reads have a narrow mg anyway
        # (truesc below 0: no shortcut for the shortest reads, and one call whatever the edits cost)
        b.edited(f"lq{lq}_narrow", lq, _seg_edits(lq), truesc=-20, w=10, frame="band1", tries=1, cd=cd)
        # past 128 columns: lq >= 263 has mg >= 127; shorter reads get there by dl = 61 (w = dl + 3 = 64)
        if lq >= 263:
            b.edited(f"lq{lq}_wide", lq, _seg_edits(lq), truesc=0, w=400, frame="col", tries=1, cd=cd)
        xs = [e for e in _seg_edits(lq) if e[0] == "X"]
        c = next(c for c in (max(lq // 2, 1), lq // 3, lq // 2 + 20) if all(abs(c - e[1]) > 4 for e in xs) or lq < 9)
        ed = xs + [("D", c, 61)]
        b.edited(f"lq{lq}_wide_del61", lq, ed, truesc=-300, w=400, where=del_fixed(c, 61) if lq > 1 else None, frame="col", tries=1, cd=cd, run={"D": 61})
    # the HBM slice at its largest: 1023 bases with a 128-base deletion, w = 318, 637 x 1151 bytes
    b.edited("lq1023_del128_hbm", 1023, [("D", 510, 128), ("X", 63), ("X", 1022)], truesc=0, w=400, frame="col",
             w_=318, ncol=637, cd=16, run={"D": 128}, cigar="510M128D513M", where=del_fixed(510, 128))
    for e in b.expect:
        if "w_" in e:
            e["w"] = e.pop("w_")
    return b.done(_opt(), "every CD bucket once in the band frame and once in the column frame; the score lane at "
                  "ql = 64k; H/F/E hand-offs at columns 63/64, 127/128, ...")


def _runs():
    b = _Build()
    for n in RUN_LENS:
        b.edited(f"M{n}_whole", n, [], run={"M": n}, cigar=f"{n}M")
        b.edited(f"M{n}_then_del", n + 40, [("D", n, 1)], run={"M": n}, cigar=f"{n}M1D40M",
                 where=lambda p, n=n: SEQ[p + n] != SEQ[p + n - 1] and SEQ[p + n] != SEQ[p + n + 1])
        b.edited(f"ins_then_M{n}", n + 41, [("I", 40, 1)], run={"M": n}, cigar=f"40M1I{n}M",
                 where=lambda p: (SEQ[p + 40] + 1) & 3 != SEQ[p + 39])
        b.edited(f"D{n}_in150", 150, [("D", 74, n)], run={"D": n}, first="M", last="M", cigar=f"74M{n}D76M",
                 where=del_fixed(74, n))
        b.edited(f"I{n}_in400", 400, [("I", 200, n)], run={"I": n}, first="M", last="M")
        b.edited(f"D{n}_in1023", 1023, [("D", 510, n)], run={"D": n}, cigar=f"510M{n}D513M", where=del_fixed(510, n))
        b.edited(f"I{n}_in1023", 1023, [("I", 510, n)], run={"I": n})
    for n in END_LENS:
        b.edited(f"lead_I{n}", 100 + n, [("I", 0, n)], run={"I": n}, first="I", cigar=f"{n}I100M")
        b.edited(f"trail_I{n}", 100 + n, [("I", 100, n)], run={"I": n}, last="I", cigar=f"100M{n}I",
                 where=lambda p, n=n: SEQ[p + 99] != (SEQ[p + 99 + n] + 1 + (n - 1) % 3) & 3)
        b.edited(f"lead_D{n}", 100, [("D", 0, n)], run={"D": n}, first="D", cigar="100M")
        b.edited(f"trail_D{n}", 100, [("D", 100, n)], run={"D": n}, last="D", cigar="100M",
                 where=lambda p, n=n: SEQ[p + 99] != SEQ[p + 99 + n])
    # the entry's own worked examples
    b.edited("ex_150_del63", 150, [("D", 74, 63)], cigar="74M63D76M", where=del_fixed(74, 63))
    b.edited("ex_150_del64", 150, [("D", 74, 64)], cigar="74M64D76M", where=del_fixed(74, 64))
    b.edited("ex_250_ins64", 250, [("I", 125, 64)], cigar="125M64I61M")
    return b.done(_opt(), "single M, I and D runs of 63..129 cells (the 64-cell ballot and its f == 64 branch); "
                  "runs that end at i < 0 or kk < 0 (the two end pushes)")


def _squeeze_clip():
    b = _Build()
    c0, c1, c2 = CONTIGS
    # windows: mid-contig, starting on a contig's first base, ending on a contig's last base, ending at l_pac - 1
    spots = (("mid", 31000, None), ("start0", c0[0], None), ("start1", c1[0], None), ("end0", None, c0[1]),
             ("end1", None, c1[1]), ("endpac", None, c2[1]))
    shapes = (("leadD", 5, 0), ("trailD", 0, 4), ("bothD", 5, 4), ("noD", 0, 0))
    clips = (("noclip", 0, 0), ("clip5", 7, 0), ("clip3", 0, 3), ("clips", 7, 3))
    lq = 90
    for spot, beg, end in spots:
        for shape, d0, d1 in shapes:
            # an end deletion is unambiguous when the read's end base differs from the window's: lengthen it until so
            def start(d0, d1):
                return beg if beg is not None else end - (lq + d0 + d1)
            while d0 and SEQ[start(d0, d1) + d0] == SEQ[start(d0, d1)]:
                d0 += 1
            while d1 and SEQ[start(d0, d1) + d0 + lq - 1] == SEQ[start(d0, d1) + d0 + lq + d1 - 1]:
                d1 += 1
                while d0 and SEQ[start(d0, d1) + d0] == SEQ[start(d0, d1)]:
                    d0 += 1
            for cname, c5, c3 in clips:
                if spot != "mid" and cname in ("clip5", "clip3") and shape != "bothD":
                    continue   # the full clip cross stays on the mid window and on bothD
                rl = lq + d0 + d1
                p = start(d0, d1)
                ed = ([("D", 0, d0)] if d0 else []) + ([("D", lq, d1)] if d1 else []) + [("X", 30)]
                read, rl2 = read_of(p, lq, ed)
                assert rl2 == rl
                # the squeeze is an else-if: with both, the trailing deletion stays in the CIGAR
                exp = dict(n_ops=1 + (d0 > 0 and d1 > 0) + (c5 > 0) + (c3 > 0), run={"D": max(d0, d1)} if d0 or d1 else {})
                if d0:
                    exp["first"] = "D"
                if d1:
                    exp["last"] = "D"
                b.add(f"{spot}_{shape}_{cname}", read, p, rl, clip5=c5, clip3=c3, **exp)
    return b.done(_opt(), "CIGAR beginning with D (pos moves), ending with D (dropped), both (only the leading one "
                  "goes); clips on either side and both, swapped on the reverse strand; windows on contig and pac ends")


def _md_edges():
    b = _Build()
    for off in (0, 63, 64, 65, 127, 128, 199):
        b.edited(f"mm_at{off}", 200, [("X", off)], cigar="200M", md_nums=[off, 199 - off])
    b.edited("mm_63_64", 200, [("X", 63), ("X", 64)], cigar="200M", md_nums=[63, 0, 135])
    b.edited("mm_0_last", 200, [("X", 0), ("X", 199)], cigar="200M", md_nums=[0, 198, 0])
    b.edited("mm_all_edges", 200, [("X", c) for c in (0, 63, 64, 65, 127, 128, 199)], cigar="200M")
    for n in (64, 128, 192):
        b.edited(f"run{n}_whole", n, [], cigar=f"{n}M", md_nums=[n])
        b.edited(f"run{n}_lastmm", n, [("X", n - 1)], cigar=f"{n}M", md_nums=[n - 1, 0])
        b.edited(f"run{n}_del_run{n}", 2 * n, [("D", n, 1)], cigar=f"{n}M1D{n}M", md_nums=[n, n], md_dels=[1],
                 where=lambda p, n=n: SEQ[p + n] != SEQ[p + n - 1] and SEQ[p + n] != SEQ[p + n + 1])
    # N scores -1: a block of N stays in the M run (gaps would cost 2 (6 + n)), and every N is a mismatch
    for n, at in ((64, 0), (64, 64), (64, 32), (65, 0), (65, 63), (128, 0)):
        b.edited(f"N{n}_at{at}", 260, [("N", c) for c in range(at, at + n)], cigar="260M",
                 md_nums=[at] + [0] * (n - 1) + [260 - at - n], nm=n)
    b.edited("N_single", 100, [("N", 50)], cigar="100M", md_nums=[50, 49], nm=1)
    for n in (9, 10, 99, 100, 999, 1000):
        b.edited(f"count{n}", 1023, [("X", 7), ("X", 8 + n)], cigar="1023M", md_nums=[7, n, 1023 - 9 - n])
    for n in (1, 9, 10):
        b.edited(f"del{n}", 150, [("D", 70, n)], md_dels=[n], md_nums=[70, 80], where=del_fixed(70, n))
    return b.done(_opt(), "mismatches at offsets 0/63/64/65/127/128 and on the last base of a run; runs of 64, 128, "
                  "192; 64 and 65 mismatches in a row; N; MD numbers of 1..4 digits; deletions of 1, 9, 10")


def _band_loop():
    b = _Build()
    lq = 150
    mm = [("X", 20), ("X", 90)]                                   # score 150 - 10 = 140
    # one call, stopped by score >= truesc - a; w2 <= opt.w ignores the region's w
    b.edited("one_w2_50", lq, mm, truesc=lq - 4 - 50, w=0, tries=1, w2s=(50,))
    # the region's w below, equal to and above an inferred w2 of 146 (> opt.w = 100)
    for rw, w2 in ((145, 145), (146, 146), (147, 146), (100, 100), (99, 99)):
        b.edited(f"regw{rw}", lq, mm, truesc=0, w=rw, tries=1, w2s=(w2,))
    # infer_bw's zero boundary, lq == rl: lq - truesc = 11 -> 0 (the shortcut, twice: 0 << 1 = 0, score == last);
    # 12 -> 8, then 16 with the same score
    mm4 = mm + [("X", 40), ("X", 120)]                            # score 130 < truesc - a at both
    b.edited("zero_in", lq, mm4, truesc=lq - 11, tries=2, w2s=(0, 0), ungapped=True, cigar="150M")
    b.edited("zero_out", lq, mm4, truesc=lq - 12, tries=2, w2s=(8, 16), ungapped=False, cigar="150M")
    b.edited("zero_in_clean", lq, [], truesc=lq - 11, tries=1, w2s=(0,), ungapped=True)   # score 150 >= truesc - a
    # lq != rl at the same two values: no shortcut (w2 >= dl), one deletion
    for ts in (lq - 11, lq - 12):
        b.edited(f"nozero_ts{ts}", lq, [("D", 70, 1)] + mm4, truesc=ts, ungapped=False, tries=2)
    # three calls: a 12-base deletion and a 12-base insertion are out of reach of w = 8, inside w = 16;
    # the third call (32) finds nothing more and tries == 3 ends the loop
    far = [("D", 50, 12), ("I", 100, 12)]
    b.edited("three", lq, far, truesc=lq - 12, tries=3, w2s=(8, 16, 32), frame="band2")
    b.edited("three_400", 400, [("D", 100, 12), ("I", 300, 12)], truesc=400 - 12, tries=3, w2s=(8, 16, 32))
    # two calls ended by score == last with a gapped first call
    b.edited("two_same", lq, [("D", 50, 2), ("I", 100, 2)], truesc=lq - 12, tries=2, w2s=(8, 16))
    # w2 == wmax on the first call (the region's w does not cut below 400) ...
    b.edited("wmax_first", lq, mm, truesc=-400, w=1000, tries=1, w2s=(400,))
    b.edited("wmax_first_eq", lq, mm, truesc=lq - 4 - 400, w=400, tries=1, w2s=(400,))
    b.edited("below_wmax", lq, mm, truesc=lq - 4 - 399, w=399, tries=1, w2s=(399,))
    # ... and on the second: w2 = 200, a read of 60 mismatches scores 150 - 300 < truesc - a = -55
    junk = [("X", c) for c in range(5, 145, 7)] + [("X", c) for c in range(6, 146, 7)] + \
           [("X", c) for c in range(7, 147, 7)]
    b.edited("wmax_second", lq, junk, truesc=lq - 4 - 200, w=200, tries=2, w2s=(200, 400))
    # ... and on the third: 1023 bases (w = min(254, w2)), a 120-base indel pair within reach of w2 = 200 only,
    # a 230-base pair within reach of w2 = 400 only: the score changes at every call
    b.edited("wmax_third", 1023, [("D", 200, 120), ("I", 400, 120), ("D", 600, 230), ("I", 760, 230)],
             truesc=1023 - 4 - 100, w=400, tries=3, w2s=(100, 200, 400), frame="col")
    return b.done(_opt(), "1, 2 and 3 bwa_gen_cigar2 calls; both stop rules (score == last, w2 == wmax); the region's "
                  "w below / at / above w2; truesc on both sides of infer_bw's zero, with and without lq == rl")


def _ties(opt, name):
    """reads inside the genome's repeats, with indels of whole and of partial repeat units"""
    b = _Build()
    for rname, (at, n) in (("dinuc", DINUC), ("trinuc", TRINUC), ("homo", HOMO)):
        unit = dict(dinuc=2, trinuc=3, homo=1)[rname]
        for lq in ((60, 150, 300) if n > 400 else ((60, 150) if n > 200 else (20, 30))):
            p = at + max((n - lq) // 2 - 8, 2)
            for d in (1, unit, 2 * unit) if unit > 1 else (1, 2, 4):   # part of a unit, one unit, two
                b.edited(f"{rname}_lq{lq}_del{d}", lq, [("D", lq // 2, d)], p=p)
                b.edited(f"{rname}_lq{lq}_ins{d}", lq, [("I", lq // 2, d)], p=p)
                b.edited(f"{rname}_lq{lq}_mm_del{d}", lq, [("X", lq // 3), ("D", 2 * lq // 3, d)], p=p)
    return b.done(opt, f"{name}: ties are the rule inside repeats; the tie order (m >= e, h >= f, ed > te, fd > tf) "
                  "decides where each indel lands", flip_min=len(b.tasks) // 4)


def _limits(opt, name):
    """truesc = -300000: l a - truesc stays above infer_bw's zero boundary 2 (o + e - a) at every option set
    here, so that no job ends in the ungapped shortcut, and every job makes one call (-2^23 where a forced
    61-base deletion costs 62 x 65535)"""
    b = _Build()
    ts = -300000
    for lq in (64, 257, 1023):
        for rw in (20, 400):   # a band cut by the region's w, and whatever mg allows
            b.edited(f"lq{lq}_w{rw}_mm", lq, [("X", 3), ("X", lq - 2)], w=rw, truesc=ts, tries=1, ungapped=False)
            b.edited(f"lq{lq}_w{rw}_del1", lq, [("D", lq // 2, 1), ("X", lq // 4)], w=rw, truesc=ts, tries=1, ungapped=False)
            b.edited(f"lq{lq}_w{rw}_ins1", lq, [("I", lq // 2, 1), ("X", lq // 4)], w=rw, truesc=ts, tries=1, ungapped=False)
            b.edited(f"lq{lq}_w{rw}_pair", lq, _pair(lq), w=rw, truesc=ts, tries=1, ungapped=False)
        # the column frame whatever mg says: dl = 61 forces w >= 64
        b.edited(f"lq{lq}_del61", lq, [("D", lq // 2, 61)], w=400, truesc=-(1 << 23), frame="col", tries=1)
        b.edited(f"lq{lq}_tail61", lq, [("D", lq, 61), ("X", lq // 2)], w=400, truesc=-(1 << 23), frame="col", tries=1)
    return b.done(opt, f"{name}: every intermediate of the DP stays strictly inside int32 at the option limits "
                  "make_opt admits", calls=[(64, 2304)])   # a read of mismatches alone: MD of 2 lq + 2 bytes


TIE_OPTS = {
    "ties_unit": _opt(a=1, b=1, o_del=0, e_del=1, o_ins=0, e_ins=1),
    "ties_odel0": _opt(o_del=0, o_ins=6),
    "ties_eneq": _opt(a=2, b=2, o_del=2, e_del=2, o_ins=2, e_ins=1),
    "ties_b1": _opt(a=1, b=1, o_del=1, e_del=1, o_ins=1, e_ins=1),
}
LIMIT_OPTS = {
    "limits_a127": _opt(a=127, b=127),
    "limits_gap_max": _opt(a=127, b=127, o_del=65535, e_del=65535, o_ins=65535, e_ins=65535),
    "limits_ins_cheap": _opt(a=127, b=127, o_del=65535, e_del=65535, o_ins=1, e_ins=1),
    "limits_del_cheap": _opt(a=127, b=127, o_del=1, e_del=1, o_ins=65535, e_ins=65535),
    "limits_mixed": _opt(a=127, b=127, o_del=1, e_del=65535, o_ins=65535, e_ins=1),
    "limits_a1_gap_max": _opt(a=1, b=4, o_del=65535, e_del=1, o_ins=1, e_ins=65535),
}

# capacity: the jobs whose md_len / n_cigar set the capacities, taken from the families above
CAPACITY_JOBS = (("md_edges", "count999"), ("md_edges", "N65_at63"), ("md_edges", "del10"), ("runs", "D64_in150"),
                 ("squeeze_clip", "mid_bothD_noclip"), ("squeeze_clip", "mid_bothD_clips"),
                 ("squeeze_clip", "mid_leadD_clip5"), ("squeeze_clip", "end1_trailD_clips"),
                 ("runs", "lead_I64"), ("band_loop", "three"))


def _capacity(fams):
    """the chosen jobs (both strands) in one batch; per victim four calls: max_md = md_len + 1 (fits) and
    md_len (overflows), max_ops = n_cigar (fits) and n_cigar - 1 (overflows).  md_len and n_cigar are the
    oracle's at generous capacities."""
    import oracle
    tasks, qs, tags, qo = [], [], [], 0
    for fam, tag in CAPACITY_JOBS:
        f = fams[fam]
        for s in "fr":
            k = f.tags.index(f"{tag}/{s}")
            t = f.tasks[k].copy()
            q = f.qpool[int(t["qoff"]):int(t["qoff"]) + int(t["l_seq"])]
            t["qoff"] = qo
            qo += len(q)
            tasks.append(t)
            qs.append(q)
            tags.append(f"{fam}.{tag}/{s}")
    tasks, qpool = np.array(tasks, abi.REG2ALN_TASK_DTYPE), np.concatenate(qs)
    R = oracle.Ref(_REF["l_pac"], _REF["ann_offset"], _REF["ann_len"], _REF["pac"])
    out, _, _ = oracle.reg2aln("oracle", _opt(), R, tasks, qpool, 64, 512)
    assert (out["status"] == abi.ALN_OK).all()
    calls, victims = [(64, 512)], [None]
    for k in range(0, len(tasks), 2):           # the forward job of each pair, the reverse one of every other
        v = k + (k // 2) % 2
        ml, nc = int(out["md_len"][v]), int(out["n_cigar"][v])
        calls += [(64, ml + 1), (64, ml)]
        victims += [(v, False, "md"), (v, True, "md")]
        if nc > 1:                              # max_ops = 0 is an argument error
            calls += [(nc, 512), (nc - 1, 512)]
            victims += [(v, False, "ops"), (v, True, "ops")]
    return Family(_opt(), tasks, qpool, tags, [dict() for _ in tags], "max_md = md_len + 1 / md_len and max_ops = "
                  "n_cigar / n_cigar - 1, with and without clips: ALN_OVERFLOW exactly past the capacity",
                  calls=calls, victims=victims)


FAMILY_NAMES = ("band_form", "segments", "runs", "squeeze_clip", "md_edges", "band_loop", "capacity") + \
    tuple(TIE_OPTS) + tuple(LIMIT_OPTS)
_FAMS = None


def families() -> dict:
    """-> {name: Family}, built once"""
    global _FAMS
    if _FAMS is None:
        f = dict(band_form=_band_form(), segments=_segments(), runs=_runs(), squeeze_clip=_squeeze_clip(),
                 md_edges=_md_edges(), band_loop=_band_loop())
        f["capacity"] = _capacity(f)
        for name, opt in TIE_OPTS.items():
            f[name] = _ties(opt, name)
        for name, opt in LIMIT_OPTS.items():
            f[name] = _limits(opt, name)
        assert tuple(f) == FAMILY_NAMES
        _FAMS = f
    return _FAMS


def cigar_str(ops):
    return "".join(f"{int(v) >> 4}{OPS[int(v) & 0xf]}" for v in ops)


def md_parts(md: bytes):
    """-> (the numbers, the deletion lengths) of an MD string"""
    s = md.decode()
    return [int(x) for x in re.findall(r"\d+", s)], [len(x) - 1 for x in re.findall(r"\^[A-Z]+", s)]


def claim_failures(f: Family, out, cig, md, ext, X) -> list:
    """every claim of Family.expect that the oracle's outputs and extremes (oracle.reg2aln_extremes at the
    family's first capacities; X = oracle.R2X) do not bear out -> ["tag: what"]"""
    bad = []
    for k, (tag, e) in enumerate(zip(f.tags, f.expect)):
        x = ext[k]
        n = int(x[X["tries"]])
        lq = int(f.tasks["qe"][k] - f.tasks["qb"][k])
        last_w, last_ncol = int(x[X["w"] + n - 1]), int(x[X["ncol"] + n - 1])
        ops = cigar_str(cig[k, :int(out["n_cigar"][k])])
        nums, dels = md_parts(bytes(md[k, :int(out["md_len"][k])]))
        got = dict(status=int(out["status"][k]), tries=n, w2s=tuple(int(v) for v in x[X["w2"]:X["w2"] + n]),
                   ungapped=bool(x[X["ungapped"]]), first="MID"[int(x[X["first"]])], last="MID"[int(x[X["last"]])],
                   cigar=ops, w=last_w, ncol=last_ncol, cd=(lq + 64) >> 6, nm=int(out["NM"][k]),
                   n_ops=int(out["n_cigar"][k]), diag=(int(x[X["diag_min"]]), int(x[X["diag_max"]])),
                   frame=None if x[X["ungapped"]] else frame_of(last_w, lq))
        for key, want in dict(e, status=e.get("status", abi.ALN_OK)).items():
            if key == "run":
                for op, ln in want.items():
                    have = int(x[X["run_" + op.lower()]])
                    if have != ln:
                        bad.append(f"{tag}: longest {op} run {have}, claimed {ln}")
            elif key == "md_nums":
                if key == "md_nums" and nums != list(want):
                    bad.append(f"{tag}: MD numbers {nums[:8]}..., claimed {list(want)[:8]}...")
            elif key == "md_dels":
                if dels != list(want):
                    bad.append(f"{tag}: MD deletions {dels}, claimed {want}")
            elif got[key] != want:
                bad.append(f"{tag}: {key} {got[key]}, claimed {want}")
    return bad
