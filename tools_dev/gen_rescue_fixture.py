#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY: tests/golden/rescue_<set>.npz and
rescue_pestat_cases.npz, the expected results of bwagpu_pestat and
bwagpu_mate_rescue, made by the reference's own mem_pestat and mem_matesw
(oracle/_ref/libbwaref.so, loaded through ctypes).

    make -C oracle ref && python tools_dev/gen_rescue_fixture.py

Every set is a simulated paired-end library (reads 2i and 2i+1 are pair i),
seeded, chained and extended by the reference's own code against a bwa index
built here in a temporary directory, then post-processed per read as
RegionsToSam::compute does (mem_sort_dedup_patch and the is_alt loop: the input
bwagpu_mate_rescue takes).  mem_pestat is called on those regions; the rescue
loop of mem_sam_pe (bwamem_pair.c:271-277, ten lines restated here) calls the
reference's mem_matesw on mem_alnreg_v structs whose arrays come from libc
malloc (the function reallocs them).

Coverage counts come from a second, observing walk of every mem_matesw call in
this script (skip test, windows, the reference's ksw_align2 and
mem_sort_dedup_patch through ctypes) that must reproduce mem_matesw's return
value and its resulting regions byte for byte.  The script exits non-zero
unless the floors below are met over all sets together.

Sets (all but `rep*` on the golden genome, tests/golden/ref.npz):
  fr       FR library; mates that are clean, unseedable (a substitution every
           15th base), half junk, or random
  mixed    half FR, half RF: two orientations stay alive
  shift    a tight FR library whose mates start with 45-70 junk bases: the mate's
           own region falls just out of range, the rescue finds it again and the
           dedup removes one of the two
  ends     pairs at contig ends and around l_pac (windows clamped, clipped to
           the contig, or rejected by the rid gate); contig 1 is ALT
  rep      the set's own 120 kbp genome with tandem duplications (4 x 300 bp
           and 24 x 200 bp families): several candidates per read, calls the
           first rescue makes unnecessary, rescued regions the dedup removes
  rep_sw2  the same reads with max_matesw = 2
The C5 genome has three contigs like the golden one and its index takes minutes
to build, so the slice with many contigs is `ends` on the golden genome.
Pairs in which the reference grows a read by more than HEADROOM regions are left
out of a set (see run_pairs): the tests' output spans are n + HEADROOM regions.
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"), HERE):
    sys.path.insert(0, p)

import golden_io as G  # noqa: E402
import oracle  # noqa: E402
from bwagpu import abi  # noqa: E402
from bwagpu.engine import Batch, compact  # noqa: E402
from gen_post_fixture import BntSeq, MemOpt, RefPost, build_index, genome_bases  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
MAX_BYTES = 1 << 20
HEADROOM = 8  # regions of room per read beyond its input count in the tests' output spans
COVERAGE_KEYS = ("pairs_sw", "regs_added", "regs_added_rev", "regs_added_to_empty", "sw_no_region", "dedup_removed",
                 "windows_changed", "windows_rejected", "pairs_multi_cand", "calls_cut", "pairs_multi_orient",
                 "spec_ignored", "reads_over_17", "needed_not_speculated")
FLOORS = dict(pairs_sw=200, regs_added=100, regs_added_rev=30, regs_added_to_empty=30, sw_no_region=20,
              dedup_removed=10, windows_changed=10, windows_rejected=5, pairs_multi_cand=20, calls_cut=5,
              pairs_multi_orient=20, spec_ignored=5, reads_over_17=1)  # needed_not_speculated: recorded, no floor
PAIROPT_KEYS = ("max_ins", "max_matesw", "pen_unpaired", "min_seed_len", "max_chain_gap")
XBYTE, XSUBO, XSTART = 0x10000, 0x40000, 0x80000


class AlnRegV(C.Structure):  # mem_alnreg_v, bwa/bwamem.h:80
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class Kswr(C.Structure):  # kswr_t, bwa/ksw.h:14-19
    _fields_ = [(k, C.c_int) for k in ("score", "te", "qe", "score2", "te2", "tb", "qb")]


libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]
REG = abi.ALNREG_DTYPE.itemsize


def infer_dir(l_pac, b1, b2):
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else (l_pac << 1) - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


class RefPair:
    """the reference's mem_pestat / mem_matesw, and the observing walk"""

    def __init__(self, opt: dict, pairopt: dict, refd, alt):
        self.rp = rp = RefPost(opt, (pairopt["max_chain_gap"], pairopt["mask_level_redun"], pairopt["mask_level"]),
                               refd, alt)
        self.lib, self.o = rp.lib, rp.o
        o = self.o
        for k in ("max_ins", "max_matesw", "pen_unpaired", "min_seed_len"):
            setattr(o, k, int(pairopt[k]))
        self.l_pac = rp.l_pac
        self.ann_off = np.asarray(refd["ann_offset"], np.int64)
        self.ann_len = np.asarray(refd["ann_len"], np.int64)
        self.both = self.strands(refd)
        vp = C.c_void_p
        lib = self.lib
        lib.mem_pestat.argtypes = [C.POINTER(MemOpt), C.c_int64, C.c_int, vp, vp]
        lib.mem_pestat.restype = None
        lib.mem_matesw.argtypes = [C.POINTER(MemOpt), C.POINTER(BntSeq), vp, vp, vp, C.c_int, vp, C.POINTER(AlnRegV)]
        lib.mem_matesw.restype = C.c_int
        lib.ksw_align2.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.c_int] * 5 + [vp]
        lib.ksw_align2.restype = Kswr

    @staticmethod
    def strands(refd):
        """bns_get_seq's two strands; the walk reads window slices [rb:re) of it"""
        g = genome_bases(refd).astype(np.uint8)
        return np.concatenate([g, (3 - g[::-1]).astype(np.uint8)])

    def pestat(self, regs_by_read):
        """mem_pestat over per-read region arrays -> PESTAT_DTYPE[4]"""
        n = len(regs_by_read)
        keep = [np.ascontiguousarray(a, abi.ALNREG_DTYPE) for a in regs_by_read]
        v = (AlnRegV * max(n, 1))()
        for i, a in enumerate(keep):
            v[i].n = v[i].m = len(a)
            v[i].a = a.ctypes.data if len(a) else None
        pes = np.zeros(4, abi.PESTAT_DTYPE)
        self.lib.mem_pestat(C.byref(self.o), self.l_pac, n, C.cast(v, C.c_void_p), pes.ctypes.data)
        return pes

    # ---- the real call
    @staticmethod
    def to_v(a):
        v = AlnRegV()
        v.n = len(a)
        v.m = max(len(a), 1)
        v.a = libc.malloc(v.m * REG)
        if len(a):
            C.memmove(v.a, a.ctypes.data, len(a) * REG)
        return v

    @staticmethod
    def from_v(v):
        out = np.zeros(v.n, abi.ALNREG_DTYPE)
        if v.n:
            C.memmove(out.ctypes.data, v.a, v.n * REG)
        return out

    def matesw(self, pes, a1, ms, v):
        a1 = np.ascontiguousarray(a1)
        ms = np.ascontiguousarray(ms, np.uint8)
        return self.lib.mem_matesw(C.byref(self.o), C.byref(self.rp.bns), self.rp.pac.ctypes.data, pes.ctypes.data,
                                   a1.ctypes.data, len(ms), ms.ctypes.data, C.byref(v))

    # ---- the observing walk
    def skip(self, pes, arb, ma):
        s = [int(pes["failed"][r] != 0) for r in range(4)]
        for x in ma:
            r, d = infer_dir(self.l_pac, arb, int(x["rb"]))
            if pes["low"][r] <= d <= pes["high"][r]:
                s[r] = 1
        return s

    def window(self, pes, arb, arid, l_ms, r):
        """-> (rb, re, gate ok, changed by the clamps or the contig clip)"""
        L2 = self.l_pac << 1
        is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
        lo, hi = int(pes["low"][r]), int(pes["high"][r])
        if not is_rev:
            rb = arb + lo if is_larger else arb - hi
            re = (arb + hi if is_larger else arb - lo) + l_ms
        else:
            rb = (arb + lo if is_larger else arb - hi) - l_ms
            re = arb + hi if is_larger else arb - lo
        rb0, re0 = rb, re
        rb, re = max(rb, 0), min(re, L2)
        if rb >= re:
            return rb, re, False, True
        mid = (rb + re) >> 1
        rev = mid >= self.l_pac
        pf = L2 - 1 - mid if rev else mid
        rid = int(np.searchsorted(self.ann_off, pf, side="right") - 1)
        fb, fe = int(self.ann_off[rid]), int(self.ann_off[rid] + self.ann_len[rid])
        if rev:
            fb, fe = L2 - fe, L2 - fb
        rb, re = max(rb, fb), min(re, fe)
        return rb, re, arid == rid and re - rb >= self.o.min_seed_len, (rb, re) != (rb0, re0)

    def walk(self, pes, a1, ms, ma, ma_input, ev):
        """mem_matesw (bwamem_pair.c:114-183) on a copy of ma -> (n, new ma, its peak length)"""
        o = self.o
        arb, arid, l_ms = int(a1["rb"]), int(a1["rid"]), len(ms)
        s = self.skip(pes, arb, ma)
        s_in = self.skip(pes, arb, ma_input)
        need_cur = [r for r in range(4) if sum(s) < 4 and not s[r]]
        need_in = [r for r in range(4) if sum(s_in) < 4 and not s_in[r]]
        peak = len(ma)
        if sum(s) == 4:
            ev["spec_ignored"] += sum(self.window(pes, arb, arid, l_ms, r)[2] for r in need_in)
            return 0, ma, peak
        n = n_sw_orient = 0
        ma = ma.copy()
        rc = np.ascontiguousarray(np.where(ms < 4, 3 - ms, 4)[::-1].astype(np.uint8))
        for r in range(4):
            if s[r]:
                if r in need_in and self.window(pes, arb, arid, l_ms, r)[2]:
                    ev["spec_ignored"] += 1
                continue
            is_rev = (r >> 1) != (r & 1)
            rb, re, ok, changed = self.window(pes, arb, arid, l_ms, r)
            ev["windows_changed"] += changed and rb < re
            ev["windows_rejected"] += not ok
            if ok:
                ev["needed_not_speculated"] += r not in need_in
                q = rc if is_rev else np.ascontiguousarray(ms, np.uint8)
                t = np.ascontiguousarray(self.both[rb:re])
                xtra = XSUBO | XSTART | (XBYTE if l_ms * o.a < 250 else 0) | (o.min_seed_len * o.a)
                mat = (C.c_int8 * 25)(*o.mat)
                k = self.lib.ksw_align2(l_ms, q.ctypes.data, re - rb, t.ctypes.data, 5, C.cast(mat, C.c_void_p), o.o_del,
                                        o.e_del, o.o_ins, o.e_ins, xtra, None)
                n_sw_orient += 1
                if k.score >= o.min_seed_len and k.qb >= 0:
                    b = np.zeros(1, abi.ALNREG_DTYPE)
                    b["rid"] = arid
                    b["n_comp_is_alt"] = a1["n_comp_is_alt"] & np.uint32(0xc0000000)
                    b["qb"] = l_ms - (k.qe + 1) if is_rev else k.qb
                    b["qe"] = l_ms - k.qb if is_rev else k.qe + 1
                    L2 = self.l_pac << 1
                    b["rb"] = L2 - (rb + k.te + 1) if is_rev else rb + k.tb
                    b["re"] = L2 - (rb + k.tb) if is_rev else rb + k.te + 1
                    b["score"], b["csub"], b["secondary"] = k.score, k.score2, -1
                    b["seedcov"] = min(int(b["re"][0] - b["rb"][0]), int(b["qe"][0] - b["qb"][0])) >> 1
                    at = len(ma)
                    for i in range(len(ma)):
                        if ma["score"][i] < k.score:
                            at = i
                            break
                    ev["regs_added_to_empty"] += len(ma) == 0
                    ma = np.concatenate([ma[:at], b, ma[at:]])
                    peak = max(peak, len(ma))
                    ev["regs_added"] += 1
                    ev["regs_added_rev"] += int(b["rb"][0]) >= self.l_pac
                    ev["_pushed"] += 1
                else:
                    ev["sw_no_region"] += 1
                n += 1
            if n and len(ma) > 1:
                before = len(ma)
                ma = np.ascontiguousarray(ma)
                m = self.lib.mem_sort_dedup_patch(C.byref(o), None, None, None, len(ma), ma.ctypes.data)
                ma = ma[:m].copy()
                ev["dedup_removed"] += m < before
        ev["_orient"] = max(ev["_orient"], n_sw_orient)
        return n, ma, peak


def rescue_pairs(name, rp, pairopt, pes, seq_off, seq, regs_by_read, per_pair=None):
    """the rescue loop of mem_sam_pe over every pair, with the observing walk beside it ->
    (regions per read, out_n, n_sw, peak_n, coverage counts); per_pair, if a list, gets every pair's events"""
    nr = len(regs_by_read)
    assert nr % 2 == 0
    cov = dict.fromkeys(COVERAGE_KEYS, 0)
    out, out_n, n_sw, peak_n = [], [], [], []
    for p in range(nr // 2):
        a_in = [regs_by_read[2 * p], regs_by_read[2 * p + 1]]
        ms = [seq[seq_off[2 * p + 1]:seq_off[2 * p + 2]], seq[seq_off[2 * p]:seq_off[2 * p + 1]]]  # the mate of read i
        v = [rp.to_v(a_in[0]), rp.to_v(a_in[1])]
        cur = [a_in[0].copy(), a_in[1].copy()]
        peak = [len(a_in[0]), len(a_in[1])]
        ev = dict.fromkeys(COVERAGE_KEYS, 0)
        ev["_pushed"] = ev["_orient"] = 0
        b = [a[a["score"] >= a["score"][0] - pairopt["pen_unpaired"]] if len(a) else a for a in a_in]
        total = 0
        any_sw = False
        for i in range(2):  # bwamem_pair.c:275-277
            cov["calls_cut"] += max(len(b[i]) - pairopt["max_matesw"], 0)
            for j in range(min(len(b[i]), pairopt["max_matesw"])):
                got = rp.matesw(pes, b[i][j:j + 1], ms[i], v[1 - i])
                want, cur[1 - i], pk = rp.walk(pes, b[i][j], ms[i], cur[1 - i], a_in[1 - i], ev)
                peak[1 - i] = max(peak[1 - i], pk)
                assert got == want, f"{name} pair {p}: the walk made {want} SW calls, mem_matesw {got}"
                bad = G.region_mismatch(cur[1 - i], rp.from_v(v[1 - i]))
                assert bad is None, f"{name} pair {p}: the walk differs from mem_matesw: {bad}"
                total += got
                any_sw |= got > 0
        for i in range(2):
            out.append(rp.from_v(v[i]))
            out_n.append(len(out[-1]))
            libc.free(v[i].a)
            peak_n.append(peak[i])
            cov["reads_over_17"] += out_n[-1] > 17
        n_sw.append(total)
        cov["pairs_sw"] += any_sw
        cov["pairs_multi_cand"] += len(b[0]) >= 2 or len(b[1]) >= 2
        cov["pairs_multi_orient"] += ev["_orient"] >= 2
        for k in ("regs_added", "regs_added_rev", "regs_added_to_empty", "sw_no_region", "dedup_removed",
                  "windows_changed", "windows_rejected", "spec_ignored", "needed_not_speculated"):
            cov[k] += int(ev[k])
        if per_pair is not None:
            per_pair.append(ev)
    return out, out_n, n_sw, peak_n, cov


def run_pairs(name, opt, pairopt, refd, genome_id, alt, seq_off, seq, regs_by_read, out_dir, own_genome=None):
    """the reference over every pair -> the fixture's coverage counts"""
    rp = RefPair(opt, pairopt, refd, alt)
    nr = len(regs_by_read)
    pes = rp.pestat(regs_by_read)
    out, out_n, n_sw, peak_n, cov = rescue_pairs(name, rp, pairopt, pes, seq_off, seq, regs_by_read)
    reg_n = np.array([len(a) for a in regs_by_read], np.int32)
    # The tests give every read an output span of n + HEADROOM regions and expect every pair to
    # finish.  The reference itself grows a few reads by more (reads in repeats with ten and more
    # candidates, each pushing a region into the mate): those pairs are taken out and the set,
    # its statistics included, is made again without them.
    grown = (np.array(peak_n) - reg_n > HEADROOM).reshape(-1, 2).any(axis=1)
    if grown.any():
        print(f"[gen_rescue] rescue_{name}: pairs {np.nonzero(grown)[0].tolist()} grow a read by more than "
              f"{HEADROOM} regions (up to {int((np.array(peak_n) - reg_n).max())}): left out", flush=True)
        reads = np.nonzero(np.repeat(~grown, 2))[0]
        so, sq = pack([seq[seq_off[r]:seq_off[r + 1]] for r in reads])
        return run_pairs(name, opt, pairopt, refd, genome_id, alt, so, sq, [regs_by_read[r] for r in reads], out_dir,
                         own_genome)
    cat = lambda v: np.concatenate(v) if len(v) else np.zeros(0, abi.ALNREG_DTYPE)  # noqa: E731
    extra = {}
    if own_genome is not None:
        extra = dict(g_l_pac=np.array([refd["l_pac"]], np.int64), g_ann_offset=np.asarray(refd["ann_offset"], np.int64),
                     g_ann_len=np.asarray(refd["ann_len"], np.int32), g_pac=np.asarray(refd["pac"], np.uint8))
    path = os.path.join(out_dir, f"rescue_{name}.npz")
    np.savez_compressed(
        path, **extra, opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32), opt_mat=np.asarray(opt["mat"], np.int8),
        pairopt_int=np.array([pairopt[k] for k in PAIROPT_KEYS], np.int32),
        pairopt_mask=np.array([pairopt["mask_level_redun"], pairopt["mask_level"]], np.float32),
        genome=np.array([genome_id], np.int32), alt=np.asarray(alt, np.uint8), seq_off=np.asarray(seq_off, np.int64),
        seq=np.asarray(seq, np.uint8), reg_n=reg_n, regs=cat(regs_by_read), pes=pes,
        out_n=np.array(out_n, np.int32), out_regs=cat(out), n_sw=np.array(n_sw, np.int32),
        peak_n=np.array(peak_n, np.int32), coverage=np.array([int(cov[k]) for k in COVERAGE_KEYS], np.int64))
    size = os.path.getsize(path)
    print(f"[gen_rescue] rescue_{name}: {nr // 2} pairs, {int(reg_n.sum())} -> {sum(out_n)} regions, pes "
          f"{[(int(x['low']), int(x['high']), int(x['failed'])) for x in pes]}, {size} bytes, "
          f"{ {k: int(v) for k, v in cov.items()} }", flush=True)
    if size > MAX_BYTES:
        raise SystemExit(f"rescue_{name}.npz is {size} bytes (> {MAX_BYTES})")
    return cov


# ---------------------------------------------------------------- simulated libraries
def revcomp(x):
    return (3 - x[::-1]).astype(np.uint8)


def mutate(rng, x, rate):
    x = x.copy()
    sub = rng.random(len(x)) < rate
    x[sub] = (x[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
    return x


def damage(rng, x, kind):
    """mate kinds: 0 clean, 1 unseedable (a substitution every 15th base), 2 second half junk,
    3 random, 4 first 45-70 bases junk"""
    if kind == 1:
        x = x.copy()
        idx = np.arange(int(rng.integers(0, 15)), len(x), 15)
        x[idx] = (x[idx] + rng.integers(1, 4, len(idx))) & 3
    elif kind == 2:
        x = damage(rng, x, 1)
        h = len(x) // 2
        x[h:] = rng.integers(0, 4, len(x) - h)
    elif kind == 3:
        x = rng.integers(0, 4, len(x)).astype(np.uint8)
    elif kind == 4:
        x = x.copy()
        h = int(rng.integers(45, 71))
        x[:h] = rng.integers(0, 4, h)
    return x.astype(np.uint8)


def sim_pair(rng, g, start, isize, L, orient, kind, err=0.01):
    """one pair from fragment g[start:start+isize]: FR reads face each other, RF reads face outwards"""
    frag = g[start:start + isize]
    left, right = frag[:L], frag[isize - L:]
    if orient == "FR":
        r1, r2 = left, revcomp(right)
    else:  # RF
        r1, r2 = revcomp(left), right
    r1, r2 = mutate(rng, r1, err), damage(rng, mutate(rng, r2, err), kind)
    if rng.random() < 0.5:  # either end may be the damaged one / come first
        r1, r2 = r2, r1
    return [r1.astype(np.uint8), r2]


def pack(seqs):
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return seq_off, np.concatenate(seqs).astype(np.uint8)


def regions_of(prefix, opt, popt, refd, alt, seq_off, seq):
    """seed, chain, extend and post-process (flags 1|2) every read with the reference"""
    oref = oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])
    rco, rid, fr, cso, sd = oracle.ref_seqs2chains(prefix, seq_off, seq)
    b = Batch(seq_off, seq, rco, cso, rid, fr, sd)
    regs, n, _ = oracle.chain2aln("ref", opt, oref, b)
    regs = compact(b, regs, n)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    post = RefPost(opt, popt, refd, alt)
    return [post.run(seq[seq_off[r]:seq_off[r + 1]], regs[off[r]:off[r + 1]], r, False) for r in range(len(n))]


def lib_reads(rng, refd, n_pairs, mean, sd, orient_of, kind_of, L=150, where=None):
    g = genome_bases(refd).astype(np.uint8)
    seqs = []
    for k in range(n_pairs):
        isize = max(int(rng.normal(mean, sd)), L + 10)
        if where is None:
            c = int(rng.integers(0, len(refd["ann_len"])))
            start = int(refd["ann_offset"][c]) + int(rng.integers(0, int(refd["ann_len"][c]) - isize))
        else:
            start = where(k, isize)
        seqs += sim_pair(rng, g, start, isize, L, orient_of(k), kind_of(k))
    return pack(seqs)


def rep_genome(rng):
    """120 kbp in two contigs with tandem duplications: 40 families of 4 x 300 bp (1 % divergence
    between copies) and 3 families of 24 x 200 bp (3 %)"""
    parts = []
    for f in range(43):
        parts.append(rng.integers(0, 4, int(rng.integers(1500, 2500))).astype(np.uint8))
        unit, copies, div = (300, 4, 0.01) if f < 40 else (200, 24, 0.03)
        u = rng.integers(0, 4, unit).astype(np.uint8)
        parts += [mutate(rng, u, div) for _ in range(copies)]
    parts.append(rng.integers(0, 4, 2000).astype(np.uint8))
    g = np.concatenate(parts)
    # (first base, unit, copies) of every family
    fam, pos, i = [], 0, 0
    for f in range(43):
        pos += len(parts[i])
        i += 1
        copies, unit = (4, 300) if f < 40 else (24, 200)
        fam.append((pos, unit, copies))
        pos += unit * copies
        i += copies
    half = len(g) // 2
    l_pac = len(g)
    pac = np.zeros(l_pac // 4 + 1, np.uint8)
    x = np.arange(l_pac)
    np.bitwise_or.at(pac, x >> 2, (g << ((~x & 3) << 1)).astype(np.uint8))
    refd = dict(l_pac=l_pac, ann_offset=np.array([0, half], np.int64), ann_len=np.array([half, l_pac - half], np.int32),
                pac=pac)
    return refd, fam


def make_cases(out_dir):
    """rescue_pestat_cases.npz: hand-built region sets with the reference's pes"""
    refd = G.load_ref()
    l_pac = int(refd["l_pac"])
    opt = abi.default_opt()
    po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
              mask_level_redun=0.95, mask_level=0.50)
    rp = RefPair(opt, po, refd, np.zeros(3, np.uint8))
    rng = np.random.default_rng(7)

    def reg(rb, rev=False, rid=0, score=150, qb=0, qe=150):
        a = np.zeros(1, abi.ALNREG_DTYPE)
        a["rb"] = (l_pac << 1) - 1 - rb if rev else rb
        a["re"] = a["rb"] + 150
        a["qb"], a["qe"], a["rid"], a["score"], a["truesc"], a["secondary"] = qb, qe, rid, score, score, -1
        return a

    def fr(pos, isz, **kw):  # read 1 forward at pos, read 2 reverse: an FR pair of insert size ~isz
        return [reg(pos), reg(pos + isz, rev=True, **kw)]

    def rf(pos, isz):  # the reverse read first on the genome: the reads face outwards
        return [reg(pos + isz), reg(pos, rev=True)]

    def pairs(k, mean=400, sd=30, f=fr):
        out = []
        for _ in range(k):
            out += f(int(rng.integers(1000, 400000)), max(int(rng.normal(mean, sd)), 1))
        return out

    cases = {}
    cases["all_under_min_cnt"] = pairs(9) + pairs(3, f=rf)
    cases["exactly_10"] = pairs(10)
    cases["failed_by_ratio"] = pairs(220) + pairs(10, 2000, 100, rf)
    cases["two_alive"] = pairs(120) + pairs(40, 2000, 100, rf)
    cases["is_zero"] = pairs(12) + [x for _ in range(5) for x in (reg(5000), reg(5000))]
    cases["over_max_ins"] = pairs(12) + fr(7000, 10001) + fr(9000, 10000) + fr(9000, 20000)
    cases["low_clamped"] = [x for k in range(40) for x in fr(3000 + 997 * k, 3 + 23 * k)]
    sub = []
    for k in range(6):  # a second hit over 80 % of the best one's score that overlaps it: cal_sub fails the pair
        a, b = fr(20000 + 1000 * k, 300 + k)
        sub += [np.concatenate([a, reg(700000 + k, score=140, qb=10, qe=150)]), b]
    for k in range(3):  # ... and one that does not overlap enough: the pair counts
        a, b = fr(30000 + 1000 * k, 350 + k)
        sub += [np.concatenate([a, reg(710000 + k, score=140, qb=100, qe=150)]), b]
    cases["cal_sub"] = pairs(12) + sub
    cases["other_contig"] = pairs(12) + [x for k in range(6) for x in fr(40000 + k, 400, rid=1)]
    cases["odd_n_reads"] = pairs(21) + [reg(1234)]
    cases["n_reads_0"] = []
    cases["no_regions"] = pairs(11) + [np.zeros(0, abi.ALNREG_DTYPE), reg(99)] + [reg(77), np.zeros(0, abi.ALNREG_DTYPE)]
    arrays = dict(names=np.array(list(cases)), opt_int=np.array([opt[k] for k in G.OPT_KEYS], np.int32),
                  opt_mat=np.asarray(opt["mat"], np.int8), pairopt_int=np.array([po[k] for k in PAIROPT_KEYS], np.int32),
                  pairopt_mask=np.array([po["mask_level_redun"], po["mask_level"]], np.float32))
    for name, reads in cases.items():
        pes = rp.pestat(reads)
        arrays[name + "_n"] = np.array([len(a) for a in reads], np.int32)
        arrays[name + "_regs"] = np.concatenate(reads) if reads else np.zeros(0, abi.ALNREG_DTYPE)
        arrays[name + "_pes"] = pes
        print(f"[gen_rescue] case {name}: {len(reads)} reads, pes "
              f"{[(int(x['low']), int(x['high']), int(x['failed'])) for x in pes]}")
    np.savez_compressed(os.path.join(out_dir, "rescue_pestat_cases.npz"), **arrays)


def main():
    out_dir = GOLD
    refd = G.load_ref()
    opt = abi.default_opt()
    po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
              mask_level_redun=0.95, mask_level=0.50)
    popt = (po["max_chain_gap"], po["mask_level_redun"], po["mask_level"])
    total = dict.fromkeys(COVERAGE_KEYS, 0)

    def add(cov):
        for k in COVERAGE_KEYS:
            total[k] += int(cov[k])

    make_cases(out_dir)
    no_alt = np.zeros(len(refd["ann_len"]), np.uint8)
    with tempfile.TemporaryDirectory() as d:
        prefix = build_index(refd, d)
        rng = np.random.default_rng(20240701)
        kinds = [0, 0, 0, 1, 1, 2, 3, 0]
        so, sq = lib_reads(rng, refd, 1600, 400, 50, lambda k: "FR", lambda k: kinds[k % 8])
        add(run_pairs("fr", opt, po, refd, 0, no_alt, so, sq, regions_of(prefix, opt, popt, refd, no_alt, so, sq), out_dir))

        rng = np.random.default_rng(20240702)
        so, sq = lib_reads(rng, refd, 1400, 450, 60, lambda k: "FR" if k % 2 else "RF", lambda k: kinds[(k // 2) % 8])
        add(run_pairs("mixed", opt, po, refd, 0, no_alt, so, sq, regions_of(prefix, opt, popt, refd, no_alt, so, sq),
                      out_dir))

        rng = np.random.default_rng(20240703)
        so, sq = lib_reads(rng, refd, 1200, 350, 8, lambda k: "FR", lambda k: 4 if k % 4 == 0 else 0)
        add(run_pairs("shift", opt, po, refd, 0, no_alt, so, sq, regions_of(prefix, opt, popt, refd, no_alt, so, sq),
                      out_dir))

        rng = np.random.default_rng(20240704)
        alt = no_alt.copy()
        alt[1] = 1
        ao, al = refd["ann_offset"], refd["ann_len"]

        def at_ends(k, isize):  # fragments flush with (or close to) a contig's first / last base
            c = k % len(al)
            slack = int(rng.integers(0, 120)) if k % 3 else 0
            return int(ao[c]) + slack if (k // len(al)) % 2 else int(ao[c]) + int(al[c]) - isize - slack
        n_end = 700
        so, sq = lib_reads(rng, refd, 1200, 400, 50, lambda k: "FR", lambda k: [1, 3, 2, 0][k % 4] if k < n_end else kinds[k % 8],
                           where=lambda k, isize: at_ends(k, isize) if k < n_end else int(rng.integers(0, int(ao[2]) + int(al[2]) - isize)))
        add(run_pairs("ends", opt, po, refd, 0, alt, so, sq, regions_of(prefix, opt, popt, refd, alt, so, sq), out_dir))

    # rep: the set's own genome with tandem duplications
    rng = np.random.default_rng(20240705)
    gref, fam = rep_genome(rng)
    no_alt2 = np.zeros(2, np.uint8)
    with tempfile.TemporaryDirectory() as d:
        g = genome_bases(gref).astype(np.uint8)
        fa = os.path.join(d, "ref.fa")
        with open(fa, "w") as f:
            for i, (o, ln) in enumerate(zip(gref["ann_offset"], gref["ann_len"])):
                f.write(f">c{i}\n" + "".join(np.array(list("ACGT"))[g[int(o):int(o) + int(ln)]].tolist()) + "\n")
        lib = oracle.ref_lib()
        lib.bwa_idx_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        lib.bwa_idx_build.restype = C.c_int
        lib.bwa_idx_build(fa.encode(), fa.encode(), 0, 10000000)
        half = int(gref["ann_offset"][1])
        seqs = []
        for k in range(900):
            isize = max(int(rng.normal(500, 40)), 330)
            kind = [1, 1, 2, 3, 0][k % 5]
            if k % 3 == 0:  # anywhere: the unique pairs that give the library its statistics
                start = int(rng.integers(0, len(g) - isize))
                inside = [False, False]
                kind = [0, 0, 1][(k // 3) % 3]
            else:
                pos, unit, copies = fam[k % len(fam)]
                if copies == 24 and k % 2:  # both reads inside the long family: many regions each
                    start = pos + int(rng.integers(0, unit * copies - isize))
                elif k % 2:  # read 1 inside a copy, its mate past the family
                    start = pos + unit * int(rng.integers(0, copies)) + int(rng.integers(0, unit - 150))
                else:  # read 2 inside a copy, its mate before the family
                    start = pos + unit * int(rng.integers(0, copies)) + int(rng.integers(150, unit)) - isize
                inside = [pos <= start + x < pos + unit * copies for x in (0, isize - 150)]
            if start < 0 or start + isize > len(g) or (start < half) != (start + isize <= half):
                start, inside = 10, [False, False]
            frag = g[start:start + isize]
            r1, r2 = mutate(rng, frag[:150], 0.003), revcomp(mutate(rng, frag[isize - 150:], 0.003))
            if inside[1] and not inside[0]:  # damage the read outside the family
                r1 = damage(rng, r1, kind)
            elif inside[0] or k % 2:
                r2 = damage(rng, r2, kind)
            seqs += [r1.astype(np.uint8), r2.astype(np.uint8)]
        so, sq = pack(seqs)
        regs = regions_of(fa, opt, popt, gref, no_alt2, so, sq)
    add(run_pairs("rep", opt, po, gref, 2, no_alt2, so, sq, regs, out_dir, own_genome=True))
    po2 = dict(po, max_matesw=2)
    keep = np.arange(0, 900, 2)  # every other pair: the file stays small
    reads = np.stack([2 * keep, 2 * keep + 1], axis=1).reshape(-1)
    so2, sq2 = pack([sq[so[r]:so[r + 1]] for r in reads])
    add(run_pairs("rep_sw2", opt, po2, gref, 2, no_alt2, so2, sq2, [regs[r] for r in reads], out_dir, own_genome=True))

    print("[gen_rescue] coverage over all sets:", total)
    short = {k: (total[k], FLOORS[k]) for k in FLOORS if total[k] < FLOORS[k]}
    if short:
        raise SystemExit(f"coverage floors not met (have, need): {short}")


if __name__ == "__main__":
    main()
