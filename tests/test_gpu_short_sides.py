"""The phased extension's short phase: task sides with a query of 1 .. Q bases
run sixteen per wave, in groups of eight lanes (extend_quad<8, ...>), after
the longer sides of the same launch (Engine.ext_short(Q); Q = 0: off).

Expected regions come from the CPU oracle (oracle.chain2aln("oracle", ...)) or
the golden vectors, never from the code under test:

* a hand-made batch on the golden genome whose left and right query lengths
  each take every value 0 .. 70 (every column-class edge 7/8 .. 55/56 and the
  threshold edge 63/64), half exact copies and half with substitutions and a
  2-base deletion, at Q = 0, 7 and 63 with the row bound on and off; the
  short-phase counter against the sides counted on the CPU;
* the same batch cut to leave 1, 15, 16 and 17 short calls on a side, no long
  call at all, and no short call at all;
* every golden chain set through Engine.chain2aln at Q = 63, with the
  short-phase counter above 0 on the sets that take the eight-per-wave kernel;
* the hand-made batch under options those sets do not bring to the short
  phase: non-symmetric gap penalties, small bands with a low z-drop, and a
  band the deletions leave (the band retry inside a short call).
"""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import oracle
from bwagpu import abi
from bwagpu.engine import Batch, Engine, compact

pytestmark = pytest.mark.gpu

LQ = 150
QTOP = 70  # the side lengths run 0 .. QTOP


def side_pairs():
    """(left, right) query lengths: each side takes every value 0 .. 70, in
    three pairings so that short and long sides meet in every combination"""
    pairs = []
    for k in range(QTOP + 1):
        pairs += [(k, k), (k, QTOP - k), (k, (37 * k + 5) % (QTOP + 1))]
    return pairs


def mutate_flank(rng, both, x0, n, mutate, with_del):
    """n read bases that align to the 2-strand coordinates from x0 on: an exact
    copy, or one with up to three substitutions and (with_del, n >= 12) two
    reference bases left out"""
    if not mutate or n < 3:
        return both[x0:x0 + n].copy()
    if with_del and n >= 12:
        d = int(rng.integers(4, n - 4))
        fl = np.concatenate([both[x0:x0 + d], both[x0 + d + 2:x0 + n + 2]])
    else:
        fl = both[x0:x0 + n].copy()
    for p in rng.choice(n, size=min(3, max(1, n // 8)), replace=False):
        fl[p] = (fl[p] + 1 + int(rng.integers(0, 3))) & 3
    return fl


@pytest.fixture(scope="module")
def case():
    """-> opt, oracle.Ref, batch (one chain of one seed per 150 bp read), the
    oracle's regions and counts, the reads' (left, right) query lengths"""
    refd = G.load_ref()
    opt = G.load_chain_set("c1_default")[0]
    l_pac = refd["l_pac"]
    pac = refd["pac"]
    x = np.arange(l_pac, dtype=np.int64)
    fwd = ((pac[x >> 2].astype(np.int64) >> ((~x & 3) << 1)) & 3).astype(np.uint8)
    both = np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])  # the 2-strand coordinate space
    rng = np.random.default_rng(20260108)
    seqs, seeds, rids, lens = [], [], [], []
    i = 0
    for mutate in (False, True):
        for ql, qr in side_pairs():
            c = i % len(refd["ann_offset"])
            a0, al = int(refd["ann_offset"][c]), int(refd["ann_len"][c])
            f0 = a0 + 1000 + (7919 * i) % (al - 3000)  # the seed's first base, forward strand
            ln = LQ - ql - qr
            rev = i % 3 == 1
            rbeg = 2 * l_pac - (f0 + ln) if rev else f0  # a reverse-strand seed covers the same forward bases
            left_del = i % 2 == 0
            # the left flank ends at rbeg, so its deletion takes two more bases in front of it
            nl_ref = ql + (2 if mutate and left_del and ql >= 12 else 0)
            left = mutate_flank(rng, both, rbeg - nl_ref, ql, mutate, left_del)
            right = mutate_flank(rng, both, rbeg + ln, qr, mutate, not left_del)
            read = np.concatenate([left, both[rbeg:rbeg + ln], right])
            assert len(read) == LQ
            seqs.append(read)
            seeds.append((rbeg, ql, ln, ln, 0))
            rids.append(c)
            lens.append((ql, qr))
            i += 1
    n = len(seqs)
    batch = Batch(np.arange(n + 1) * LQ, np.concatenate(seqs), np.arange(n + 1), np.arange(n + 1),
                  np.array(rids, np.int32), np.zeros(n, np.float32), np.array(seeds, abi.SEED_DTYPE))
    ref = oracle.Ref(l_pac, refd["ann_offset"], refd["ann_len"], pac)
    oregs, on, ost = oracle.chain2aln("oracle", opt, ref, batch)
    return opt, refd, ref, batch, oregs, on, np.array(lens)


def run_device(eng, batch):
    """one batch through the device entry -> regs, n, sides run in the short phase"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    fields = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev) for k in fields}
    out = torch.zeros(max(batch.n_seeds, 1) * 88, dtype=torch.uint8, device=dev)
    nn = torch.zeros(max(batch.n_reads, 1), dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    c.seq_bytes = int(batch.seq_off[-1])
    for k in fields:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), None, stream.cuda_stream)
    torch.cuda.synchronize()
    short = np.zeros(9, np.int64)
    assert eng.lib.bwagpu_debug_spec_short(eng.ctx, C.c_void_p(stream.cuda_stream),
                                           short.ctypes.data_as(C.c_void_p)) == 0
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], int(short[0])


def short_sides(lens, q):
    """sides with a query of 1 .. q bases"""
    return int(((lens >= 1) & (lens <= q)).sum())


def check(eng, batch, oregs, on, lens, q, what):
    regs, n, short = run_device(eng, batch)
    assert np.array_equal(n, on), f"{what}: {int((n != on).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    assert short == short_sides(lens, q), f"{what}: {short} sides in the short phase, {short_sides(lens, q)} expected"


def make_engine(refd, opt, q):
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    eng.ext_short(q)
    eng.ext_short_fill(0)  # a few hundred sides never fill the grid: every short run takes the short phase
    assert eng.ext_short() == q and eng.ext_short_fill() == 0
    assert eng.ext_kernel(LQ) == eng.EXT_KERNELS[18], "the eight-per-wave phased pair runs this batch"
    return eng


def test_knob_range(case):
    opt, refd = case[0], case[1]
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    eng.ext_short(31)
    assert eng.ext_short(-1) == 31 and eng.ext_short(0) == 31 and eng.ext_short() == 0
    assert eng.ext_short(64) == 0 and eng.ext_short() == 63  # a larger threshold counts as 63
    eng.ext_short_fill(150)
    assert eng.ext_short_fill(-1) == 150 and eng.ext_short_fill(0) == 150 and eng.ext_short_fill() == 0
    eng.close()


@pytest.mark.parametrize("bound", [1, 0])
@pytest.mark.parametrize("q", [0, 7, 63])
def test_boundary_sweep(case, q, bound):
    opt, refd, ref, batch, oregs, on, lens = case
    assert set(lens[:, 0]) == set(range(QTOP + 1)) and set(lens[:, 1]) == set(range(QTOP + 1))
    eng = make_engine(refd, opt, q)
    eng.row_bound(bound)
    check(eng, batch, oregs, on, lens, q, f"Q = {q}, row bound {bound}")
    eng.close()


def test_fill_rule(case):
    """a short run far below the grid's sixteen-per-wave slots runs eight per
    wave (the launch's own rule, Engine.ext_short_fill): same regions, no side
    in the short phase"""
    opt, refd, ref, batch, oregs, on, lens = case
    eng = make_engine(refd, opt, 63)
    eng.ext_short_fill(150)
    check(eng, batch, oregs, on, lens, 0, "Q = 63, fill 150 %")
    eng.close()


def cut(lens, kind, side=0):
    """reads of the batch for a ragged case at Q = 63; an integer `kind` leaves
    that many short calls on `side` (0 left, 1 right) beside every long one"""
    ql, qr = lens[:, 0], lens[:, 1]
    if kind == "no_long":
        return np.flatnonzero((ql <= 63) & (qr <= 63))
    if kind == "no_short":
        return np.flatnonzero(((ql == 0) | (ql > 63)) & ((qr == 0) | (qr > 63)))
    qs = lens[:, side]
    long_s = np.flatnonzero(qs > 63)
    short_s = np.flatnonzero((qs >= 1) & (qs <= 63))
    # every read with a long call on the side, and `kind` reads with a short one, spread over the lengths
    return np.concatenate([long_s, short_s[np.linspace(0, len(short_s) - 1, kind).astype(int)]])


@pytest.mark.parametrize("kind,side", [(1, 0), (15, 0), (16, 0), (17, 0), (1, 1), (15, 1), (16, 1), (17, 1),
                                       ("no_long", 0), ("no_short", 0)])
def test_ragged_tails(case, kind, side):
    opt, refd, ref, batch, oregs, on, lens = case
    reads = cut(lens, kind, side)
    assert len(reads) > 0
    sub = batch.subset(reads)
    sl = lens[reads]
    if isinstance(kind, int):
        assert short_sides(sl[:, side], 63) == kind
    elif kind == "no_long":
        assert (sl <= 63).all() and short_sides(sl, 63) > 0
    else:
        assert short_sides(sl, 63) == 0 and (sl > 63).any()
    sregs, sn, _ = oracle.chain2aln("oracle", opt, ref, sub)
    eng = make_engine(refd, opt, 63)
    check(eng, sub, sregs, sn, sl, 63, f"cut {kind} on side {side}")
    eng.close()


# the golden sets whose options take the eight-per-wave phased kernel, the only
# one with a short phase (opt1_scoring's match score of 2 does not fit its 8-bit
# row-max key: it runs four per wave and only checks that the knob is harmless)
SHORT_SETS = {"c1_default", "c5_mixed", "opt2_band"}


@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_option_sets(case, name):
    refd = case[1]
    opt, batch, want, want_n = G.load_chain_set(name)
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    eng.ext_short(63)
    eng.ext_short_fill(0)
    regs, n = eng.chain2aln(batch)
    assert np.array_equal(n, want_n), f"{int((n != want_n).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), want) is None
    lq_max = int(np.diff(batch.seq_off).max())
    assert (eng.ext_kernel(lq_max) == eng.EXT_KERNELS[18]) == (name in SHORT_SETS)
    # the same batch through the device entry, whose counters can be read: the short phase ran
    dregs, dn, short = run_device(eng, batch)
    assert np.array_equal(dn, want_n) and G.region_mismatch(compact(batch, dregs, dn), want) is None
    assert (short > 0) == (name in SHORT_SETS), f"{short} sides in the short phase"
    eng.close()


# options the golden sets do not bring to the short phase, on the hand-made
# batch (the oracle gives the regions): gap penalties that differ between
# deletions and insertions (extend_quad<8, ., true, false>), and a small band
# with a low z-drop and clipping penalty (the band retry and z-drop inside a
# short call).  The match score stays 1: the eight-per-wave kernel's condition.
VARIANTS = {"asym_gaps": dict(o_del=7, e_del=2, o_ins=5, e_ins=1),
            "asym_gaps2": dict(o_del=4, e_del=1, o_ins=8, e_ins=2),
            "small_band": dict(w=8, zdrop=15, pen_clip5=1, pen_clip3=1),
            "small_band_asym": dict(w=5, zdrop=10, o_del=5, o_ins=7, pen_clip5=2, pen_clip3=0),
            "retry_band": dict(w=2, zdrop=15)}  # the 2-base deletions leave w = 2's band: the second try runs


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_option_variants(case, variant):
    opt0, refd, ref, batch, _, _, lens = case
    opt = dict(opt0, **VARIANTS[variant])
    oregs, on, _ = oracle.chain2aln("oracle", opt, ref, batch)
    eng = make_engine(refd, opt, 63)
    check(eng, batch, oregs, on, lens, 63, variant)
    eng.close()
