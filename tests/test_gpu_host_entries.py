"""The blocking host-buffer entries of the stages after mem_chain2aln (bwagpu_regs_post,
bwagpu_pestat, bwagpu_mate_rescue, bwagpu_mark_primary, bwagpu_pair_select) share one
staging scaffold and one set of device buffers on the context: a call must see nothing of
the call before it, whatever the order and the sizes, and last_stats() must count exactly
the caller's arrays that were moved.  All sets here lie on genome 0 with one option set,
so one context serves them all."""
import numpy as np
import pytest

import golden_io as G
import pair_io as P
import post_io as PO
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import Engine

pytestmark = pytest.mark.gpu

REG = abi.ALNREG_DTYPE.itemsize


@pytest.fixture(scope="module")
def sets():
    post, resc, pair, cases = PO.load("c5_mixed"), R.load("ends"), P.load("ends"), P.load_cases()
    _, pestat_po, pestat_cases = R.load_cases()
    opts = [post.opt, resc.opt, pair.opt, cases["n0_n0"].opt, R.load_cases()[0]]
    assert post.genome == 0 and resc.genome_id == 0 and pair.genome_id == 0 and cases["n0_n0"].genome_id == 0
    for o in opts[1:]:
        assert all(int(o[k]) == int(opts[0][k]) for k in G.OPT_KEYS) and np.array_equal(o["mat"], opts[0]["mat"])
    return post, resc, pair, cases, pestat_po, pestat_cases


@pytest.fixture(scope="module")
def eng(sets):
    g = G.load_ref()
    e = Engine(0, sets[0].opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e.set_regs_post(0)
    yield e
    e.close()


def span_of(off, n):
    """regions of regs[lo, hi), the part of the array that holds every non-empty span"""
    used = np.asarray(n) > 0
    if not used.any():
        return 0
    off, n = np.asarray(off, np.int64)[used], np.asarray(n, np.int64)[used]
    return int((off + n).max() - off.min())


def run_rescue(eng, s):
    eng.set_alt(s.alt)
    out_off = s.out_off(8)
    return out_off, eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt())


def check_rescue(s, out_off, got):
    out, out_n, status, n_sw = got
    assert (status == 0).all() and np.array_equal(out_n, s.out_n) and np.array_equal(n_sw, s.n_sw)
    want = G.dense(s.out_regs, G.offsets(s.out_n), s.out_n)
    bad = G.region_mismatch(G.dense(out, out_off[:-1], out_n), want)
    assert bad is None, f"mate_rescue: {bad}"


def check_mark(eng, d, what):
    got, n_pri, status = eng.mark_primary(d.off, d.regs, d.n, 2 * d.pair_id0, d.selopt())
    assert (status == abi.SEL_DONE).all(), what
    assert np.array_equal(n_pri, d.n_pri), what
    assert got.tobytes() == d.marked.tobytes(), what


def check_post(eng, s):
    eng.set_alt(s.alt)
    regs, n = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, 3, s.id0, s.popt)
    want_regs, want_n = s.want[3]
    assert np.array_equal(n, want_n)
    bad = G.region_mismatch(G.dense(regs, s.off, n), want_regs)
    assert bad is None, f"regs_post: {bad}"


def check_select(d, got, what):
    sel, om, regs = got
    assert sel.tobytes() == d.sel[0].tobytes(), f"{what}: sel"
    assert np.array_equal(om, d.out_mapq[0]), f"{what}: out_mapq"
    assert regs.tobytes() == d.final.tobytes(), f"{what}: regions"


def test_shared_staging_carries_nothing_over(eng, sets):
    post, resc, pair, cases, pestat_po, pestat_cases = sets
    check_rescue(resc, *run_rescue(eng, resc))
    for c in ("n0_n0", "n17"):  # no region at all; one read past the insertion-sort threshold
        check_mark(eng, cases[c], c)
    check_post(eng, post)
    for c in ("odd_n_reads", "no_regions"):
        n, regs, want = pestat_cases[c]
        got = eng.pestat(G.offsets(n), regs, n, pestat_po)
        assert got.tobytes() == want.tobytes(), f"pestat {c}: got {got} want {want}"
    check_select(pair, eng.pair_select(pair.pes, pair.off, pair.marked, pair.n, pair.n_pri, pair.pair_id0, pair.selopt()),
                 "pair_select(ends)")
    check_mark(eng, cases["n0_n0"], "n0_n0 again")
    # in_status = None directly after a call that passed one: no word of the earlier call is read
    skip = np.zeros(pair.n_reads // 2, np.int32)
    skip[::7] = abi.RESCUE_OVERFLOW
    sel, _, _ = eng.pair_select(pair.pes, pair.off, pair.marked, pair.n, pair.n_pri, pair.pair_id0, pair.selopt(), skip)
    assert (sel["status"][::7] == abi.SEL_SKIPPED).all()
    check_select(pair, eng.pair_select(pair.pes, pair.off, pair.marked, pair.n, pair.n_pri, pair.pair_id0, pair.selopt()),
                 "pair_select(ends) without in_status")


def test_stats_count_the_callers_arrays(eng, sets):
    """h2d_bytes / d2h_bytes in closed form (bwagpu.h); nr reads, np pairs, S = hi - lo regions
    copied, O the output spans, B bases"""
    post, resc, pair = sets[0], sets[1], sets[2]

    def stats(h2d, d2h):
        st = eng.last_stats()
        print(f"last_stats: {st}; want h2d {h2d} d2h {d2h}")
        assert st["kernel_ms"] > 0
        assert (st["h2d_bytes"], st["d2h_bytes"]) == (h2d, d2h)

    nr, S = len(post.n), span_of(post.off, post.n)
    B = int(post.seq_off[-1] - post.seq_off[0])
    check_post(eng, post)
    stats(REG * S + B + 8 * (2 * nr + 1) + 4 * nr, REG * S + 4 * nr)

    nr, np_, S = resc.n_reads, resc.n_reads // 2, span_of(resc.off, resc.n)
    B = int(resc.seq_off[-1] - resc.seq_off[0])
    out_off, got = run_rescue(eng, resc)
    check_rescue(resc, out_off, got)
    stats(REG * S + B + 8 * (3 * nr + 2) + 4 * nr, REG * int(out_off[-1] - out_off[0]) + 4 * (nr + 2 * np_))

    nr, np_, S = pair.n_reads, pair.n_reads // 2, span_of(pair.off, pair.n)
    check_mark(eng, pair, "pair_ends")
    stats(REG * S + 12 * nr, REG * S + 8 * nr)

    in_status = np.zeros(np_, np.int32)
    check_select(pair, eng.pair_select(pair.pes, pair.off, pair.marked, pair.n, pair.n_pri, pair.pair_id0, pair.selopt(),
                                       in_status), "pair_select(ends) with in_status")
    stats((REG + 4) * S + 8 * nr + 4 * (2 * nr + np_), (REG + 4) * S + abi.PAIRSEL_DTYPE.itemsize * np_)
    # without in_status its np words are not moved and not counted
    eng.pair_select(pair.pes, pair.off, pair.marked, pair.n, pair.n_pri, pair.pair_id0, pair.selopt())
    stats((REG + 4) * S + 8 * nr + 4 * 2 * nr, (REG + 4) * S + abi.PAIRSEL_DTYPE.itemsize * np_)


def test_regs_post_spans_with_gaps_and_a_front_offset(eng, sets):
    s = sets[0]
    n, nr = s.n, len(s.n)
    off = (np.cumsum(n.astype(np.int64) + 3) - n - 3 + 5).astype(np.int64)  # 3 records between spans, 5 in front
    regs = np.zeros(int(off[-1] + n[-1]) + 2, abi.ALNREG_DTYPE)
    regs["score"] = -12345
    used = np.zeros(len(regs), bool)
    for r in range(nr):
        regs[off[r]:off[r] + n[r]] = s.regs[s.off[r]:s.off[r] + n[r]]
        used[off[r]:off[r] + n[r]] = True
    eng.set_alt(s.alt)
    got, got_n = eng.regs_post(s.seq_off, s.seq, off, regs, n, 3, s.id0, s.popt)
    want_regs, want_n = s.want[3]
    assert np.array_equal(got_n, want_n)
    bad = G.region_mismatch(G.dense(got, off, got_n), want_regs)
    assert bad is None, bad
    assert (~used[:5]).all() and (~used[off[0] + n[0]:off[0] + n[0] + 3]).all()
    assert got[~used].tobytes() == regs[~used].tobytes()
    st = eng.last_stats()
    S = span_of(off, n)  # the gaps between the first and the last span travel with them
    assert S > int(n.sum())
    assert st["h2d_bytes"] == REG * S + int(s.seq_off[-1] - s.seq_off[0]) + 8 * (2 * nr + 1) + 4 * nr
