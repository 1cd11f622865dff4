"""CPU: the job families at the CIGAR kernel's band, segment and run-length
boundaries (tests/cigar_cases.py) are what they claim to be.

* the instrumented oracle entry (oracle_reg2aln_batch_extremes, which shares
  ksw_global.c's loops) returns exactly what oracle_reg2aln_batch returns, on
  every family and on the four cigar_* golden sets;
* the committed golden file (tests/golden/cigar_edges.npz: the same families
  through the reference's mem_reg2aln) holds these families' inputs, and the
  oracle reproduces its records, CIGARs and MDs at every capacity; where
  oracle/_ref is built, the compiled reference does too;
* reach: every claim a family makes per job (columns, band and frame of the
  last call, calls and their w2, run lengths, first and last op, CIGAR, MD
  numbers) holds in the extremes; together the families land in all six CD
  buckets and all three matrix classes; each `ties` family tells the
  reference's m >= e from m > e on a stated number of jobs;
* conditions: no job of any family reads the direction matrix outside a row's
  band or a cell no row wrote; every intermediate of the `limits` families
  lies strictly inside int32.
"""
import os

import numpy as np
import pytest

import cigar_cases as CC
import golden_io as G
import oracle
from bwagpu import abi
from cigar_helpers import zb_class

FAMS = CC.families()
NAMES = list(CC.FAMILY_NAMES)
X = oracle.R2X
REQUIRED = ("band_form", "segments", "runs", "squeeze_clip", "md_edges", "capacity", "band_loop")
COMPARED = ("pos", "rid", "is_rev", "n_cigar", "NM", "md_len", "score", "w", "status")


@pytest.fixture(scope="module")
def R():
    d = G.load_ref()
    return oracle.Ref(d["l_pac"], d["ann_offset"], d["ann_len"], d["pac"])


@pytest.fixture(scope="module")
def extremes(R):
    """per family, once: (records, cigar, md, extremes) at the family's first capacities"""
    return {n: oracle.reg2aln_extremes(f.opt, R, f.tasks, f.qpool, *f.calls[0]) for n, f in FAMS.items()}


def same(tasks, got, want):
    bad = G.aln_mismatch(tasks, *got, *G.aln_expected_from(*want))
    if bad is None and got[0].tobytes() != np.ascontiguousarray(want[0]).tobytes():
        bad = "records differ outside the compared fields"
    return bad


def test_family_shapes():
    """every family of the list is there; 20..150 jobs each, about 2,500 at most in all; both strands of every
    construction; every job inside the entry's limits"""
    assert all(n in FAMS for n in REQUIRED)
    assert sum(n.startswith("ties") for n in FAMS) >= 3 and sum(n.startswith("limits") for n in FAMS) >= 3
    total = 0
    for name, f in FAMS.items():
        n = len(f.tasks)
        total += n
        assert 20 <= n <= 150, (name, n)
        assert len(f.tags) == len(f.expect) == n and len(set(f.tags)) == n and f.reaches
        assert [t[-2:] for t in f.tags] == ["/f", "/r"] * (n // 2), name
        fwd, rev = f.tasks[0::2], f.tasks[1::2]
        assert (fwd["re"] <= CC.L_PAC).all() and (rev["rb"] >= CC.L_PAC).all()
        assert np.array_equal(rev["rb"], 2 * CC.L_PAC - fwd["re"]) and np.array_equal(rev["re"], 2 * CC.L_PAC - fwd["rb"])
        lq = f.tasks["qe"] - f.tasks["qb"]
        assert lq.min() >= 1 and lq.max() <= 1023 and (f.tasks["re"] - f.tasks["rb"]).max() <= 8192
        assert (f.tasks["qoff"] + f.tasks["l_seq"]).max() <= len(f.qpool)
    assert total <= 2500, total


@pytest.mark.parametrize("name", NAMES)
def test_extremes_entry_returns_the_same_outputs(R, extremes, name):
    f = FAMS[name]
    for c, caps in enumerate(f.calls):
        want = oracle.reg2aln("oracle", f.opt, R, f.tasks, f.qpool, *caps)
        got = extremes[name][:3] if c == 0 else oracle.reg2aln_extremes(f.opt, R, f.tasks, f.qpool, *caps)[:3]
        assert same(f.tasks, got, want) is None, caps
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), caps


@pytest.mark.parametrize("name", G.CIGAR_SETS)
def test_extremes_entry_on_the_golden_cigar_sets(R, name):
    opt, tasks, qpool, exp, ops, mds = G.load_cigar_set(name)
    out, cig, md, ext = oracle.reg2aln_extremes(opt, R, tasks, qpool, 64, 512)
    assert G.aln_mismatch(tasks, out, cig, md, exp, ops, mds) is None
    want = oracle.reg2aln("oracle", opt, R, tasks, qpool, 64, 512)
    assert all(np.array_equal(a, b) for a, b in zip((out, cig, md), want))
    assert (ext[:, X["oob"]] == 0).all() and (ext[:, X["unwritten"]] == 0).all()


def test_golden_file_holds_these_families(R):
    path = os.path.join(G.GOLD, "cigar_edges.npz")
    assert os.path.getsize(path) <= 1 << 20
    gold = G.load_cigar_edges()
    assert set(gold) == set(FAMS)
    again = "regenerate with oracle/gen_golden.py --only-cigar-edges"
    for name, f in FAMS.items():
        g = gold[name]
        assert all(int(g["opt"][k]) == int(f.opt[k]) for k in G.OPT_KEYS), f"{name}: {again}"
        assert np.array_equal(g["opt"]["mat"], np.asarray(f.opt["mat"], np.int8)), f"{name}: {again}"
        assert np.array_equal(g["tasks"], f.tasks) and np.array_equal(g["qpool"], f.qpool), f"{name}: {again}"
        assert [tuple(c) for c in g["caps"].tolist()] == [tuple(c) for c in f.calls], f"{name}: {again}"
        for c, caps in enumerate(f.calls):
            exp, ops, mds = g["calls"][c]
            out, cig, md = oracle.reg2aln("oracle", f.opt, R, f.tasks, f.qpool, *caps)
            bad = G.aln_mismatch(f.tasks, out, cig, md, exp, ops, mds, fields=COMPARED)
            assert bad is None, f"{name} call {caps}: oracle vs the reference's recorded results: {bad}"
            assert out.tobytes() == exp.tobytes(), f"{name} call {caps}: a record byte differs"


def test_reference_agrees_on_every_family(R, extremes):
    """the compiled reference, where oracle/_ref is built.  ref_reg2aln_batch (in every build of libbwaref.so)
    gives what mem_aln_t holds: compared on every job's status and NM, and on every ALN_OK job's position,
    strand, CIGAR and MD.  A build that also has ref_reg2aln_batch_calls gives the last bwa_gen_cigar2 call's
    score and band and the number of calls: then whole records are compared, and the calls with the extremes."""
    lib = oracle.ref_lib()
    if lib is None:
        pytest.skip("oracle/_ref not built")
    filled = ("pos", "rid", "is_rev", "n_cigar", "NM", "md_len", "status")
    for name, f in FAMS.items():
        for c, caps in enumerate(f.calls):
            want = oracle.reg2aln("oracle", f.opt, R, f.tasks, f.qpool, *caps)
            exp, cig, md = oracle.reg2aln("ref", f.opt, R, f.tasks, f.qpool, *caps)
            assert np.array_equal(want[0]["status"], exp["status"]) and np.array_equal(want[0]["NM"], exp["NM"]), (name, caps)
            ok = exp["status"] == abi.ALN_OK
            bad = G.aln_mismatch(f.tasks[ok], want[0][ok], want[1][ok], want[2][ok],
                                 *G.aln_expected_from(exp[ok], cig[ok], md[ok]), fields=filled)
            assert bad is None, (name, caps, bad)
            if hasattr(lib, "ref_reg2aln_batch_calls"):
                exp, cig, md, tries = oracle.ref_reg2aln_calls(f.opt, R, f.tasks, f.qpool, *caps)
                assert same(f.tasks, want, (exp, cig, md)) is None, (name, caps)
                if c == 0:   # the oracle's band loop makes the reference's number of bwa_gen_cigar2 calls
                    assert np.array_equal(tries, extremes[name][3][:, X["tries"]]), name


@pytest.mark.parametrize("name", NAMES)
def test_reach(extremes, name):
    """every per-job claim, from the extremes; printed: the family's row of DESIGN.md §9's table"""
    f = FAMS[name]
    out, cig, md, ext = extremes[name]
    bad = CC.claim_failures(f, out, cig, md, ext, X)
    assert not bad, f"{len(bad)} claims fail: {bad[:5]}"
    n = ext[:, X["tries"]]
    last = np.maximum(n - 1, 0)
    ncol = ext[np.arange(len(n)), X["ncol"] + last]
    frames = sorted({CC.frame_of(int(ext[k, X["w"] + last[k]]), int(f.tasks["qe"][k] - f.tasks["qb"][k]))
                     for k in range(len(n)) if not ext[k, X["ungapped"]]})
    digits = sorted({len(str(v)) for k in range(len(n)) for v in CC.md_parts(bytes(md[k, :out["md_len"][k]]))[0]})
    print(f"| {name} | {len(n)} | {np.bincount(n, minlength=4)[1:].tolist()} | {int(ncol[ncol > 0].min())}.."
          f"{int(ncol.max())} | {'/'.join(frames)} | M {int(ext[:, X['run_m']].max())} I {int(ext[:, X['run_i']].max())} "
          f"D {int(ext[:, X['run_d']].max())} | {digits} | {int(sum(len(e) for e in f.expect))} |")
    assert all(f.expect) or f.flip_min or name == "capacity"   # a claim per job, or the family's own (below)


def test_reach_family_claims(extremes):
    """what each family is for, over its jobs together"""
    def col(name, key):
        return extremes[name][3][:, X[key]]

    def last(name, key):
        e = extremes[name][3]
        return e[np.arange(len(e)), X[key] + e[:, X["tries"]] - 1]
    # band_form: the six column counts, reached through lq and through w2, in both band frames and past them
    f = FAMS["band_form"]
    for ncol in (61, 63, 65, 125, 127, 129):
        hit = [t for t, n in zip(f.tags, last("band_form", "ncol")) if n == ncol]
        assert any("_w2_" in t for t in hit) and any("_w2_" not in t for t in hit), ncol
    # ... and a path along each band's top and bottom edge column
    w_last, dmin, dmax = last("band_form", "w"), col("band_form", "diag_min"), col("band_form", "diag_max")
    for w in (30, 31, 32, 62, 63, 64):
        assert ((w_last == w) & (dmax == w)).any() and ((w_last == w) & (dmin == -w)).any(), w
    cd1 = [(e["frame"], e["ncol"]) for t, e in zip(f.tags, f.expect) if t.startswith("cd1_")]
    assert ("band1", 40) in cd1 and ("col", 40) in cd1 and ("col", 63) in cd1 and ("band1", 63) in cd1
    assert {e["frame"] for e in f.expect} == {"band1", "band2", "col"}
    # segments: every listed lq in the band frame and in the column frame
    f = FAMS["segments"]
    lq = f.tasks["qe"] - f.tasks["qb"]
    for q in CC.SEG_LQ:
        fr = {e["frame"] for e, x in zip(f.expect, lq) if x == q}
        assert fr == {"band1", "col"}, (q, fr)
    assert int((last("segments", "ncol") * (f.tasks["re"] - f.tasks["rb"])).max()) > 700 * 1024   # the HBM slice
    # runs: one run of exactly n per op, and the two end pushes
    for op in "mid":
        assert set(CC.RUN_LENS) <= set(col("runs", "run_" + op).tolist()), op
    f = FAMS["runs"]
    for n in CC.END_LENS:
        for kind, key, op in (("lead_I", "first", 1), ("trail_I", "last", 1), ("lead_D", "first", 2), ("trail_D", "last", 2)):
            k = f.tags.index(f"{kind}{n}/f")
            assert col("runs", key)[k] == op and col("runs", "run_" + "mid"[op])[k] == n, (kind, n)
    # squeeze_clip: the three shapes under the four clippings; the trailing deletion stays only next to a leading one
    f = FAMS["squeeze_clip"]
    first, lst = col("squeeze_clip", "first"), col("squeeze_clip", "last")
    seen = {((a == 2), (b == 2), int(t["qb"]) > 0, int(t["qe"]) < int(t["l_seq"])) for a, b, t in zip(first, lst, f.tasks)}
    assert len(seen) == 16
    out = extremes["squeeze_clip"][0]
    raw, clips = col("squeeze_clip", "n_raw"), (f.tasks["qb"] > 0).astype(int) + (f.tasks["qe"] < f.tasks["l_seq"])
    assert np.array_equal(out["n_cigar"], raw - ((first == 2) | (lst == 2)) + clips)
    ends = {c[1] for c in CC.CONTIGS}
    assert {int(t["re"]) for t in f.tasks[0::2]} >= ends and {int(t["rb"]) for t in f.tasks[0::2]} >= {c[0] for c in CC.CONTIGS[:2]}
    assert (out["rid"][[int(t["re"]) == CC.L_PAC for t in f.tasks]] == 2).all()
    # md_edges: MD numbers of one to four digits, and the counts on both sides of each digit step
    md = extremes["md_edges"]
    nums = {v for k in range(len(md[0])) for v in CC.md_parts(bytes(md[2][k, :md[0]["md_len"][k]]))[0]}
    assert {9, 10, 99, 100, 999, 1000} <= nums
    assert int(md[0]["NM"].max()) >= 128
    # band_loop: 1, 2 and 3 calls; a loop ended by w2 == wmax on each call number, and by score == last
    n = col("band_loop", "tries")
    assert set(n.tolist()) == {1, 2, 3}
    w2_last = last("band_loop", "w2")
    assert {int(a) for a, b in zip(n, w2_last) if b == 400} == {1, 2, 3}
    assert ((n == 2) & (w2_last < 400)).any() and col("band_loop", "ungapped").sum() >= 4
    # capacity: every victim's status on each side of its capacity is in the golden file (test_golden_file...)
    f = FAMS["capacity"]
    over = [v[2] for v in f.victims if v is not None and v[1]]
    assert len(f.calls) == len(f.victims) and over.count("md") == len(f.tasks) // 2 and over.count("ops") >= 6
    assert any(t["qb"] > 0 or t["qe"] < t["l_seq"] for t in f.tasks) and any(t["qb"] == 0 for t in f.tasks)


def test_capacity_victims(R):
    """each victim overflows exactly past its capacity, and in every call exactly the jobs overflow whose
    n_cigar or md_len (at generous capacities) is past the call's"""
    f = FAMS["capacity"]
    full, _, _ = oracle.reg2aln("oracle", f.opt, R, f.tasks, f.qpool, *f.calls[0])
    assert (full["status"] == abi.ALN_OK).all() and f.victims[0] is None
    for (max_ops, max_md), v in zip(f.calls[1:], f.victims[1:]):
        out, _, _ = oracle.reg2aln("oracle", f.opt, R, f.tasks, f.qpool, max_ops, max_md)
        over = (full["n_cigar"] > max_ops) | (full["md_len"] + 1 > max_md)
        assert np.array_equal(out["status"], np.where(over, abi.ALN_OVERFLOW, abi.ALN_OK)), (max_ops, max_md)
        k, overflows, kind = v
        assert bool(over[k]) == overflows, (max_ops, max_md, f.tags[k])
        assert (max_md == full["md_len"][k] + (not overflows)) if kind == "md" else \
            (max_ops == full["n_cigar"][k] - overflows)


def test_buckets_and_classes():
    """together the families run every CD instantiation in every matrix class it can hold (the shortest reads
    cannot fill the HBM class: 63 columns x 8192 rows is the bound), the HBM slice included"""
    where = set()
    for f in FAMS.values():
        where |= {zb_class(f.opt, CC.L_PAC, t) for t in f.tasks}
    assert {b for b, _ in where} == set(range(6)) and {c for _, c in where} == {0, 1, 2}, sorted(where)
    assert {b for b, c in where if c == 2} >= {2, 3, 4, 5} and {b for b, c in where if c == 1} >= {1, 2, 3, 4, 5}
    print("bins reached:", sorted(where))


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("ties")])
def test_ties_tell_the_orders_apart(R, extremes, name):
    """the reference takes M on m == e; with that one comparison turned around at least flip_min jobs get
    another raw CIGAR, so a kernel with the wrong order cannot pass the family"""
    f = FAMS[name]
    ext = extremes[name][3]
    counts = {}
    for flag, what in ((oracle.FLIP_ME, "m >= e"), (oracle.FLIP_HF, "h >= f"), (oracle.FLIP_E, "ed > te"),
                       (oracle.FLIP_F, "fd > tf")):
        flipped = oracle.reg2aln_extremes(f.opt, R, f.tasks, f.qpool, *f.calls[0], flip=flag)[3]
        counts[what] = int((flipped[:, X["hash"]] != ext[:, X["hash"]]).sum())
    print(f"{name}: raw CIGAR changes on {counts} of {len(f.tasks)} jobs")
    assert f.flip_min >= len(f.tasks) // 4 and counts["m >= e"] >= f.flip_min
    assert counts["h >= f"] > 0 and counts["ed > te"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_conditions(extremes, name):
    """no read of the direction matrix outside a row's band, none of a cell no row wrote; the limits
    families strictly inside int32"""
    ext = extremes[name][3]
    assert (ext[:, X["oob"]] == 0).all() and (ext[:, X["unwritten"]] == 0).all()
    dp = ext[ext[:, X["max_h"]] >= ext[:, X["min_h"]]]          # jobs with at least one DP cell
    lo = dp[:, [X["min_m"], X["min_e"], X["min_f"], X["min_h"]]].min() if len(dp) else 0
    hi = dp[:, [X["max_m"], X["max_e"], X["max_f"], X["max_h"]]].max() if len(dp) else 0
    print(f"{name}: intermediates in [{lo}, {hi}]")
    if name.startswith("limits"):
        assert len(dp) == len(ext)
    assert -(1 << 31) < lo and hi < (1 << 31) - 1
