"""CPU: the ksw_align2 families at the reference's SIMD width limits
(tests/align2_cases.py) are what they claim to be, and the oracle refuses what
it does not restate.

* the builder reproduces the inputs of tests/golden/align2_range.npz (the
  reference's own ksw_align2 on every family side) byte for byte;
* on every "in" side the gated oracle equals the recorded reference in all
  seven fields; where oracle/_ref is built, the compiled reference reproduces
  the whole file;
* on every "out" side the gated oracle raises, and the tasks the gate still
  admits there (word tasks under a byte gate) are exact;
* the ungated int arithmetic differs from the recorded reference on at least
  one refused task of every "out" side: each gate is needed (the counts are
  printed);
* reach: the saturation, ceiling, BIG and flag-equality tasks land where the
  builder says (Family.expect), read from the reference's records.

word-BIG: with e_ins = 65534 and a = 1 no alignment can pay for an insertion
(131069 for the two planted bases against a score of at most 1023), so the
reach asserted there is that the reference scores exactly the best gapless
diagonal although the insertion is there to take, and that the half after it
ends in the query's last column, where the scan's T + j * e_ins is largest
(align2_cases.WORD_BIG_DERIVATION).
"""
import numpy as np
import pytest

import align2_cases as A
import golden_io as G
import oracle

FLAT = A.flat()
IDS = [f"{n}-{s}" for n, s, _ in FLAT]
GOLD = G.load_align2_range()


def seven(r):
    return r.view(np.int32).reshape(-1, 7)


def differ(a, b):
    return np.nonzero((seven(a) != seven(b)).any(axis=1))[0]


def subset(f, keep):
    """the tasks keep[] of a family as a batch of their own (same pools)"""
    return f.tasks[keep], f.qpool, f.tpool


def test_family_shapes():
    names = {n for n, _, _ in FLAT}
    assert names == {"byte-oe_del", "byte-oe_ins", "byte-e_del", "byte-e_ins", "byte-mixed", "word-oe_del",
                     "word-oe_ins", "word-BIG", "word-ceiling", "byte-sat-shift4", "byte-sat-shift127",
                     "byte-sat-shift128", "byte-sat-shift0", "flags"}
    for name, side, f in FLAT:
        assert 20 <= len(f.tasks) <= 40, (name, side, len(f.tasks))
        ql, tl = f.tasks["qlen"], f.tasks["tlen"]
        if name == "word-BIG":
            assert set(ql.tolist()) == {1000, 1023}
        elif name == "word-ceiling":
            assert ql.max() == (259 if side == "out" else 258)
        elif name == "byte-sat-shift0":
            assert ql.max() == 256
        else:
            assert ql.max() <= 255
        assert ((tl >= ql) & (tl <= ql + 300)).all(), (name, side)
        assert (f.tasks["qoff"] + ql).max() <= len(f.qpool) and (f.tasks["toff"] + tl).max() <= len(f.tpool)
        assert f.side == side and f.gate
        u8 = (f.tasks["xtra"] & A.XB) != 0
        if A.is_in(side):
            assert not f.refused.any() and not f.opt_refused
        else:
            assert f.refused.any() or f.opt_refused
        if name.startswith("byte-") and not name.startswith("byte-sat"):
            assert u8.any() and (~u8).any()          # byte and word tasks under the same options
            assert (f.refused == (u8 & (not A.is_in(side)))).all()   # the word tasks stay admitted
        if name.startswith("word-"):
            assert not u8.any()
    # the values on the two sides of each gate: the last admitted and the first refused
    fam = A.families()
    oe = lambda o: (o["e_del"], o["e_ins"], o["o_del"] + o["e_del"], o["o_ins"] + o["e_ins"])  # noqa: E731
    assert max(oe(fam["byte-oe_del"]["in"].opt)) == 255 and oe(fam["byte-oe_del"]["out"].opt)[2] == 256
    assert max(oe(fam["byte-oe_ins"]["in"].opt)) == 255 and oe(fam["byte-oe_ins"]["out"].opt)[3] == 256
    assert oe(fam["byte-e_del"]["in"].opt)[0] == 254 and oe(fam["byte-e_del"]["out"].opt)[0] == 255
    assert oe(fam["byte-e_del"]["out2"].opt)[0] == 256 and oe(fam["byte-e_del"]["out2"].opt)[2] == 256
    assert oe(fam["byte-e_ins"]["in"].opt)[1] == 254 and oe(fam["byte-e_ins"]["out"].opt)[1] == 255
    assert oe(fam["word-oe_del"]["in"].opt)[2] == 65535 and oe(fam["word-oe_del"]["out"].opt)[2] == 65536
    for s in ("in", "in2"):
        assert oe(fam["word-oe_ins"][s].opt)[3] == 65535
    for s in ("out", "out2"):
        assert oe(fam["word-oe_ins"][s].opt)[3] == 65536
    assert [A.shift_of(fam[f"byte-sat-shift{s}"]["in"].opt) for s in (4, 127, 128, 0)] == [4, 127, 128, 0]


def test_builder_reproduces_the_golden_inputs():
    assert set(GOLD) == {(n, s) for n, s, _ in FLAT}
    for name, side, f in FLAT:
        opt, tasks, _, qp, tp = GOLD[(name, side)]
        assert all(int(opt[k]) == int(f.opt[k]) for k in G.OPT_KEYS), (name, side)
        assert np.array_equal(opt["mat"], np.asarray(f.opt["mat"], np.int8))
        assert tasks.tobytes() == f.tasks.tobytes() and qp.tobytes() == f.qpool.tobytes() \
            and tp.tobytes() == f.tpool.tobytes(), f"{name}-{side}: regenerate with oracle/gen_golden.py --only-align2-range"


@pytest.mark.parametrize("name,side,f", FLAT, ids=IDS)
def test_gated_oracle_against_the_recorded_reference(name, side, f):
    want = GOLD[(name, side)][2]
    if A.is_in(side):
        got, cells = oracle.align2("oracle", f.opt, f.tasks, f.qpool, f.tpool)
        assert G.kswr_mismatch(f.tasks, got, want) is None
        assert cells[0] > 0
        return
    with pytest.raises(oracle.Align2Outside):
        oracle.align2("oracle", f.opt, f.tasks, f.qpool, f.tpool)
    keep = np.nonzero(~f.refused)[0]
    if f.opt_refused:
        keep = keep[:0]
        with pytest.raises(oracle.Align2Outside):  # every single task
            oracle.align2("oracle", f.opt, f.tasks[:1], f.qpool, f.tpool)
    else:
        assert len(keep)  # a batch of the admitted tasks alone keeps working under the same options
        got, _ = oracle.align2("oracle", f.opt, *subset(f, keep))
        assert G.kswr_mismatch(f.tasks[keep], got, want[keep]) is None
        for k in np.nonzero(f.refused)[0][:3]:
            with pytest.raises(oracle.Align2Outside):
                oracle.align2("oracle", f.opt, f.tasks[k:k + 1], f.qpool, f.tpool)


def test_every_gate_is_needed():
    """the ungated arithmetic and the reference part company on every "out" side, and only on refused tasks"""
    for name, side, f in FLAT:
        want = GOLD[(name, side)][2]
        got, _ = oracle.align2("oracle_ungated", f.opt, f.tasks, f.qpool, f.tpool)
        bad = differ(got, want)
        if A.is_in(side):
            assert len(bad) == 0, (name, side)
            continue
        gated = np.ones(len(f.tasks), bool) if f.opt_refused else f.refused
        print(f"{name}-{side}: ungated oracle != reference on {len(bad)} of {int(gated.sum())} refused tasks")
        assert len(bad) >= 1, f"{name}-{side}: the gate refuses nothing the int arithmetic gets wrong"
        assert gated[bad].all(), f"{name}-{side}: an admitted task differs"


def test_compiled_reference_reproduces_the_file():
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    for name, side, f in FLAT:
        got, _ = oracle.align2("ref", f.opt, f.tasks, f.qpool, f.tpool)
        assert G.kswr_mismatch(f.tasks, got, GOLD[(name, side)][2]) is None, (name, side)


def _check_expect(name, side, f):
    want = GOLD[(name, side)][2]
    for k, exp in f.expect.items():
        for fld, v in exp.items():
            assert int(want[fld][k]) == v, \
                f"{name}-{side} task {k} ({f.names.get(k, '')}): reference {fld} = {want[fld][k]}, the builder says {v}"
    return want


def test_reach_byte_saturation():
    for s in (4, 127, 128, 0):
        name = f"byte-sat-shift{s}"
        f = A.families()[name]["in"]
        want = _check_expect(name, "in", f)
        exact = [k for k in f.expect if f.tasks["qlen"][k] + s == 254]
        over = [k for k in f.expect if f.tasks["qlen"][k] + s == 255]
        assert exact and over
        assert all(want["score"][k] == 254 - s and want["qe"][k] == 254 - s - 1 for k in exact)
        assert all(want["score"][k] == 255 and want["qe"][k] == -1 and want["tb"][k] == -1 for k in over)
    # the issue's numbers under the defaults: 249, 250 -> themselves; 251, 252 -> 255
    f = A.families()["byte-sat-shift4"]["in"]
    want = GOLD[("byte-sat-shift4", "in")][2]
    got = {int(f.tasks["qlen"][k]): int(want["score"][k]) for k in f.expect}
    assert got == {249: 249, 250: 250, 251: 255, 252: 255}


def test_reach_word_ceiling_and_big():
    for side in ("in", "out"):
        f = A.families()["word-ceiling"][side]
        want = _check_expect("word-ceiling", side, f)
        assert 32766 in want["score"].tolist() and 32639 in want["score"].tolist()
        assert want["score"].max() == (32767 if side == "out" else 32766)  # the reference's clamp on the refused ones
    f = A.families()["word-BIG"]["in"]
    want = _check_expect("word-BIG", "in", f)
    last = [k for k, e in f.expect.items() if f.tasks["qlen"][k] == 1023 and e.get("qe") == 1022]
    assert last, "no task whose last column (j = 1022) holds the best score"
    for k in f.expect:  # the insertion was there to take and was not: each half alone, never their sum
        assert 0 < want["score"][k] < f.tasks["qlen"][k] - 2
    assert A.WORD_BIG_DERIVATION < 1 << 26


def test_reach_flag_equalities():
    f = A.families()["flags"]["in"]
    want = _check_expect("flags", "in", f)
    names = [f.names[k] for k in sorted(f.names)]
    assert len(names) == 20 and len(set(names)) == 20
    by = {f.names[k]: want[k] for k in f.names}
    for w in ("byte", "word"):
        assert by[f"{w}:xstop=S-1 stops a row early"]["te"] + 1 == by[f"{w}:xstop=S stops at te"]["te"]
        assert by[f"{w}:xsubo minsc=S runs the reverse pass"]["tb"] >= 0 > \
            by[f"{w}:xsubo minsc=S+1 skips the reverse pass (ksw.c:356)"]["tb"]
        for d in (-65, 65):
            assert by[f"{w}:second copy at te{d:+d} is outside the window"]["score2"] == 24
        for d in (-64, 64):
            assert by[f"{w}:second copy at te{d:+d} is inside the window"]["score2"] == -1
    # XSTOP at S and at S + 1 return the same record; only the rows differ (the GPU test compares cell counts)
    o = A._opt()
    for w in (A.XB, 0):
        ks = [k for k in sorted(f.names) if f.names[k].split(":")[1].startswith("xstop=S") and
              bool(f.tasks["xtra"][k] & A.XB) == bool(w)]
        rows = []
        for k in ks:
            _, c = oracle.align2("oracle", o, f.tasks[k:k + 1], f.qpool, f.tpool)
            rows.append(int(c[1]))
        assert rows[0] + 1 == rows[1] < rows[2], rows
