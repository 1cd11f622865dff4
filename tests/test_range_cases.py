"""CPU: the task families at the edges of the packed kernels' range gates
(tests/range_cases.py) are what they claim to be.

* the instrumented oracle entry (oracle_extend_batch_extremes, which shares
  ksw_ext.c's row loop) returns the six outputs of oracle_extend_batch, on
  every family and on the ksw_edge_* golden sets;
* the committed golden file (tests/golden/ksw_range.npz: the same families
  through the reference's ksw_extend2) holds these families' inputs, and the
  oracle reproduces its results; where oracle/_ref is built, the compiled
  reference does too;
* reach: in every score-ceiling, shifted-ceiling and 32-bit family some "in"
  task's largest H equals the last hb the gate admits, and some "out" task's
  the first it refuses (quad_bound_ok / wave_bound_ok, pure.h) -- the numbers
  are range_cases', derived from the gates, and only the oracle says whether a
  task gets there;
* the two quantities the gates bound but no call reaches (the z-drop term, the
  rows run) are printed with the largest values seen.
"""
import numpy as np
import pytest

import golden_io as G
import oracle
import range_cases as R

FLAT = R.flat()
IDS = [f"{n}-{s}" for n, s, _ in FLAT]


def six(r):
    return r.view(np.int32).reshape(-1, 6)


def assert_same(tasks, got, want, what):
    bad = np.nonzero((six(got) != six(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} tasks differ; first {tasks[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"


def test_family_shapes():
    """40..150 tasks a family; qlen <= 255 but in the 32-bit one; every h0 positive; both
    sides hold the same constructions"""
    names = set()
    for name, side, f in FLAT:
        names.add(name)
        assert 40 <= len(f.tasks) <= 150, (name, side, len(f.tasks))
        assert f.tasks["h0"].min() >= 1
        assert f.side == side and f.gate
        if name == "wave32":
            assert set(f.tasks["qlen"].tolist()) == {100, 255, 700, 1022}
        else:
            assert f.tasks["qlen"].max() <= 255
        assert (f.tasks["qoff"] + f.tasks["qlen"]).max() <= len(f.qpool)
        assert (f.tasks["toff"] + f.tasks["tlen"]).max() <= len(f.tpool)
    fams = R.families()
    for name, d in fams.items():
        if "out" in d:
            assert len(d["in"].tasks) == len(d["out"].tasks)
            assert np.array_equal(d["in"].tasks["qlen"], d["out"].tasks["qlen"])
    assert len(names) >= 18


@pytest.mark.parametrize("name,side,f", FLAT, ids=IDS)
def test_extremes_entry_returns_the_same_outputs(name, side, f):
    want, cells = oracle.extend("oracle", f.opt, f.tasks, f.qpool, f.tpool)
    got, xcells, ext = oracle.extend_extremes(f.opt, f.tasks, f.qpool, f.tpool)
    assert_same(f.tasks, got, want, "extremes entry")
    assert np.array_equal(cells, xcells) and int(ext[:, 4].sum()) == cells[1]
    assert (ext[:, 0] >= f.tasks["h0"]).all() and (ext[:, 0] >= want["score"]).all()


@pytest.mark.parametrize("name", G.KSW_SETS)
def test_extremes_entry_on_the_golden_edge_sets(name):
    opt, tasks, want, qp, tp = G.load_tasks(name)
    got, _, ext = oracle.extend_extremes(opt, tasks, qp, tp)
    assert_same(tasks, got, want, name)
    live = tasks["h0"] > 0
    assert (ext[live, 0] == np.maximum(want["score"][live], tasks["h0"][live])).all()  # max H = the returned max
    assert (ext[~live] == 0).all()


def test_golden_file_holds_these_families():
    gold = G.load_range()
    assert set(gold) == {(n, s) for n, s, _ in FLAT}
    for name, side, f in FLAT:
        opt, tasks, want, qp, tp = gold[(name, side)]
        assert all(int(opt[k]) == int(f.opt[k]) for k in G.OPT_KEYS), (name, side)
        assert np.array_equal(opt["mat"], np.asarray(f.opt["mat"], np.int8))
        assert np.array_equal(tasks, f.tasks) and np.array_equal(qp, f.qpool) and np.array_equal(tp, f.tpool), \
            f"{name}-{side}: regenerate with oracle/gen_golden.py --only-range"
        got, _ = oracle.extend("oracle", f.opt, f.tasks, f.qpool, f.tpool)
        assert_same(f.tasks, got, want, f"{name}-{side} oracle vs the reference's recorded results")


def test_reference_agrees_on_every_family():
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    for name, side, f in FLAT:
        a, _ = oracle.extend("oracle", f.opt, f.tasks, f.qpool, f.tpool)
        b, _ = oracle.extend("ref", f.opt, f.tasks, f.qpool, f.tpool)
        assert_same(f.tasks, a, b, f"{name}-{side} oracle vs compiled reference")


def test_reach():
    """the families that claim a peak reach it exactly: the last admitted hb on the "in"
    side, one more on the "out" side (mat_mismatch127: the same hb on both)"""
    claimed = 0
    for name, side, f in FLAT:
        _, _, ext = oracle.extend_extremes(f.opt, f.tasks, f.qpool, f.tpool)
        gate_hb = f.tasks["h0"].astype(np.int64) + f.tasks["qlen"].astype(np.int64) * R.max_mat(f.opt)
        assert (ext[:, 0] <= gate_hb).all(), f"{name}-{side}: an H above the gate's bound h0 + qlen * max_mat"
        if f.peak is None:
            continue
        claimed += 1
        assert (gate_hb == f.peak).all(), f"{name}-{side}: a task's gate value is not {f.peak}"
        assert int(ext[:, 0].max()) == f.peak, f"{name}-{side}: largest H {int(ext[:, 0].max())}, claimed {f.peak}"
    peaks = {(n, s): f.peak for n, s, f in FLAT}
    # pure.h quad_bound_ok: hb < 4096; (hb << 3) + 128 < 32768; (hb << 4) + 128 < 32768; wave_bound_ok: hb < 2^21
    assert peaks[("ceiling_a1", "in")] == peaks[("ceiling_a3", "in")] == 4095
    assert peaks[("shifted_a4", "in")] == peaks[("shifted_a7", "in")] == (32767 - 128) >> 3 == 4079
    assert peaks[("shifted_a8", "in")] == peaks[("shifted_a15", "in")] == peaks[("shifted_diag15", "in")] \
        == (32767 - 128) >> 4 == 2039
    assert peaks[("wave32", "in")] == (1 << 21) - 1
    for n in ("ceiling_a1", "ceiling_a3", "shifted_a4", "shifted_a7", "shifted_a8", "shifted_a15", "shifted_diag15",
              "wave32"):
        assert peaks[(n, "out")] == peaks[(n, "in")] + 1
    assert claimed == 18


def test_report_the_unreachable_quantities():
    """quad_rows_ok bounds the z-drop term by 28671 and the rows by 16383; no call gets near
    either (the term: both cells lie on paths from h0, so about 2 hb; the rows: the plan's
    LDS rows).  Printed for DESIGN.md; asserted only to stay inside the gate."""
    zt = rows = 0
    for name, side, f in FLAT:
        if side != "in" or not f.packed:
            continue
        _, _, ext = oracle.extend_extremes(f.opt, f.tasks, f.qpool, f.tpool)
        zt, rows = max(zt, int(ext[:, 3].max())), max(rows, int(ext[:, 4].max()))
        print(f"{name}: largest H {ext[:, 0].max()}, E {ext[:, 1].max()}, F {ext[:, 2].max()}, "
              f"z-drop term {ext[:, 3].max()}, rows {ext[:, 4].max()}")
    print(f"largest z-drop term of any packed family: {zt} (gate: < 28672); rows run: {rows} (gate: < 16384)")
    assert 0 < zt < 28672 and 0 < rows < 16384
