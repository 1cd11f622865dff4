"""The mate-rescue fixtures (tests/golden/rescue_*.npz, tools_dev/gen_rescue_fixture.py)
load, are consistent, and cover what the generator's floors promise; the Python
mirrors of the new structs have the ABI's sizes.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import golden_io as G
import rescue_io as R
from bwagpu import abi


def test_struct_sizes():
    assert C.sizeof(abi.PairOpt) == 32
    assert abi.PESTAT_DTYPE.itemsize == 32
    assert [abi.PESTAT_DTYPE.fields[k][1] for k in ("low", "high", "failed", "avg", "std")] == [0, 4, 8, 16, 24]
    d = abi.default_pairopt()
    assert (d.max_ins, d.max_matesw, d.pen_unpaired, d.min_seed_len, d.max_chain_gap, d.max_rounds) == \
        (10000, 50, 17, 19, 10000, 3)
    assert (d.mask_level_redun, d.mask_level) == (np.float32(0.95), np.float32(0.5))
    assert (abi.RESCUE_DONE, abi.RESCUE_UNFINISHED, abi.RESCUE_OVERFLOW, abi.RESCUE_UNSUPPORTED) == (0, 1, 2, 3)


@pytest.mark.parametrize("name", R.RESCUE_SETS)
def test_set_loads_and_is_consistent(name):
    s = R.load(name)
    assert os.path.getsize(os.path.join(G.GOLD, f"rescue_{name}.npz")) <= 1 << 20
    nr = s.n_reads
    assert nr % 2 == 0 and nr >= 800
    assert len(s.seq_off) == nr + 1 and s.seq_off[-1] == len(s.seq) and s.seq.max() <= 4
    assert s.n.sum() == len(s.regs) and s.out_n.sum() == len(s.out_regs)
    assert len(s.out_n) == nr and len(s.peak_n) == nr and len(s.n_sw) == nr // 2
    assert (s.peak_n >= s.n).all() and (s.peak_n >= s.out_n).all() and (s.n_sw >= 0).all()
    lens = np.diff(s.seq_off)
    for regs, off, n in ((s.regs, s.off, s.n), (s.out_regs, R.offsets(s.out_n), s.out_n)):
        l_seq = np.repeat(lens, n)
        assert (regs["qb"] >= 0).all() and (regs["qe"] > regs["qb"]).all() and (regs["qe"] <= l_seq).all()
    # a pair that made no ksw_align2 call keeps its regions
    off_o = R.offsets(s.out_n)
    for p in np.nonzero(s.n_sw == 0)[0][:200]:
        for r in (2 * p, 2 * p + 1):
            assert s.out_n[r] == s.n[r]
            assert s.out_regs[off_o[r]:off_o[r] + s.out_n[r]].tobytes() == s.regs[s.off[r]:s.off[r] + s.n[r]].tobytes()
    # pes: bit patterns of live orientations are finite, failed ones are mem_pestat's memset
    assert (s.pes["pad"] == 0).all() and (s.pes["failed"] == 0).any()
    for r in range(4):
        if s.pes["failed"][r] == 0:
            assert np.isfinite(s.pes["avg"][r]) and np.isfinite(s.pes["std"][r])
            assert 1 <= s.pes["low"][r] <= s.pes["high"][r]
    assert s.pairopt().max_matesw == (2 if name == "rep_sw2" else 50)


def test_floors_are_met():
    total = dict.fromkeys(R.COVERAGE_KEYS, 0)
    for name in R.RESCUE_SETS:
        for k, v in R.load(name).coverage.items():
            total[k] += v
    short = {k: (total[k], f) for k, f in R.FLOORS.items() if total[k] < f}
    assert not short, f"coverage floors not met (have, need): {short}"
    # two orientations alive somewhere, a set with candidates cut by max_matesw
    assert (R.load("mixed").pes["failed"] == 0).sum() >= 2
    assert R.load("rep_sw2").coverage["calls_cut"] >= 5


def test_pestat_cases_load():
    opt, po, cases = R.load_cases()
    assert sorted(cases) == sorted(R.PESTAT_CASES)
    assert C.sizeof(po) == 32 and po.max_ins == 10000
    for name, (n, regs, pes) in cases.items():
        assert n.sum() == len(regs) and len(pes) == 4 and (pes["pad"] == 0).all()
        live = pes["failed"] == 0
        assert np.isfinite(pes["avg"][live]).all() and np.isfinite(pes["std"][live]).all()
    failed = {k: cases[k][2]["failed"].tolist() for k in cases}
    assert failed["all_under_min_cnt"] == [1, 1, 1, 1] and failed["n_reads_0"] == [1, 1, 1, 1]
    assert failed["exactly_10"] == [1, 0, 1, 1]
    assert failed["failed_by_ratio"] == [1, 0, 1, 1] and cases["failed_by_ratio"][2]["high"][2] > 0  # computed, then failed
    assert failed["two_alive"] == [1, 0, 0, 1]
    assert cases["low_clamped"][2]["low"][1] == 1
    assert len(cases["odd_n_reads"][0]) % 2 == 1 and len(cases["n_reads_0"][0]) == 0
