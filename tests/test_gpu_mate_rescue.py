"""GPU parity of the paired-end entries (bwagpu_pestat*, bwagpu_mate_rescue*):
mem_pestat and the rescue loop of mem_sam_pe with mem_matesw on the device, byte
for byte against the reference's own results (tests/golden/rescue_*.npz),
through the host and the device entries; output spans without headroom, the
retry round and the round cap (bwagpu_debug_rescue_drop), the error paths."""
import numpy as np
import pytest

import golden_io as G
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine

pytestmark = pytest.mark.gpu

_engines = {}


def engine(s) -> Engine:
    """one context per (genome, scoring options), shared by the module's tests"""
    opt, g = s.opt, s.genome
    key = (s.genome_id, tuple(int(opt[k]) for k in G.OPT_KEYS), bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        _engines[key] = Engine(0, opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e = _engines[key]
    e.set_alt(s.alt)
    e.set_regs_post(0)
    e.debug_rescue_drop(0)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))


def pestat_device(torch, eng, off, regs, n, po):
    d_off, d_regs, d_n = to_dev(torch, off), to_dev(torch, regs), to_dev(torch, n)
    d_pes = torch.full((128,), 0xAB, dtype=torch.uint8, device=torch.device("cuda", 0))
    stream = torch.cuda.Stream()
    eng.pestat_device(len(n), d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_pes.data_ptr(), po,
                      stream.cuda_stream)
    stream.synchronize()
    return d_pes.cpu().numpy().view(abi.PESTAT_DTYPE)


@pytest.mark.parametrize("name", R.RESCUE_SETS)
def test_pestat_matches_the_reference(name):
    torch = pytest.importorskip("torch")
    s = R.load(name)
    eng = engine(s)
    got = eng.pestat(s.off, s.regs, s.n, s.pairopt())
    assert got.tobytes() == s.pes.tobytes(), f"{name}: got {got} want {s.pes}"
    got = pestat_device(torch, eng, s.off, s.regs, s.n, s.pairopt())
    assert got.tobytes() == s.pes.tobytes(), f"{name} (device entry): got {got} want {s.pes}"


@pytest.mark.parametrize("case", R.PESTAT_CASES)
def test_pestat_hand_built_cases(case):
    torch = pytest.importorskip("torch")
    _, po, cases = R.load_cases()
    n, regs, want = cases[case]
    eng = engine(R.load("fr"))
    off = R.offsets(n)
    got = eng.pestat(off, regs, n, po)
    assert got.tobytes() == want.tobytes(), f"{case}: got {got} want {want}"
    if len(n):
        got = pestat_device(torch, eng, off, regs, n, po)
        assert got.tobytes() == want.tobytes(), f"{case} (device entry): got {got} want {want}"


def check_pairs(s, out, out_n, status, n_sw, out_off, expect_status, what):
    """every pair with expect_status 0 equals the fixture; every other pair has that status,
    a verbatim copy of its input and n_sw = -1"""
    assert np.array_equal(status, expect_status), \
        f"{what}: status differs at pairs {np.nonzero(status != expect_status)[0][:8].tolist()}: " \
        f"got {status[status != expect_status][:8].tolist()}"
    ok = np.repeat(expect_status == 0, 2)
    want_n = np.where(ok, s.out_n, s.n)
    assert np.array_equal(out_n, want_n), f"{what}: per-read counts differ at reads " \
        f"{np.nonzero(out_n != want_n)[0][:8].tolist()}"
    assert np.array_equal(n_sw, np.where(expect_status == 0, s.n_sw, -1)), f"{what}: n_sw differs at pairs " \
        f"{np.nonzero(n_sw != np.where(expect_status == 0, s.n_sw, -1))[0][:8].tolist()}"
    off_o = R.offsets(s.out_n)
    parts = [s.out_regs[off_o[r]:off_o[r] + s.out_n[r]] if ok[r] else s.regs[s.off[r]:s.off[r] + s.n[r]]
             for r in range(s.n_reads)]
    bad = G.region_mismatch(R.dense(out, out_off[:-1], out_n), np.concatenate(parts))
    assert bad is None, f"{what}: {bad}"


@pytest.mark.parametrize("name", R.RESCUE_SETS)
def test_mate_rescue_matches_the_reference(name):
    s = R.load(name)
    eng = engine(s)
    regs_before, n_before = s.regs.copy(), s.n.copy()
    out_off = s.out_off(8)
    out, out_n, status, n_sw = eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt())
    check_pairs(s, out, out_n, status, n_sw, out_off, np.zeros(s.n_reads // 2, np.int32), name)
    assert s.regs.tobytes() == regs_before.tobytes() and np.array_equal(s.n, n_before)
    st = eng.last_stats()
    assert st["kernel_ms"] > 0 and st["rows"] >= 1
    assert st["ext_calls"] >= st["cells"] == int(s.n_sw.sum())  # speculated >= used == the reference's calls


def test_device_entries_on_one_stream():
    """regs_post_device, pestat_device and mate_rescue_device back to back on one stream,
    on resident regions: the result of the host entries on the same input"""
    torch = pytest.importorskip("torch")
    s = R.load("ends")
    eng = engine(s)
    po = s.pairopt()
    ppo = abi.PostOpt(po.max_chain_gap, po.mask_level_redun, po.mask_level, 0)
    # the host path
    regs1, n1 = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, 3, 0, ppo)
    pes1 = eng.pestat(s.off, regs1, n1, po)
    out_off = np.concatenate([[0], np.cumsum(n1.astype(np.int64) + 8)]).astype(np.int64)
    want = eng.mate_rescue(pes1, s.seq_off, s.seq, s.off, regs1, n1, out_off, po)
    if np.array_equal(n1, s.n) and regs1.tobytes() == s.regs.tobytes():  # post-processing its own output changes nothing
        check_pairs(s, *want, out_off, np.zeros(s.n_reads // 2, np.int32), "ends, host chain")
    # the device path
    dev = torch.device("cuda", 0)
    d_seq_off, d_seq = to_dev(torch, s.seq_off), to_dev(torch, s.seq)
    bc = abi.BatchC()
    bc.n_reads, bc.seq_bytes = s.n_reads, int(s.seq_off[-1])
    bc.seq_off, bc.seq = d_seq_off.data_ptr(), d_seq.data_ptr()
    d_regs, d_off, d_n, d_ooff = to_dev(torch, s.regs), to_dev(torch, s.off), to_dev(torch, s.n), to_dev(torch, out_off)
    d_pes = torch.zeros(128, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(int(out_off[-1]) * 88, dtype=torch.uint8, device=dev)
    d_out_n = torch.zeros(s.n_reads, dtype=torch.int32, device=dev)
    d_status = torch.full((s.n_reads // 2,), -7, dtype=torch.int32, device=dev)
    d_nsw = torch.full((s.n_reads // 2,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    eng.regs_post_device(bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), 3, 0, ppo, stream.cuda_stream)
    eng.pestat_device(s.n_reads, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_pes.data_ptr(), po,
                      stream.cuda_stream)
    eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(),
                           d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(),
                           d_nsw.data_ptr(), po, stream.cuda_stream)
    stream.synchronize()
    assert d_pes.cpu().numpy().view(abi.PESTAT_DTYPE).tobytes() == pes1.tobytes()
    w_out, w_n, w_status, w_nsw = want
    got_n = d_out_n.cpu().numpy()
    assert np.array_equal(got_n, w_n) and np.array_equal(d_status.cpu().numpy(), w_status)
    assert np.array_equal(d_nsw.cpu().numpy(), w_nsw) and (w_status == 0).all()
    got = d_out.cpu().numpy().view(abi.ALNREG_DTYPE)
    bad = G.region_mismatch(R.dense(got, out_off[:-1], got_n), R.dense(w_out, out_off[:-1], w_n))
    assert bad is None, bad
    assert np.array_equal(d_n.cpu().numpy().view(np.int32), n1)  # the inputs as regs_post_device left them
    assert eng.last_stats()["ext_calls"] > 0


def test_no_headroom_overflows_exactly_the_pairs_that_grow():
    s = R.load("fr")
    eng = engine(s)
    out_off = s.out_off(0)
    out, out_n, status, n_sw = eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt())
    grows = (s.peak_n > s.n).reshape(-1, 2).any(axis=1)  # a push needs room even if the dedup then removes a region
    assert 100 < grows.sum() < len(grows)
    check_pairs(s, out, out_n, status, n_sw, out_off, np.where(grows, abi.RESCUE_OVERFLOW, 0).astype(np.int32),
                "fr without headroom")


def test_dropped_tasks_are_recomputed_in_a_second_round():
    s = R.load("rep")
    eng = engine(s)
    out_off = s.out_off(8)
    eng.debug_rescue_drop(3)
    try:
        out, out_n, status, n_sw = eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt(3))
        st = eng.last_stats()
    finally:
        eng.debug_rescue_drop(0)
    check_pairs(s, out, out_n, status, n_sw, out_off, np.zeros(s.n_reads // 2, np.int32), "rep, every third task dropped")
    assert st["rows"] >= 2, f"rounds run: {st['rows']}"


def test_round_cap_leaves_pairs_unfinished():
    s = R.load("rep")
    eng = engine(s)
    out_off = s.out_off(8)
    eng.debug_rescue_drop(3)
    try:
        out, out_n, status, n_sw = eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt(1))
        st = eng.last_stats()
    finally:
        eng.debug_rescue_drop(0)
    assert st["rows"] == 1
    assert set(np.unique(status).tolist()) == {abi.RESCUE_DONE, abi.RESCUE_UNFINISHED}
    unfinished = status == abi.RESCUE_UNFINISHED
    # a pair is unfinished only if its replay needed a dropped task: it made ksw_align2 calls, and no
    # more pairs are unfinished than tasks were dropped
    assert (s.n_sw[unfinished] > 0).all()
    assert 0 < unfinished.sum() <= st["ext_calls"] // 3
    check_pairs(s, out, out_n, status, n_sw, out_off, status, "rep, one round")


def test_all_orientations_failed_copies_the_input():
    s = R.load("mixed")
    eng = engine(s)
    pes = np.zeros(4, abi.PESTAT_DTYPE)
    pes["failed"] = 1
    out_off = s.out_off(0)
    out, out_n, status, n_sw = eng.mate_rescue(pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt())
    assert (status == 0).all() and (n_sw == 0).all() and np.array_equal(out_n, s.n)
    assert out[:len(s.regs)].tobytes() == s.regs.tobytes()
    st = eng.last_stats()
    assert st["ext_calls"] == 0 and st["cells"] == 0 and st["rows"] == 1  # no align2 launch


def test_empty_batch():
    s = R.load("fr")
    eng = engine(s)
    out, out_n, status, n_sw = eng.mate_rescue(s.pes, np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int64),
                                               np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32), np.zeros(1, np.int64))
    assert len(out_n) == 0 and len(status) == 0 and len(n_sw) == 0
    pes = eng.pestat(np.zeros(0, np.int64), np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32))
    assert pes["failed"].tolist() == [1, 1, 1, 1] and pes.tobytes() == R.load_cases()[2]["n_reads_0"][2].tobytes()


def test_errors_launch_nothing():
    s = R.load("fr")
    eng = engine(s)
    nr = 40
    seq_off, n, off = s.seq_off[:nr + 1], s.n[:nr], s.off[:nr]
    seq, regs = s.seq[:int(seq_off[-1])], s.regs[:int(n.sum())]
    out_off = np.concatenate([[0], np.cumsum(n.astype(np.int64) + 8)]).astype(np.int64)
    eng.mate_rescue(s.pes, seq_off, seq, off, regs, n, out_off, s.pairopt())  # a finished pass: its stats must stay
    before = eng.last_stats()

    def code(pes=s.pes, seq_off=seq_off, seq=seq, off=off, regs=regs, n=n, out_off=out_off, po=s.pairopt()):
        with pytest.raises(BwaGpuError) as e:
            eng.mate_rescue(pes, seq_off, seq, off, regs, n, out_off, po)
        return e.value.code

    assert code(seq_off=seq_off[:-1], n=n[:-1], off=off[:-1], out_off=out_off[:-1]) == abi.E_INVAL  # odd n_reads
    bad_n = n.copy()
    bad_n[3] = -1
    assert code(n=bad_n) == abi.E_INVAL
    bad = regs.copy()
    bad["qe"][0] = 151
    assert code(regs=bad) == abi.E_INVAL                                   # qe outside its read
    bad["qe"][0], bad["qb"][0] = 100, -1
    assert code(regs=bad) == abi.E_INVAL
    small = out_off.copy()
    small[1:] -= 9
    assert code(out_off=small) == abi.E_INVAL                              # a span smaller than its input
    assert code(po=s.pairopt(0)) == abi.E_INVAL and code(po=s.pairopt(9)) == abi.E_INVAL
    wide = s.pes.copy()
    wide["high"][1] = wide["low"][1] + (1 << 20) + 1
    assert code(pes=wide) == abi.E_UNSUPPORTED
    with pytest.raises(BwaGpuError) as e:
        eng.pestat(off, regs, bad_n, s.pairopt())
    assert e.value.code == abi.E_INVAL
    assert eng.last_stats() == before
    # options ksw_align2 is not run with on the device (align2_opt_unsupported)
    opt0 = dict(s.opt, o_ins=0)
    g = s.genome
    e0 = Engine(0, opt0, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    try:
        with pytest.raises(BwaGpuError) as e:
            e0.mate_rescue(s.pes, seq_off, seq, off, regs, n, out_off, s.pairopt())
        assert e.value.code == abi.E_UNSUPPORTED
    finally:
        e0.close()


def test_long_read_is_unsupported_per_pair():
    s = R.load("fr")
    eng = engine(s)
    # pair 0 as it is, pair 1 with a 1024-base first read and no regions for it
    L = abi.MAX_READ_LEN + 1
    lens = np.diff(s.seq_off[:5]).astype(np.int64)
    seqs = [s.seq[s.seq_off[r]:s.seq_off[r + 1]] for r in range(4)]
    seqs[2] = np.resize(seqs[2], L)
    lens[2] = L
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = s.n[:4].copy()
    n[2] = 0
    off = s.off[:4]
    out_off = np.concatenate([[0], np.cumsum(n.astype(np.int64) + 8)]).astype(np.int64)
    out, out_n, status, n_sw = eng.mate_rescue(s.pes, seq_off, np.concatenate(seqs), off, s.regs, n, out_off, s.pairopt())
    assert status.tolist() == [0, abi.RESCUE_UNSUPPORTED] and n_sw[1] == -1
    assert np.array_equal(out_n[2:], n[2:])
    assert out[out_off[3]:out_off[3] + n[3]].tobytes() == s.regs[off[3]:off[3] + n[3]].tobytes()
    assert n_sw[0] == s.n_sw[0] and out_n[0] == s.out_n[0] and out_n[1] == s.out_n[1]
