"""GPU parity of bwagpu_pair_select / bwagpu_pair_select_device: mem_pair, the proper-pair /
unpaired decision and the mapq arithmetic of mem_sam_pe on the device, byte for byte against
tests/golden/pair_*.npz (the reference's own functions, pinned against its mem_sam_pe), with
and without MEM_F_NOPAIRING, through the host and the device entry; the statuses, the refused
flags and argument errors, and the device chain from regs_post to pair_select on one stream."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import pair_io as P
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine

pytestmark = pytest.mark.gpu

_engines = {}


def engine(d) -> Engine:
    opt, g = d.opt, d.genome
    key = (d.genome_id, d.name if d.genome_id else "", tuple(int(opt[k]) for k in G.OPT_KEYS),
           bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        _engines[key] = Engine(0, opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e = _engines[key]
    e.set_alt(d.alt)
    e.set_regs_post(0)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).copy()
    if b.size == 0:  # a batch without regions still hands the entry a valid pointer
        b = np.zeros(88, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


def select_device(torch, eng, d, so, in_status=None):
    dev = torch.device("cuda", 0)
    d_pes, d_off, d_regs = to_dev(torch, d.pes), to_dev(torch, d.off), to_dev(torch, d.marked)
    d_n, d_npri = to_dev(torch, d.n), to_dev(torch, d.n_pri)
    d_in = to_dev(torch, np.asarray(in_status, np.int32)) if in_status is not None else None
    np_ = d.n_reads // 2
    d_sel = torch.full((max(np_, 1) * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_mapq = torch.full((max(len(d.marked), 1),), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    eng.pair_select_device(d_pes.data_ptr(), d.n_reads, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(),
                           d_npri.data_ptr(), d_in.data_ptr() if d_in is not None else None, d_sel.data_ptr(),
                           d_mapq.data_ptr(), d.pair_id0, so, stream.cuda_stream)
    stream.synchronize()
    return (d_sel.cpu().numpy().view(abi.PAIRSEL_DTYPE)[:np_], d_mapq.cpu().numpy()[:len(d.marked)],
            d_regs.cpu().numpy().view(abi.ALNREG_DTYPE)[:len(d.marked)])


def check(what, d, mode, got, expect_status=None):
    """pairs with expect_status 0 equal the fixture; the others have that status, an empty
    record, out_mapq -1 and their regions untouched"""
    sel, om, regs = got
    np_ = d.n_reads // 2
    status = np.zeros(np_, np.int32) if expect_status is None else np.asarray(expect_status, np.int32)
    want_sel = d.sel[mode].copy()
    want_om = d.out_mapq[mode].copy()
    want_regs = (d.final if mode == 0 else d.marked).copy()
    for p in np.nonzero(status)[0]:
        t = np.zeros((), abi.PAIRSEL_DTYPE)
        t["status"], t["n_pri"], t["z"], t["alt"] = status[p], d.n_pri[2 * p:2 * p + 2], -1, -1
        want_sel[p] = t
        lo, hi = int(d.off[2 * p]), int(d.off[2 * p + 1] + d.n[2 * p + 1])
        want_om[lo:hi] = -1
        want_regs[lo:hi] = d.marked[lo:hi]
    for f in abi.PAIRSEL_DTYPE.names:
        if f == "pad":
            continue
        diff = np.nonzero((sel[f] != want_sel[f]).reshape(np_, -1).any(axis=1))[0]
        assert len(diff) == 0, f"{what}: sel.{f} differs at pairs {diff[:8].tolist()}: got {sel[f][diff[:4]].tolist()} " \
            f"want {want_sel[f][diff[:4]].tolist()}"
    assert sel.tobytes() == want_sel.tobytes(), what
    assert np.array_equal(om, want_om), f"{what}: out_mapq differs at regions {np.nonzero(om != want_om)[0][:8].tolist()}"
    bad = G.region_mismatch(regs, want_regs)
    assert bad is None, f"{what}: {bad}"
    assert regs.tobytes() == want_regs.tobytes(), what


def run_both(torch, what, d, mode, expect_status=None, in_status=None):
    eng = engine(d)
    so = d.selopt(abi.MEM_F_NOPAIRING if mode else 0)
    marked = d.marked.copy()
    check(what, d, mode, eng.pair_select(d.pes, d.off, d.marked, d.n, d.n_pri, d.pair_id0, so, in_status),
          expect_status)
    assert d.marked.tobytes() == marked.tobytes()
    check(what + " (device entry)", d, mode, select_device(torch, eng, d, so, in_status), expect_status)


@pytest.mark.parametrize("mode", [0, 1], ids=["pairing", "nopairing"])
@pytest.mark.parametrize("name", P.PAIR_SETS)
def test_sets_match_the_reference(name, mode):
    torch = pytest.importorskip("torch")
    run_both(torch, f"pair_{name}", P.load(name), mode)


@pytest.mark.parametrize("case", [c for c in P.CASES if c != "pri_cap_plus_1"])
def test_hand_built_cases(case):
    torch = pytest.importorskip("torch")
    d = P.load_cases()[case]
    for mode in (0, 1):
        run_both(torch, f"{case} mode {mode}", d, mode)


def test_too_many_primaries_leave_the_pair_untouched():
    torch = pytest.importorskip("torch")
    d = P.load_cases()["pri_cap_plus_1"]
    assert d.n_pri[0] + d.n_pri[1] == abi.SEL_MAX_REGS + 1
    run_both(torch, "pri_cap_plus_1", d, 0, expect_status=[abi.SEL_TOO_MANY, 0])
    run_both(torch, "pri_cap_plus_1 nopairing", d, 1, expect_status=[abi.SEL_TOO_MANY, 0])  # the cap is one rule


def test_in_status_is_passed_through():
    torch = pytest.importorskip("torch")
    d = P.load("rep")
    np_ = d.n_reads // 2
    in_status = np.zeros(np_, np.int32)
    in_status[::7] = abi.RESCUE_OVERFLOW
    in_status[3] = abi.RESCUE_UNFINISHED
    expect = np.where(in_status != 0, abi.SEL_SKIPPED, 0)
    run_both(torch, "rep with in_status", d, 0, expect_status=expect, in_status=in_status)


def test_log_argument_outside_the_table():
    """sub_n + 1 beyond the context's log table: the pair gets a status, no wrong answer"""
    d = P.load("shift")
    eng = engine(d)
    regs = d.marked.copy()
    p = int(np.nonzero((d.sel[0]["branch"] == 1) & (d.n[0::2] == 1) & (d.n[1::2] == 1))[0][0])
    regs["sub_n"][d.off[2 * p]] = 1 << 16
    sel, om, out = eng.pair_select(d.pes, d.off, regs, d.n, d.n_pri, d.pair_id0, d.selopt())
    assert sel["status"][p] == abi.SEL_TOO_MANY and sel["status"].sum() == abi.SEL_TOO_MANY
    lo, hi = int(d.off[2 * p]), int(d.off[2 * p + 1] + d.n[2 * p + 1])
    assert out[lo:hi].tobytes() == regs[lo:hi].tobytes() and (om[lo:hi] == -1).all()
    keep = np.ones(len(regs), bool)
    keep[lo:hi] = False
    assert out[keep].tobytes() == d.final[keep].tobytes() and np.array_equal(om[keep], d.out_mapq[0][keep])


def test_refused_flags_and_argument_errors_launch_nothing():
    d = P.load("fr")
    eng = engine(d)
    nr = 40
    n, off, n_pri = d.n[:nr], d.off[:nr], d.n_pri[:nr]
    regs = d.marked[:int(n.sum())]
    eng.pair_select(d.pes, off, regs, n, n_pri, d.pair_id0, d.selopt())
    before = eng.last_stats()

    def code(pes=d.pes, off=off, regs=regs, n=n, n_pri=n_pri, so=d.selopt()):
        with pytest.raises(BwaGpuError) as e:
            eng.pair_select(pes, off, regs, n, n_pri, d.pair_id0, so)
        return e.value.code

    for f in (abi.MEM_F_ALL, abi.MEM_F_NO_MULTI, abi.MEM_F_PRIMARY5, abi.MEM_F_KEEP_SUPP_MAPQ):
        assert code(so=d.selopt(f)) == abi.E_UNSUPPORTED
        assert code(so=d.selopt(f | abi.MEM_F_NOPAIRING)) == abi.E_UNSUPPORTED
    assert code(off=off[:-1], n=n[:-1], n_pri=n_pri[:-1]) == abi.E_INVAL  # odd n_reads
    bad = n.copy()
    bad[3] = -1
    assert code(n=bad) == abi.E_INVAL
    bad = n_pri.copy()
    bad[2] = n[2] + 1
    assert code(n_pri=bad) == abi.E_INVAL
    over = off.copy()
    over[5] = off[4]
    assert code(off=over) == abi.E_INVAL  # spans overlap
    bad = regs.copy()
    bad["rid"][0] = 99
    assert code(regs=bad) == abi.E_INVAL
    wide = d.pes.copy()
    wide["high"][1] = wide["low"][1] + (1 << 20) + 1
    assert code(pes=wide) == abi.E_UNSUPPORTED
    so = d.selopt()
    pes = np.ascontiguousarray(d.pes)
    vp = C.c_void_p
    assert eng.lib.bwagpu_pair_select(eng.ctx, C.byref(so), pes.ctypes.data_as(vp), 0, nr, None, None, None, None,
                                      None, None, None) == abi.E_INVAL
    assert eng.lib.bwagpu_pair_select(eng.ctx, C.byref(so), None, 0, nr, None, None, None, None, None, None,
                                      None) == abi.E_INVAL
    assert eng.lib.bwagpu_pair_select_device(eng.ctx, C.byref(so), None, 0, nr, None, None, None, None, None, None,
                                             None, None) == abi.E_INVAL
    so = d.selopt(abi.MEM_F_ALL)
    assert eng.lib.bwagpu_pair_select_device(eng.ctx, C.byref(so), None, 0, nr, None, None, None, None, None, None,
                                             None, None) == abi.E_UNSUPPORTED
    assert eng.last_stats() == before
    sel, om, out = eng.pair_select(d.pes, np.zeros(0, np.int64), np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32),
                                   np.zeros(0, np.int32))
    assert len(sel) == 0 and len(om) == 0 and len(out) == 0


def test_device_chain_on_one_stream():
    """regs_post_device -> pestat_device -> mate_rescue_device -> mark_primary_device ->
    pair_select_device on one stream, on resident regions"""
    torch = pytest.importorskip("torch")
    s = R.load("ends")
    d = P.load("ends")
    eng = engine(d)
    po = s.pairopt()
    ppo = abi.PostOpt(po.max_chain_gap, po.mask_level_redun, po.mask_level, 0)
    so = d.selopt()
    out_off = s.out_off(8)
    # the host entries on the same input
    regs1, n1 = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, 3, 0, ppo)
    pes1 = eng.pestat(s.off, regs1, n1, po)
    w_out, w_n, w_status, _ = eng.mate_rescue(pes1, s.seq_off, s.seq, s.off, regs1, n1, out_off, po)
    w_marked, w_npri, w_mstat = eng.mark_primary(out_off[:-1], w_out, w_n, 2 * d.pair_id0, so)
    w_sel, w_om, w_final = eng.pair_select(pes1, out_off[:-1], w_marked, w_n, w_npri, d.pair_id0, so, w_status)
    assert (w_status == 0).all() and (w_mstat == 0).all()
    if np.array_equal(w_n, d.n) and pes1.tobytes() == d.pes.tobytes():  # post-processing its own output changes nothing
        check("ends, host chain", d, 0, (w_sel, R.dense(w_om, out_off[:-1], w_n), R.dense(w_final, out_off[:-1], w_n)))
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
    d_npri = torch.full((s.n_reads,), -7, dtype=torch.int32, device=dev)
    d_mstat = torch.full((s.n_reads,), -7, dtype=torch.int32, device=dev)
    d_sel = torch.full((s.n_reads // 2 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_mapq = torch.full((int(out_off[-1]),), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    eng.regs_post_device(bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), 3, 0, ppo, st)
    eng.pestat_device(s.n_reads, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_pes.data_ptr(), po, st)
    eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(),
                           d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(),
                           d_nsw.data_ptr(), po, st)
    eng.mark_primary_device(s.n_reads, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_npri.data_ptr(),
                            d_mstat.data_ptr(), 2 * d.pair_id0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), s.n_reads, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(),
                           d_npri.data_ptr(), d_status.data_ptr(), d_sel.data_ptr(), d_mapq.data_ptr(), d.pair_id0, so,
                           st)
    stream.synchronize()
    assert d_pes.cpu().numpy().view(abi.PESTAT_DTYPE).tobytes() == pes1.tobytes()
    assert (d_status.cpu().numpy() == 0).all() and (d_mstat.cpu().numpy() == 0).all()
    got_n = d_out_n.cpu().numpy()
    assert np.array_equal(got_n, w_n) and np.array_equal(d_npri.cpu().numpy(), w_npri)
    got = R.dense(d_out.cpu().numpy().view(abi.ALNREG_DTYPE), out_off[:-1], got_n)
    bad = G.region_mismatch(got, R.dense(w_final, out_off[:-1], w_n))
    assert bad is None, bad
    assert d_sel.cpu().numpy().view(abi.PAIRSEL_DTYPE).tobytes() == w_sel.tobytes()
    assert np.array_equal(R.dense(d_mapq.cpu().numpy(), out_off[:-1], got_n), R.dense(w_om, out_off[:-1], w_n))
