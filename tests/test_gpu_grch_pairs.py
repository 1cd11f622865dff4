"""GPU parity of the stages after the extension at GRCh38 coordinates: bwagpu_regs_post*,
bwagpu_pestat*, bwagpu_mate_rescue*, bwagpu_mark_primary*, bwagpu_pair_select* and the
CIGAR jobs and records behind them, byte for byte against the reference's own answers on
the composite genome of tests/grch_io.py (tests/golden/grch_*.npz): forward coordinates
past 2^31, two-strand coordinates past 2^32, rid 0-2 and 198-200 of 201 contigs.  Every
input is the small-genome fixture's, translated; a 64-bit coordinate that loses its high
word, a sign-extended low word or an int distance shows here and nowhere else."""
import numpy as np
import pytest

import golden_io as G
import grch_io as GI
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import Engine
from test_gpu_mark_primary import mark_device
from test_gpu_mate_rescue import check_pairs, pestat_device, to_dev
from test_gpu_pair_select import check as check_select
from test_gpu_pair_select import select_device

pytestmark = pytest.mark.gpu

SENT = 0xA5
_engines = {}  # at most two alive: every set here has one scoring, a second key only evicts


def engine(opt, alt) -> Engine:
    key = (tuple(int(opt[k]) for k in G.OPT_KEYS), bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        while len(_engines) >= 2:
            _engines.pop(next(iter(_engines))).close()
        g = GI.composite().genome
        _engines[key] = Engine(0, opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e = _engines[key]
    e.set_alt(alt)
    e.set_regs_post(0)
    e.debug_rescue_drop(0)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def batch_c(torch, s):
    d_seq_off, d_seq = to_dev(torch, s.seq_off), to_dev(torch, s.seq)
    bc = abi.BatchC()
    bc.n_reads, bc.seq_bytes = len(s.n), int(s.seq_off[-1])
    bc.seq_off, bc.seq = d_seq_off.data_ptr(), d_seq.data_ptr()
    return bc, (d_seq_off, d_seq)


def check_regs(what, got, got_n, want):
    want_regs, want_n = want
    assert np.array_equal(got_n, want_n), f"{what}: per-read counts differ at reads {np.nonzero(got_n != want_n)[0][:8].tolist()}"
    bad = G.region_mismatch(got, want_regs)
    assert bad is None, f"{what}: {bad}"
    assert np.ascontiguousarray(got).tobytes() == want_regs.tobytes(), what


@pytest.mark.parametrize("name", GI.POST_SETS)
def test_regs_post(torch, name):
    """flags 3 through the host and the device entry; flags 7 is flags 3 followed by the marking
    (bwagpu_regs_post refuses BWAGPU_POST_PRIMARY), through both entries too"""
    s = GI.load_post(name)
    eng = engine(s.opt, s.alt)
    before = s.regs.copy()
    regs, n = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, 3, s.id0, s.popt)
    assert s.regs.tobytes() == before.tobytes()
    got3 = R.dense(regs, s.off, n)
    check_regs(f"{name} flags 3", got3, n, s.want[3])
    assert eng.last_stats()["ext_calls"] >= s.coverage["patched_copy_a"] + s.coverage["patched_copy_b"]
    bc, keep = batch_c(torch, s)
    d_regs, d_off, d_n = to_dev(torch, s.regs), to_dev(torch, s.off), to_dev(torch, s.n)
    stream = torch.cuda.Stream()
    eng.regs_post_device(bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), 3, s.id0, s.popt, stream.cuda_stream)
    stream.synchronize()
    dn = d_n.cpu().numpy().view(np.int32)
    check_regs(f"{name} flags 3 (device entry)", R.dense(d_regs.cpu().numpy().view(abi.ALNREG_DTYPE), s.off, dn), dn, s.want[3])
    del keep
    so = abi.default_selopt()
    so.mask_level = float(s.popt.mask_level)
    off3 = G.offsets(n)
    assert n.max() <= abi.SEL_MAX_REGS
    for what, (got, _, status) in (("host", eng.mark_primary(off3, got3, n, s.id0, so)),
                                   ("device", mark_device(torch, eng, off3, got3, n, s.id0, so))):
        assert (status == abi.SEL_DONE).all()
        check_regs(f"{name} flags 7 ({what} marking)", got, n, s.want[7])


@pytest.mark.parametrize("name", GI.RESCUE_SETS + [GI.CROSS])
def test_pestat(torch, name):
    s = GI.load_rescue(name)
    eng = engine(s.opt, s.alt)
    got = eng.pestat(s.off, s.regs, s.n, s.pairopt())
    assert got.tobytes() == s.pes_own.tobytes(), f"{name}: got {got} want {s.pes_own}"
    got = pestat_device(torch, eng, s.off, s.regs, s.n, s.pairopt())
    assert got.tobytes() == s.pes_own.tobytes(), f"{name} (device entry): got {got} want {s.pes_own}"


def rescue(s, eng, rounds=3):
    regs_before, n_before = s.regs.copy(), s.n.copy()
    out_off = s.out_off(8)
    out, out_n, status, n_sw = eng.mate_rescue(s.pes, s.seq_off, s.seq, s.off, s.regs, s.n, out_off, s.pairopt(rounds))
    st = eng.last_stats()
    check_pairs(s, out, out_n, status, n_sw, out_off, np.zeros(s.n_reads // 2, np.int32), s.name)
    assert s.regs.tobytes() == regs_before.tobytes() and np.array_equal(s.n, n_before)
    assert st["cells"] == int(s.n_sw.sum()) and st["ext_calls"] >= st["cells"]
    return st


@pytest.mark.parametrize("name", GI.RESCUE_SETS + [GI.CROSS])
def test_mate_rescue(name):
    s = GI.load_rescue(name)
    rescue(s, engine(s.opt, s.alt))


def test_mate_rescue_retry_round_rebuilds_windows():
    s = GI.load_rescue("fr")
    eng = engine(s.opt, s.alt)
    eng.debug_rescue_drop(3)
    try:
        st = rescue(s, eng)
    finally:
        eng.debug_rescue_drop(0)
    assert st["rows"] >= 2, f"rounds run: {st['rows']}"


@pytest.mark.parametrize("mode", [0, 1], ids=["pairing", "nopairing"])
@pytest.mark.parametrize("name", GI.PAIR_SETS + [GI.CROSS])
def test_mark_primary_and_pair_select(torch, name, mode):
    d = GI.load_pair(name)
    eng = engine(d.opt, d.alt)
    so = d.selopt(abi.MEM_F_NOPAIRING if mode else 0)
    for what, (got, n_pri, status) in (("host", eng.mark_primary(d.off, d.regs, d.n, 2 * d.pair_id0, so)),
                                       ("device", mark_device(torch, eng, d.off, d.regs, d.n, 2 * d.pair_id0, so))):
        assert (status == abi.SEL_DONE).all(), what
        bad = G.region_mismatch(got, d.marked)
        assert bad is None, f"{name} marking ({what}): {bad}"
        assert got.tobytes() == d.marked.tobytes() and np.array_equal(n_pri, d.n_pri), what
    marked = d.marked.copy()
    check_select(f"grch pair_{name}", d, mode, eng.pair_select(d.pes, d.off, d.marked, d.n, d.n_pri, d.pair_id0, so))
    assert d.marked.tobytes() == marked.tobytes()
    check_select(f"grch pair_{name} (device entry)", d, mode, select_device(torch, eng, d, so))


def test_device_chain_on_one_stream(torch):
    """regs_post_device -> pestat_device -> mate_rescue_device -> mark_primary_device -> pair_select_device ->
    reg2aln_jobs_device -> reg2aln_device on translated `ends`, nothing copied to the host between them:
    every stage's result against the fixtures, the records against the reference's mem_reg2aln"""
    s, d = GI.load_rescue(GI.ALN_SET), GI.load_pair(GI.ALN_SET)
    jobs, exp, ops, mds = GI.load_aln()
    eng = engine(d.opt, d.alt)
    po, so = s.pairopt(), d.selopt()
    ppo = abi.PostOpt(po.max_chain_gap, po.mask_level_redun, po.mask_level, 0)
    out_off = s.out_off(8)
    dev = torch.device("cuda", 0)
    nr, span = s.n_reads, int(out_off[-1])
    bc, keep = batch_c(torch, s)
    d_regs, d_off, d_n, d_ooff = to_dev(torch, s.regs), to_dev(torch, s.off), to_dev(torch, s.n), to_dev(torch, out_off)
    d_pes = torch.zeros(128, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(span * 88, dtype=torch.uint8, device=dev)
    d_out_n = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_status = torch.full((nr // 2,), -7, dtype=torch.int32, device=dev)
    d_nsw = torch.full((nr // 2,), -7, dtype=torch.int32, device=dev)
    d_npri = torch.full((nr,), -7, dtype=torch.int32, device=dev)
    d_mstat = torch.full((nr,), -7, dtype=torch.int32, device=dev)
    d_sel = torch.full((nr // 2 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_mapq = torch.full((span,), -7, dtype=torch.int32, device=dev)
    cap, max_ops, max_md = len(jobs) + 7, GI.ALN_MAX_OPS, GI.ALN_MAX_MD
    d_tasks = torch.full((cap * 48,), SENT, dtype=torch.uint8, device=dev)
    d_job_of = torch.full((span,), -7, dtype=torch.int32, device=dev)
    d_nj = torch.full((2,), -7, dtype=torch.int32, device=dev)
    d_aln = torch.full((cap * 40,), SENT, dtype=torch.uint8, device=dev)
    d_cig = torch.full((cap * max_ops * 4,), SENT, dtype=torch.uint8, device=dev)
    d_md = torch.full((cap * max_md,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    eng.regs_post_device(bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), 3, 0, ppo, st)
    eng.pestat_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_pes.data_ptr(), po, st)
    eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_ooff.data_ptr(),
                           d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(), d_nsw.data_ptr(), po, st)
    eng.mark_primary_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_npri.data_ptr(),
                            d_mstat.data_ptr(), 2 * d.pair_id0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(),
                           d_npri.data_ptr(), d_status.data_ptr(), d_sel.data_ptr(), d_mapq.data_ptr(), d.pair_id0, so, st)
    eng.reg2aln_jobs_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_mapq.data_ptr(),
                            bc.seq_off, cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(), st)
    eng.reg2aln_device(cap, d_tasks.data_ptr(), bc.seq, len(s.seq), d_aln.data_ptr(), d_cig.data_ptr(), d_md.data_ptr(),
                       max_ops, max_md, d_nj.data_ptr(), st)
    stream.synchronize()
    del keep
    # post-processing its own output changes nothing; the statistics; the rescue
    assert np.array_equal(d_n.cpu().numpy().view(np.int32), s.n)
    assert d_regs.cpu().numpy().view(abi.ALNREG_DTYPE).tobytes() == s.regs.tobytes()
    assert d_pes.cpu().numpy().view(abi.PESTAT_DTYPE).tobytes() == s.pes.tobytes()
    assert (d_status.cpu().numpy() == 0).all() and (d_mstat.cpu().numpy() == 0).all()
    got_n = d_out_n.cpu().numpy()
    assert np.array_equal(got_n, s.out_n) and np.array_equal(d_nsw.cpu().numpy(), s.n_sw)
    assert np.array_equal(d_npri.cpu().numpy(), d.n_pri)
    # the selection: final regions, sel, mapq
    final = R.dense(d_out.cpu().numpy().view(abi.ALNREG_DTYPE), out_off[:-1], got_n)
    bad = G.region_mismatch(final, d.final)
    assert bad is None, bad
    sel = d_sel.cpu().numpy().view(abi.PAIRSEL_DTYPE)
    for f in ("status", "branch", "z", "mapq", "alt", "extra_flag", "o", "subo", "n_sub"):
        diff = np.nonzero((sel[f] != d.sel[0][f]).reshape(nr // 2, -1).any(axis=1))[0]
        assert len(diff) == 0, f"sel.{f} differs at pairs {diff[:8].tolist()}"
    assert sel.tobytes() == d.sel[0].tobytes()
    assert np.array_equal(R.dense(d_mapq.cpu().numpy(), out_off[:-1], got_n), d.out_mapq[0])
    # the jobs and the records
    needed = len(jobs)
    assert d_nj.cpu().numpy().tolist() == [needed, needed]
    tasks = d_tasks.cpu().numpy().view(abi.REG2ALN_TASK_DTYPE)
    assert tasks[:needed].tobytes() == jobs.tobytes() and (tasks[needed:].view(np.uint8) == SENT).all()
    want_job_of = np.full(len(d.final), -1, np.int32)
    want_job_of[d.out_mapq[0] >= 0] = np.arange(needed)
    assert np.array_equal(R.dense(d_job_of.cpu().numpy(), out_off[:-1], got_n), want_job_of)
    aln = d_aln.cpu().numpy().view(abi.ALN_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32).reshape(cap, max_ops)
    md = d_md.cpu().numpy().reshape(cap, max_md)
    bad = G.aln_mismatch(jobs, aln[:needed], cig[:needed], md[:needed], exp, ops, mds,
                         fields=("pos", "rid", "is_rev", "n_cigar", "NM", "md_len", "status"))
    assert bad is None, bad
    assert (aln[needed:].view(np.uint8) == SENT).all() and (cig[needed:].view(np.uint8) == SENT).all()
    ok = aln["status"][:needed] == abi.ALN_OK
    rid = aln["rid"][:needed][ok]
    assert ok.sum() > needed // 2 and rid.min() <= 2 and rid.max() >= 198
    g = GI.composite().genome
    assert (aln["pos"][:needed][ok] >= 0).all() and (aln["pos"][:needed][ok] < np.asarray(g["ann_len"])[rid]).all()
