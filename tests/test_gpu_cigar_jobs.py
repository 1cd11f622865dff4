"""GPU tests of bwagpu_reg2aln_jobs_device (the CIGAR jobs of a selection over
device-resident regions) against a numpy construction, and of the device chain
mark_primary_device -> pair_select_device -> reg2aln_jobs_device ->
reg2aln_device on one stream against the oracle's mem_reg2aln on jobs built in
numpy from the fixture's final regions and out_mapq."""
import numpy as np
import pytest

import golden_io as G
import oracle
import pair_io as P
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import Engine

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def engine(d) -> Engine:
    g = d.genome
    e = Engine(0, d.opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e.set_alt(d.alt)
    e.set_regs_post(0)
    return e


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    if b.size == 0:
        b = np.zeros(88, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


def jobs_numpy(off, regs, n, select, seq_off, job_cap):
    """-> tasks[min(needed, job_cap)], job_of (parallel to regs; -1), needed"""
    tasks, job_of = [], np.full(len(regs), -1, np.int32)
    for r in range(len(n)):
        for k in range(int(n[r])):
            i = int(off[r]) + k
            if select[i] < 0:
                continue
            g = regs[i]
            if len(tasks) < job_cap:
                job_of[i] = len(tasks)
            tasks.append((g["rb"], g["re"], seq_off[r], seq_off[r + 1] - seq_off[r], g["qb"], g["qe"], g["truesc"],
                          g["w"], 0))
    return np.array(tasks[:job_cap], abi.REG2ALN_TASK_DTYPE).reshape(-1), job_of, len(tasks)


def jobs_device(torch, eng, off, regs, n, select, seq_off, job_cap, stream=None):
    dev = torch.device("cuda", 0)
    d = [to_dev(torch, x) for x in (off, regs, n, select, seq_off)]
    d_tasks = torch.full((max(job_cap, 1) * 48,), SENT, dtype=torch.uint8, device=dev)
    d_job_of = torch.full((max(len(regs), 1),), -7, dtype=torch.int32, device=dev)
    d_nj = torch.full((2,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.reg2aln_jobs_device(len(n), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                            d[4].data_ptr(), job_cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(), stream)
    torch.cuda.synchronize()
    return (d_tasks.cpu().numpy().view(abi.REG2ALN_TASK_DTYPE)[:job_cap], d_job_of.cpu().numpy()[:len(regs)],
            d_nj.cpu().numpy())


@pytest.mark.parametrize("mode", [0, 1], ids=["pairing", "nopairing"])
@pytest.mark.parametrize("name", ["rep_sw2", "rep"])  # the two smallest pair sets
def test_builder_against_numpy(torch, name, mode):
    d, s = P.load(name), R.load(name)
    regs = d.final if mode == 0 else d.marked
    select = d.out_mapq[mode]
    assert (d.n == 0).any() and len(s.seq_off) == d.n_reads + 1
    eng = engine(d)
    _, _, needed = jobs_numpy(d.off, regs, d.n, select, s.seq_off, 1 << 30)
    assert needed == int((select >= 0).sum()) > 0
    for cap in (needed, needed + 5, needed - 1, 0):
        w_tasks, w_job_of, _ = jobs_numpy(d.off, regs, d.n, select, s.seq_off, cap)
        tasks, job_of, nj = jobs_device(torch, eng, d.off, regs, d.n, select, s.seq_off, cap)
        assert nj.tolist() == [min(cap, needed), needed], cap
        assert tasks[:min(cap, needed)].tobytes() == w_tasks.tobytes(), cap
        assert (tasks[min(cap, needed):].view(np.uint8) == SENT).all(), cap
        assert np.array_equal(job_of, w_job_of), cap
    # more reads than one workgroup scans, with gaps between the spans: the same reads four times over
    nr = d.n_reads
    off4 = np.concatenate([d.off + k * (len(regs) + 3) for k in range(4)])
    regs4 = np.zeros(4 * (len(regs) + 3), abi.ALNREG_DTYPE)
    sel4 = np.full(len(regs4), 5, np.int32)  # a gap's entry would be selected if it were read
    for k in range(4):
        lo = k * (len(regs) + 3)
        regs4[lo:lo + len(regs)] = regs
        sel4[lo:lo + len(regs)] = select
    n4 = np.tile(d.n, 4)
    so4 = np.concatenate([s.seq_off[:-1] + k * int(s.seq_off[-1]) for k in range(4)] + [[4 * int(s.seq_off[-1])]])
    w_tasks, w_job_of, need4 = jobs_numpy(off4, regs4, n4, sel4, so4, 1 << 30)
    assert need4 == 4 * needed and 4 * nr > 256
    tasks, job_of, nj = jobs_device(torch, eng, off4, regs4, n4, sel4, so4, need4)
    live = np.zeros(len(regs4), bool)
    for r in range(len(n4)):
        live[off4[r]:off4[r] + n4[r]] = True
    assert nj.tolist() == [need4, need4] and tasks.tobytes() == w_tasks.tobytes()
    assert np.array_equal(job_of[live], w_job_of[live]) and (job_of[~live] == -7).all()
    # no reads at all
    _, _, nj = jobs_device(torch, eng, off4[:0], regs4, n4[:0], sel4, so4[:1], 10)
    assert nj.tolist() == [0, 0]
    eng.close()


def test_chain_to_cigars_on_one_stream(torch):
    """no host copy of the regions between the stages; the job count stays on the device"""
    d, s = P.load("ends"), R.load("ends")
    eng = engine(d)
    so = d.selopt()
    dev = torch.device("cuda", 0)
    nr, n_regs = d.n_reads, len(d.regs)
    d_pes, d_off, d_regs, d_n = to_dev(torch, d.pes), to_dev(torch, d.off), to_dev(torch, d.regs), to_dev(torch, d.n)
    d_seq_off, d_seq = to_dev(torch, s.seq_off), to_dev(torch, s.seq)
    d_npri = torch.full((nr,), -7, dtype=torch.int32, device=dev)
    d_mstat = torch.full((nr,), -7, dtype=torch.int32, device=dev)
    d_sel = torch.full((nr // 2 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_mapq = torch.full((n_regs,), -7, dtype=torch.int32, device=dev)
    cap, max_ops, max_md = n_regs, 64, 512
    d_tasks = torch.full((cap * 48,), SENT, dtype=torch.uint8, device=dev)
    d_job_of = torch.full((n_regs,), -7, dtype=torch.int32, device=dev)
    d_nj = torch.full((2,), -7, dtype=torch.int32, device=dev)
    d_out = torch.full((cap * 40,), SENT, dtype=torch.uint8, device=dev)
    d_cig = torch.full((cap * max_ops * 4,), SENT, dtype=torch.uint8, device=dev)
    d_md = torch.full((cap * max_md,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    eng.mark_primary_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_npri.data_ptr(),
                            d_mstat.data_ptr(), 2 * d.pair_id0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(),
                           d_npri.data_ptr(), None, d_sel.data_ptr(), d_mapq.data_ptr(), d.pair_id0, so, st)
    eng.reg2aln_jobs_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_mapq.data_ptr(),
                            d_seq_off.data_ptr(), cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(), st)
    eng.reg2aln_device(cap, d_tasks.data_ptr(), d_seq.data_ptr(), len(s.seq), d_out.data_ptr(), d_cig.data_ptr(),
                       d_md.data_ptr(), max_ops, max_md, d_nj.data_ptr(), st)
    stream.synchronize()
    # the same jobs in numpy from the fixture, through the oracle
    w_tasks, w_job_of, needed = jobs_numpy(d.off, d.final, d.n, d.out_mapq[0], s.seq_off, cap)
    assert 0 < needed < cap and d_nj.cpu().numpy().tolist() == [needed, needed]
    assert d_tasks.cpu().numpy().view(abi.REG2ALN_TASK_DTYPE)[:needed].tobytes() == w_tasks.tobytes()
    assert np.array_equal(d_job_of.cpu().numpy(), w_job_of)
    g = d.genome
    ref = oracle.Ref(g["l_pac"], g["ann_offset"], g["ann_len"], g["pac"])
    want, wc, wm = oracle.reg2aln("oracle", d.opt, ref, w_tasks, s.seq, max_ops, max_md)
    out = d_out.cpu().numpy().view(abi.ALN_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32).reshape(cap, max_ops)
    md = d_md.cpu().numpy().reshape(cap, max_md)
    assert G.aln_mismatch(w_tasks, out[:needed], cig[:needed], md[:needed], *G.aln_expected_from(want, wc, wm)) is None
    assert (want["status"] == abi.ALN_OK).sum() > needed // 2
    assert (out[needed:].view(np.uint8) == SENT).all() and (cig[needed:].view(np.uint8) == SENT).all()
    assert (md[needed:] == SENT).all()
    eng.close()
