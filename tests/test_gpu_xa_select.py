"""GPU tests of bwagpu_xa_select_device (mem_gen_alt's selection on the device)
against the reference's XA fields (tests/golden/xa_select.npz: the hits of every
record mem_sam_pe prints) and against the numpy restatement the fixture's
generator pinned to those fields; and of the device chain mark_primary_device ->
pair_select_device -> xa_select_device -> reg2aln_jobs_device -> reg2aln_device
on one stream, where the XA hits get their CIGARs."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import oracle
import pair_io as P
import rescue_io as R
import xa_io as X
from bwagpu import abi
from bwagpu.engine import Engine

pytestmark = pytest.mark.gpu

SENT = -7


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    d = X.load("rep")
    g = d.genome
    e = Engine(0, d.opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    yield e
    e.close()


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    if b.size == 0:
        b = np.zeros(88, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


def spread(off, regs, n, out_mapq):
    """the same reads with gaps between their spans; a gap's region would join region 0's string
    and have a record if it were read"""
    nr = len(n)
    off2 = (off + 2 * np.arange(nr) + 1).astype(np.int64)
    tot = len(regs) + 2 * nr + 5
    regs2, om2 = np.zeros(tot, abi.ALNREG_DTYPE), np.full(tot, 5, np.int32)
    live = np.zeros(tot, bool)
    for r in range(nr):
        k = int(n[r])
        regs2[off2[r]:off2[r] + k] = regs[off[r]:off[r] + k]
        om2[off2[r]:off2[r] + k] = out_mapq[off[r]:off[r] + k]
        live[off2[r]:off2[r] + k] = True
    return off2, regs2, om2, live


def xa_device(torch, eng, off, regs, n, sel, out_mapq, xopt=None, stream=None, sync=True):
    dev = torch.device("cuda", 0)
    d = [to_dev(torch, x) for x in (off, regs, n, sel, out_mapq)]
    d_xa = torch.full((max(len(regs), 1),), SENT, dtype=torch.int32, device=dev)
    d_job = torch.full((max(len(regs), 1),), SENT, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    eng.xa_select_device(len(n), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                         d_xa.data_ptr(), d_job.data_ptr(), xopt, stream)
    if not sync:
        return d, d_xa, d_job
    torch.cuda.synchronize()
    return d_xa.cpu().numpy()[:len(regs)], d_job.cpu().numpy()[:len(regs)]


def check(torch, eng, off, regs, n, sel, out_mapq, xopt=None):
    """device == restatement on the reads' spans, the sentinel everywhere else -> the device's xa_of, job_select"""
    off2, regs2, om2, live = spread(off, regs, n, out_mapq)
    w_xa, w_job, ev = X.xa_model(off2, regs2, n, sel, om2, xopt)
    xa_of, job = xa_device(torch, eng, off2, regs2, n, sel, om2, xopt)
    assert np.array_equal(xa_of[live], w_xa[live]) and np.array_equal(job[live], w_job[live])
    assert (xa_of[~live] == SENT).all() and (job[~live] == SENT).all()
    return xa_of[live], job[live], ev


@pytest.mark.parametrize("mode", [0, 1], ids=["pairing", "nopairing"])
@pytest.mark.parametrize("name", X.SETS + ["cases"])
def test_selection_against_the_reference_fields(torch, eng, name, mode):
    d = X.load_cases() if name == "cases" else X.load(name)
    assert d.n_reads > 4 and (name == "cases" or (d.n == 0).any())
    xa_of, job, ev = check(torch, eng, d.off, d.regs[mode], d.n, d.sel[mode], d.out_mapq[mode])
    # the hits of every record the reference printed, counted from the device's xa_of
    cnt = np.where(d.out_mapq[mode] >= 0, 0, -1).astype(np.int32)
    for r in range(d.n_reads):
        lo, n = int(d.off[r]), int(d.n[r])
        x = xa_of[lo:lo + n]
        assert ((x >= -1) & (x < n)).all()
        np.add.at(cnt, lo + x[x >= 0], 1)
    assert np.array_equal(cnt, d.xa_cnt[mode])
    assert ev["hits"] == int((xa_of >= 0).sum()) > 0
    assert int((job >= 0).sum()) > int((d.out_mapq[mode] >= 0).sum())  # the hits' jobs come on top


@pytest.mark.parametrize("ratio,mx,mx_alt", [(0.5, 2, 4), (1.0, 0, 0), (0.0, 1 << 30, 1 << 30), (0.8, 5, 4)])
def test_other_options(torch, eng, ratio, mx, mx_alt):
    xo = abi.SamOpt(0, ratio, mx, mx_alt)
    total = 0
    for name, mode in (("rep_sw2", 1), ("ends", 0)):  # repeats; ALT hits
        d = X.load(name)
        xa_of, _, ev = check(torch, eng, d.off, d.regs[mode], d.n, d.sel[mode], d.out_mapq[mode], xo)
        total += ev["hits"]
    assert (total > 0) == (mx > 0)


def test_hostile_and_large_inputs(torch, eng):
    """what the fixture's pairs do not hold: a pair that was not selected, the no-pairing mate record on
    a region without a record, secondary_all outside the read, and reads of many regions"""
    d = X.load("rep")
    mode = 1
    regs, sel, om = d.regs[mode].copy(), d.sel[mode].copy(), d.out_mapq[mode].copy()
    xa0, job0, _ = X.xa_model(d.off, regs, d.n, sel, om)
    assert (sel["status"] == abi.SEL_DONE).all() and (sel["branch"] == abi.SEL_NO_PAIRING).all()
    # pairs with strings that are not selected
    with_xa = sorted({r >> 1 for r in range(d.n_reads) if (xa0[d.off[r]:d.off[r] + d.n[r]] >= 0).any()})
    assert len(with_xa) > 10
    sel["status"][with_xa[0]] = abi.SEL_SKIPPED
    sel["status"][with_xa[1]] = abi.SEL_TOO_MANY
    # mate records on regions that need no CIGAR otherwise
    moved = 0
    for r in range(d.n_reads):
        lo, n = int(d.off[r]), int(d.n[r])
        idle = np.nonzero(job0[lo:lo + n] < 0)[0]
        if len(idle) and (r >> 1) not in with_xa[:2] and moved < 20:
            sel["z"][r >> 1][r & 1] = idle[-1]
            moved += 1
    assert moved == 20
    # secondary_all outside the read: hits of with_xa[2]'s first read
    r = 2 * with_xa[2] + (0 if (xa0[d.off[2 * with_xa[2]]:][:d.n[2 * with_xa[2]]] >= 0).any() else 1)
    hits = d.off[r] + np.nonzero(xa0[d.off[r]:d.off[r] + d.n[r]] >= 0)[0]
    regs["secondary_all"][hits[0]] = d.n[r]
    if len(hits) > 1:
        regs["secondary_all"][hits[1]] = 0x7fffffff
    xa_of, job, ev = check(torch, eng, d.off, regs, d.n, sel, om)
    lo = int(d.off[2 * with_xa[0]])
    assert (xa_of[lo:lo + int(d.n[2 * with_xa[0]])] == -1).all() and (job[lo:lo + int(d.n[2 * with_xa[0]])] == -1).all()
    assert xa_of[hits[0]] == -1 and int((job >= 0).sum()) >= int((job0 >= 0).sum()) - 40 + moved
    # reads of 64, 65, 300 and 1500 regions: region 0 and 1 are records, every other region is a
    # hit of one of them or of nothing, some of them ALT
    rng = np.random.default_rng(5)
    ns = np.array([64, 0, 65, 1, 300, 2, 1500, 3], np.int32)
    off = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    big = np.zeros(int(ns.sum()), abi.ALNREG_DTYPE)
    big["secondary_all"] = -1
    bom = np.full(len(big), -1, np.int32)
    for r in range(len(ns)):
        lo, n = int(off[r]), int(ns[r])
        if n == 0:
            continue
        big["score"][lo:lo + n] = rng.integers(60, 151, n)
        big["score"][lo:lo + min(n, 2)] = 150
        bom[lo:lo + min(n, 2)] = 60
        if n > 2:
            big["secondary_all"][lo + 2:lo + n] = rng.integers(-1, 2, n - 2)
            big["n_comp_is_alt"][lo + 2:lo + n] = (rng.integers(0, 50, n - 2) == 0).astype(np.uint32) << np.uint32(30)
    bsel = np.zeros(len(ns) // 2, abi.PAIRSEL_DTYPE)
    bsel["branch"] = abi.SEL_PAIRED
    for xo in (abi.SamOpt(0, 0.8, 5, 200), abi.SamOpt(0, 0.8, 1000, 2000), abi.SamOpt(0, 0.5, 100, 100)):
        _, _, ev = check(torch, eng, off, big, ns, bsel, bom, xo)
    assert ev["hits"] > 100 and ev["strings_over_cap"] > 0


def test_two_calls_on_two_streams(torch, eng):
    a, b = X.load("rep"), X.load("mixed")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    keep1, xa1, job1 = xa_device(torch, eng, a.off, a.regs[0], a.n, a.sel[0], a.out_mapq[0], None, s1.cuda_stream, False)
    keep2, xa2, job2 = xa_device(torch, eng, b.off, b.regs[1], b.n, b.sel[1], b.out_mapq[1], None, s2.cuda_stream, False)
    s1.synchronize()
    s2.synchronize()
    for d, mode, xa, job in ((a, 0, xa1, job1), (b, 1, xa2, job2)):
        w_xa, w_job, _ = X.xa_model(d.off, d.regs[mode], d.n, d.sel[mode], d.out_mapq[mode])
        assert np.array_equal(xa.cpu().numpy(), w_xa) and np.array_equal(job.cpu().numpy(), w_job)


def test_chain_to_the_hits_cigars_on_one_stream(torch):
    """no host copy between the stages: the selection's job_select feeds the job builder in the place of out_mapq"""
    d, s, xd = P.load("ends"), R.load("ends"), X.load("ends")
    g = d.genome
    eng = Engine(0, d.opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    eng.set_alt(d.alt)
    eng.set_regs_post(0)
    so = d.selopt()
    dev = torch.device("cuda", 0)
    nr, n_regs = d.n_reads, len(d.regs)
    d_pes, d_off, d_regs, d_n = to_dev(torch, d.pes), to_dev(torch, d.off), to_dev(torch, d.regs), to_dev(torch, d.n)
    d_seq_off, d_seq = to_dev(torch, s.seq_off), to_dev(torch, s.seq)
    i32 = lambda k: torch.full((k,), SENT, dtype=torch.int32, device=dev)  # noqa: E731
    d_npri, d_mstat, d_mapq, d_xa, d_jsel, d_job_of, d_nj = i32(nr), i32(nr), i32(n_regs), i32(n_regs), i32(n_regs), \
        i32(n_regs), i32(2)
    d_sel = torch.full((nr // 2 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    cap, max_ops, max_md = n_regs, 64, 512
    d_tasks = torch.full((cap * 48,), 0xA5, dtype=torch.uint8, device=dev)
    d_out = torch.full((cap * 40,), 0xA5, dtype=torch.uint8, device=dev)
    d_cig = torch.full((cap * max_ops * 4,), 0xA5, dtype=torch.uint8, device=dev)
    d_md = torch.full((cap * max_md,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    eng.mark_primary_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_npri.data_ptr(),
                            d_mstat.data_ptr(), 2 * d.pair_id0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(),
                           d_npri.data_ptr(), None, d_sel.data_ptr(), d_mapq.data_ptr(), d.pair_id0, so, st)
    eng.xa_select_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_sel.data_ptr(), d_mapq.data_ptr(),
                         d_xa.data_ptr(), d_jsel.data_ptr(), None, st)
    eng.reg2aln_jobs_device(nr, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_jsel.data_ptr(),
                            d_seq_off.data_ptr(), cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(), st)
    eng.reg2aln_device(cap, d_tasks.data_ptr(), d_seq.data_ptr(), len(s.seq), d_out.data_ptr(), d_cig.data_ptr(),
                       d_md.data_ptr(), max_ops, max_md, d_nj.data_ptr(), st)
    stream.synchronize()
    w_xa, w_job, _ = X.xa_model(d.off, d.final, d.n, d.sel[0], d.out_mapq[0])
    assert np.array_equal(d_xa.cpu().numpy(), w_xa) and np.array_equal(d_jsel.cpu().numpy(), w_job)
    # the jobs, in (read, k) order, and the hits' CIGARs through the oracle
    sel_idx = np.concatenate([d.off[r] + np.nonzero(w_job[d.off[r]:d.off[r] + d.n[r]] >= 0)[0] for r in range(nr)])
    needed = len(sel_idx)
    assert int((d.out_mapq[0] >= 0).sum()) < needed < cap and d_nj.cpu().numpy().tolist() == [needed, needed]
    job_of = d_job_of.cpu().numpy()
    assert np.array_equal(job_of[sel_idx], np.arange(needed)) and int((job_of >= 0).sum()) == needed
    read_of = np.repeat(np.arange(nr), d.n)
    w_tasks = np.zeros(needed, abi.REG2ALN_TASK_DTYPE)
    for f in ("rb", "re", "qb", "qe", "truesc", "w"):
        w_tasks[f] = d.final[f][sel_idx]
    w_tasks["qoff"] = s.seq_off[read_of[sel_idx]]
    w_tasks["l_seq"] = (s.seq_off[1:] - s.seq_off[:-1])[read_of[sel_idx]]
    assert d_tasks.cpu().numpy().view(abi.REG2ALN_TASK_DTYPE)[:needed].tobytes() == w_tasks.tobytes()
    ref = oracle.Ref(g["l_pac"], g["ann_offset"], g["ann_len"], g["pac"])
    want, wc, wm = oracle.reg2aln("oracle", d.opt, ref, w_tasks, s.seq, max_ops, max_md)
    out = d_out.cpu().numpy().view(abi.ALN_DTYPE)
    cig = d_cig.cpu().numpy().view(np.uint32).reshape(cap, max_ops)
    md = d_md.cpu().numpy().reshape(cap, max_md)
    assert G.aln_mismatch(w_tasks, out[:needed], cig[:needed], md[:needed], *G.aln_expected_from(want, wc, wm)) is None
    hit_jobs = job_of[w_xa >= 0]
    assert len(hit_jobs) == int(xd.xa_cnt[0][xd.xa_cnt[0] > 0].sum()) and (want["status"][hit_jobs] == abi.ALN_OK).all()
    eng.close()


def test_argument_errors(torch, eng):
    lib = abi.load()
    p = C.c_void_p(to_dev(torch, np.zeros(64, np.int64)).data_ptr())
    xo = abi.default_samopt()

    def call(opt=xo, n=2, a=(p,) * 7, ctx=eng.ctx):
        return lib.bwagpu_xa_select_device(ctx, C.byref(opt) if opt is not None else None, n, *a, None)

    assert call(ctx=None) == abi.E_INVAL and call(opt=None) == abi.E_INVAL
    assert call(n=-2) == abi.E_INVAL and call(n=3) == abi.E_INVAL
    for k in range(7):
        assert call(a=tuple(None if j == k else p for j in range(7))) == abi.E_INVAL, k
    for f in (abi.MEM_F_ALL, abi.MEM_F_NO_MULTI, abi.MEM_F_PRIMARY5, abi.MEM_F_KEEP_SUPP_MAPQ):
        assert call(opt=abi.default_samopt(f)) == abi.E_UNSUPPORTED, f
    assert b"MEM_F_ALL" in lib.bwagpu_last_error(eng.ctx)
    assert call(opt=abi.default_samopt(abi.MEM_F_NOPAIRING | 0x200 | 0x2000)) == abi.OK  # n = 0 regions per read
    assert call(n=0, a=(None,) * 7) == abi.OK
    torch.cuda.synchronize()
