"""GPU parity of bwagpu_reg2aln_device: the CIGAR kernel on jobs, pool and
outputs in device memory (device-side classification and binning, one
read-back of the bin table).  Against the reference's own outputs (the golden
sets), against bwagpu_reg2aln_batch on the same context, and against the
oracle on the edge jobs; the per-job refusals, the job count on the device and
two calls on two streams.  Every output buffer is pre-filled with a sentinel
byte, so an unwritten record and a touched slot of a refused job both show."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import oracle
from bwagpu import abi
from cigar_helpers import DevCall, engine, run_device, same_as, untouched, zb_class

pytestmark = pytest.mark.gpu

SCORING = dict(a=2, b=5, o_del=7, e_del=2, o_ins=5, e_ins=3, pen_clip5=3, pen_clip3=9, w=30, zdrop=40,
               mat=abi.fill_scmat(2, 5))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def refd():
    return G.load_ref()


@pytest.fixture(scope="module")
def R(refd):
    return oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])


@pytest.fixture(scope="module")
def synth(refd):
    """per scoring: the two synthetic job sets of test_gpu_cigar.py in one list, made once"""
    made = {}

    def get(optname):
        if optname not in made:
            opt = abi.default_opt() if optname == "default" else SCORING
            parts, pools, qo = [], [], 0
            for lens, n in [((100, 150, 250), 700), ((400, 700, 1000), 120)]:
                rng = np.random.default_rng(41 + len(lens) + n)
                t, q = G.synth_reg2aln_jobs(rng, refd["pac"], int(refd["l_pac"]), refd["ann_offset"], refd["ann_len"], n,
                                            lens=lens, mat=opt["mat"])
                t = t.copy()
                t["qoff"] += qo
                qo += len(q)
                parts.append(t)
                pools.append(q)
            made[optname] = (opt, np.concatenate(parts), np.concatenate(pools))
        return made[optname]
    return get


@pytest.mark.parametrize("name", G.CIGAR_SETS)
def test_golden_sets_bit_exact(torch, refd, name):
    opt, tasks, qpool, exp, ops, mds = G.load_cigar_set(name)
    eng = engine(refd, opt)
    out, cig, md = run_device(torch, eng, tasks, qpool, 64, 512)
    assert G.aln_mismatch(tasks, out, cig, md, exp, ops, mds) is None
    st = eng.last_stats()
    assert st["h2d_bytes"] == 0 and st["d2h_bytes"] == 0 and st["kernel_ms"] == 0 and st["ext_calls"] == len(tasks)
    assert (out["status"] != abi.ALN_REFUSED).all()
    eng.close()


@pytest.mark.parametrize("optname", ["default", "scoring"])
def test_same_context_both_forms(torch, refd, synth, optname):
    opt, tasks, qpool = synth(optname)
    l_pac = int(refd["l_pac"])
    where = {zb_class(opt, l_pac, t) for t in tasks}
    assert len({b for b, _ in where}) >= 5 and {c for _, c in where} == {0, 1, 2}, sorted(where)
    eng = engine(refd, opt)
    want = eng.reg2aln_batch(tasks, qpool, 256, 2048)
    got = run_device(torch, eng, tasks, qpool, 256, 2048)
    assert same_as(tasks, got, want) is None
    assert (want[0]["status"] == abi.ALN_OK).sum() > len(tasks) // 2
    # and the batch form after it, on the same context: the two share no scratch
    again = eng.reg2aln_batch(tasks, qpool, 256, 2048)
    assert same_as(tasks, again, want) is None
    eng.close()


def test_edge_jobs(torch, refd, R):
    """the jobs of test_reg2aln_edge_jobs: unmapped, strand-spanning, past the end, empty query range,
    the ungapped shortcut, and capacity overflow"""
    opt = abi.default_opt()
    rng = np.random.default_rng(9)
    tasks, qpool = G.synth_reg2aln_jobs(rng, refd["pac"], int(refd["l_pac"]), refd["ann_offset"], refd["ann_len"], 40)
    l_pac = int(refd["l_pac"])
    t = tasks.copy()
    t[0]["rb"], t[0]["re"] = -1, -1
    t[1]["rb"], t[1]["re"] = l_pac - 50, l_pac + 50
    t[2]["rb"], t[2]["re"] = 2 * l_pac - 10, 2 * l_pac + 40
    t[3]["qe"] = t[3]["qb"]
    for k in range(4, 10):
        t[k]["re"] = t[k]["rb"] + (t[k]["qe"] - t[k]["qb"])
        t[k]["truesc"] = 0
    eng = engine(refd, opt)
    for max_ops, max_md in [(64, 512), (3, 8)]:
        out, cig, md = run_device(torch, eng, t, qpool, max_ops, max_md)
        want, wc, wm = oracle.reg2aln("oracle", opt, R, t, qpool, max_ops, max_md)
        assert G.aln_mismatch(t, out, cig, md, *G.aln_expected_from(want, wc, wm)) is None
        assert out["status"][0] == abi.ALN_UNMAPPED and (out["status"][1:4] == abi.ALN_NO_CIGAR).all()
    assert (out["status"][4:] == abi.ALN_OVERFLOW).any()
    eng.close()


def test_refusals(torch, refd):
    """one job per refusal reason between good jobs; the limits themselves are accepted"""
    opt = abi.default_opt()
    rng = np.random.default_rng(17)
    good, qpool = G.synth_reg2aln_jobs(rng, refd["pac"], int(refd["l_pac"]), refd["ann_offset"], refd["ann_len"], 16)
    qpool = np.concatenate([qpool, rng.integers(0, 4, 1200).astype(np.uint8)])
    base = good[0].copy()
    base["rb"], base["qb"] = 1000, 0
    base["qe"] = base["l_seq"]
    base["re"] = 1000 + int(base["l_seq"])
    base["truesc"], base["w"] = int(base["l_seq"]) - 10, 100

    def job(**kw):
        t = base.copy()
        for f, v in kw.items():
            t[f] = v
        return t
    imin = -(1 << 31)
    refused = [
        job(qoff=len(qpool) - int(base["l_seq"]) + 1),          # read outside the pool
        job(qoff=-1),
        job(qb=-1),
        job(qe=int(base["l_seq"]) + 1),
        job(qoff=0, l_seq=1100, qb=0, qe=1024, re=1000 + 1024),  # qe - qb = 1024
        job(qb=0, qe=2, re=1000 + 8193),                        # re - rb = 8193
        job(truesc=(1 << 24) + 1), job(truesc=-(1 << 24) - 1), job(truesc=imin),
        job(w=-1), job(w=(1 << 24) + 1),
    ]
    # re - rb = 8192 fits a workgroup's LDS only in the one-wave class (a matrix of 8-24 KB: a 2 or 3 bp query)
    limits = [
        job(qb=0, qe=2, re=1000 + 8192),
        job(qoff=0, l_seq=1023, qb=0, qe=1023, re=1000 + 1023),
        job(truesc=1 << 24), job(truesc=-(1 << 24)), job(w=0), job(w=1 << 24),
    ]
    tasks, kind = [good[0]], ["good"]
    for k, e in enumerate(refused + limits):
        tasks += [e, good[(k + 1) % len(good)]]
        kind += ["refused" if k < len(refused) else "limit", "good"]
    tasks = np.array(tasks, abi.REG2ALN_TASK_DTYPE)
    is_ref, is_lim = np.array(kind) == "refused", np.array(kind) == "limit"
    eng = engine(refd, opt)
    want = eng.reg2aln_batch(tasks[~is_ref], qpool, 64, 512)
    out, cig, md = run_device(torch, eng, tasks, qpool, 64, 512)
    st = eng.last_stats()
    assert st["ext_calls"] == len(tasks) and (out["status"] == abi.ALN_REFUSED).sum() == len(refused)
    for k in np.nonzero(is_ref)[0]:
        r = out[k]
        assert (r["status"], r["rid"], r["pos"], r["n_cigar"], r["md_len"]) == (abi.ALN_REFUSED, -1, -1, 0, 0), (k, r)
        assert untouched(cig[k]) and untouched(md[k]), k
    assert same_as(tasks[~is_ref], (out[~is_ref], cig[~is_ref], md[~is_ref]), want) is None
    assert (out["status"][is_lim] != abi.ALN_REFUSED).all() and (out["status"][is_lim] == abi.ALN_OK).any()
    eng.close()


def test_count_on_the_device(torch, refd, synth):
    opt, tasks, qpool = synth("default")
    tasks = tasks[:300]
    eng = engine(refd, opt)
    want = eng.reg2aln_batch(tasks, qpool, 64, 512)
    for n in (0, 1, 65, 300):
        out, cig, md = run_device(torch, eng, tasks, qpool, 64, 512, n_cap=300, n_on_device=n)
        assert same_as(tasks[:n], (out[:n], cig[:n], md[:n]), tuple(a[:n] for a in want)) is None, n
        assert untouched(out[n:]) and untouched(cig[n:]) and untouched(md[n:]), n
        assert eng.last_stats()["ext_calls"] == n
    # a count over the capacity is the capacity
    out, cig, md = run_device(torch, eng, tasks, qpool, 64, 512, n_cap=100, n_on_device=5000)
    assert same_as(tasks[:100], (out, cig, md), tuple(a[:100] for a in want)) is None
    c = DevCall(torch, eng, tasks, qpool, 64, 512, n_cap=0)
    torch.cuda.synchronize()
    assert untouched(c.d_out.cpu().numpy()) and untouched(c.d_cig.cpu().numpy())
    eng.close()


def test_two_streams_back_to_back(torch, refd, synth):
    """two calls on two streams with nothing between them: everything is uploaded and pre-filled first,
    then the calls alone.  The first has the long reads (the HBM class, its slowest bins) and is still
    running when the second one's stream reaches the shared scratch, which only the context's event
    keeps it from zeroing; the third call, on the first stream again, meets the second the same way."""
    opt, tasks, qpool = synth("default")
    a, b = tasks[300:], tasks[:500]
    eng = engine(refd, opt)
    want_a = eng.reg2aln_batch(a, qpool, 64, 512)
    want_b = eng.reg2aln_batch(b, qpool, 64, 512)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ca = DevCall(torch, eng, a, qpool, 64, 512, stream=s1.cuda_stream, launch=False)
    cb = DevCall(torch, eng, b, qpool, 64, 512, stream=s2.cuda_stream, launch=False)
    cc = DevCall(torch, eng, a, qpool, 64, 512, stream=s1.cuda_stream, launch=False)
    ca.launch()
    cb.launch()
    cc.launch()
    s1.synchronize()
    s2.synchronize()
    assert same_as(a, ca.results(), want_a) is None
    assert same_as(b, cb.results(), want_b) is None
    assert same_as(a, cc.results(), want_a) is None
    eng.close()


def test_argument_errors_launch_nothing(torch, refd):
    eng = engine(refd, abi.default_opt())
    lib, vp = eng.lib, C.c_void_p
    buf = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", 0))
    p = vp(buf.data_ptr())

    def call(n_cap=1, tasks=p, q=p, qlen=10, max_ops=4, max_md=8, out=p, cig=p, md=p):
        return lib.bwagpu_reg2aln_device(eng.ctx, n_cap, None, tasks, q, qlen, max_ops, max_md, out, cig, md, None)
    for kw in (dict(n_cap=-1), dict(tasks=None), dict(q=None), dict(out=None), dict(cig=None), dict(md=None),
               dict(max_ops=0), dict(max_md=0), dict(qlen=-1)):
        assert call(**kw) == abi.E_INVAL, kw
    assert call(n_cap=0, tasks=None, q=None, out=None, cig=None, md=None) == 0
    assert lib.bwagpu_reg2aln_jobs_device(eng.ctx, -1, p, p, p, p, p, 1, p, p, p, None) == abi.E_INVAL
    assert lib.bwagpu_reg2aln_jobs_device(eng.ctx, 1, p, p, p, p, p, 1, p, p, None, None) == abi.E_INVAL
    assert lib.bwagpu_reg2aln_jobs_device(eng.ctx, 1, None, p, p, p, p, 1, p, p, p, None) == abi.E_INVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0).all()
    eng.close()
