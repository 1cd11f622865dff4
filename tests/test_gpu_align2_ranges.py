"""GPU: the batched ksw_align2 at the reference's SIMD width limits
(tests/align2_cases.py; expected records: tests/golden/align2_range.npz, the
reference's own ksw_align2).

* every "in" side -- the last admitted gap penalties of the 8-bit and 16-bit
  passes, the u8 saturation boundary at four shifts, the 16-bit ceiling, the
  largest value of the segmented scan, the equality cases of XSTOP / XSUBO and
  of the second best's window -- is exact in all seven fields through
  bwagpu_align2_batch and bwagpu_align2_device, with the oracle's cell count;
* every "out" side is refused: bwagpu_align2_batch with E_UNSUPPORTED and its
  reason, leaving the context usable; bwagpu_align2_device answers the refused
  tasks with seven -1 and runs the admitted ones beside them;
* options past the word limit are refused by every entry that reaches the
  kernel (the context itself is created: the other stages do not depend on
  it), and mate rescue refuses gap penalties past the byte limit.
"""
import numpy as np
import pytest

import align2_cases as A
import golden_io as G
import oracle
import rescue_io as R
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine

pytestmark = pytest.mark.gpu

FLAT = A.flat()
IN = [(n, s, f) for n, s, f in FLAT if A.is_in(s)]
OUT = [(n, s, f) for n, s, f in FLAT if not A.is_in(s)]
ids = lambda v: [f"{n}-{s}" for n, s, _ in v]  # noqa: E731
WORD_WHY, BYTE_WHY, SAT_WHY = "_mm_set1_epi16, ksw.c:252-255", "_mm_set1_epi8, ksw.c:132-135", "i16 scores could saturate"

_engines = {}


@pytest.fixture(scope="module")
def gold():
    return G.load_align2_range()


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def engine(opt) -> Engine:
    """one context per option set"""
    key = (tuple(int(opt[k]) for k in G.OPT_KEYS), bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        refd = G.load_ref()
        _engines[key] = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    return _engines[key]


def run_device(eng, tasks, qp, tp):
    """bwagpu_align2_device on torch buffers -> the result records; they start as 0x5a bytes"""
    import torch
    dev = torch.device("cuda:0")
    d_tasks = torch.from_numpy(tasks.view(np.uint8).copy()).to(dev)
    d_q = torch.from_numpy(qp.copy()).to(dev)
    d_t = torch.from_numpy(tp.copy()).to(dev)
    d_out = torch.full((len(tasks) * abi.KSWR_DTYPE.itemsize,), 0x5a, dtype=torch.uint8, device=dev)
    d_scr = torch.zeros(8 * (int(tasks["tlen"].sum()) + len(tasks)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    eng.align2_device(len(tasks), d_tasks.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d_out.data_ptr(),
                      d_scr.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize(dev)
    return d_out.cpu().numpy().view(abi.KSWR_DTYPE)


def refusal(call):
    with pytest.raises(BwaGpuError) as e:
        call()
    assert e.value.code == abi.E_UNSUPPORTED, e.value
    return str(e.value)


@pytest.mark.parametrize("name,side,f", IN, ids=ids(IN))
def test_in_sides_are_exact(gold, name, side, f):
    want = gold[(name, side)][2]
    eng = engine(f.opt)
    got = eng.align2_batch(f.tasks, f.qpool, f.tpool)
    bad = G.kswr_mismatch(f.tasks, got, want)
    assert bad is None, f"{name}-{side} ({f.gate}): {bad}"
    _, cells = oracle.align2("oracle", f.opt, f.tasks, f.qpool, f.tpool)
    assert eng.last_stats()["cells"] == cells[0]
    dev = run_device(eng, f.tasks, f.qpool, f.tpool)
    assert dev.tobytes() == got.tobytes(), G.kswr_mismatch(f.tasks, dev, got)


@pytest.mark.parametrize("name,side,f", OUT, ids=ids(OUT))
def test_out_sides_refuse_the_batch_and_leave_the_context_usable(gold, name, side, f):
    want = gold[(name, side)][2]
    eng = engine(f.opt)
    why = refusal(lambda: eng.align2_batch(f.tasks, f.qpool, f.tpool))
    assert (WORD_WHY if f.opt_refused else SAT_WHY if name == "word-ceiling" else BYTE_WHY) in why, why
    if f.opt_refused:  # no batch is admitted under these options: the refusal repeats, an empty batch passes
        assert WORD_WHY in refusal(lambda: eng.align2_batch(f.tasks[:1], f.qpool, f.tpool))
        assert len(eng.align2_batch(f.tasks[:0], f.qpool, f.tpool)) == 0
        return
    keep = np.nonzero(~f.refused)[0]  # the side's admitted tasks alone, under the same options
    got = eng.align2_batch(f.tasks[keep], f.qpool, f.tpool)
    bad = G.kswr_mismatch(f.tasks[keep], got, want[keep])
    assert bad is None, f"{name}-{side}: admitted tasks after a refusal: {bad}"
    _, cells = oracle.align2("oracle", f.opt, f.tasks[keep], f.qpool, f.tpool)
    assert eng.last_stats()["cells"] == cells[0]


@pytest.mark.parametrize("name,side,f", OUT, ids=ids(OUT))
def test_out_sides_through_the_device_entry(gold, name, side, f):
    want = gold[(name, side)][2]
    eng = engine(f.opt)
    if f.opt_refused:
        assert WORD_WHY in refusal(lambda: run_device(eng, f.tasks, f.qpool, f.tpool))
        return
    # refused and admitted tasks alternate while both last
    no, yes = np.nonzero(f.refused)[0], np.nonzero(~f.refused)[0]
    m = min(len(no), len(yes))
    order = np.concatenate([np.stack([no[:m], yes[:m]], axis=1).reshape(-1), no[m:], yes[m:]])
    assert m >= 1 and sorted(order.tolist()) == list(range(len(f.tasks)))
    tasks, want, refused = f.tasks[order], want[order], f.refused[order]
    got = run_device(eng, tasks, f.qpool, f.tpool)
    assert (got.view(np.int32).reshape(-1, 7)[refused] == -1).all(), "a refused task's record is not seven -1"
    bad = G.kswr_mismatch(tasks[~refused], got[~refused], want[~refused])
    assert bad is None, f"{name}-{side}: admitted tasks beside refused ones: {bad}"


def test_byte_and_word_task_side_by_side_under_o_del_300(gold):
    """the smallest mixed batch: one byte task (refused: seven -1) and one word task (exact)"""
    f = A.families()["byte-mixed"]["out"]
    want = gold[("byte-mixed", "out")][2]
    pick = np.array([np.nonzero(f.refused)[0][0], np.nonzero(~f.refused)[0][0]])
    got = run_device(engine(f.opt), f.tasks[pick], f.qpool, f.tpool)
    assert got.view(np.int32).reshape(-1, 7)[0].tolist() == [-1] * 7
    assert G.kswr_mismatch(f.tasks[pick[1:]], got[1:], want[pick[1:]]) is None


def _rescue_input():
    s = R.load("rep_sw2")  # the smallest rescue fixture; its first 40 reads
    nr = 40
    seq_off, n, off = s.seq_off[:nr + 1], s.n[:nr], s.off[:nr]
    seq, regs = s.seq[:int(seq_off[-1])], s.regs[:int(n.sum())]
    out_off = np.concatenate([[0], np.cumsum(n.astype(np.int64) + 8)]).astype(np.int64)
    return s, seq_off, seq, off, regs, n, out_off


def _rescue_refusals(opt):
    """the refusal texts of bwagpu_mate_rescue and bwagpu_mate_rescue_device under opt, on valid buffers"""
    import torch
    s, seq_off, seq, off, regs, n, out_off = _rescue_input()
    g = s.genome
    eng = Engine(0, dict(s.opt, **opt), g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    try:
        host = refusal(lambda: eng.mate_rescue(s.pes, seq_off, seq, off, regs, n, out_off, s.pairopt()))
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
        d_seq_off, d_seq, d_regs, d_off, d_n, d_ooff, d_pes = (up(seq_off), up(seq), up(regs), up(off), up(n),
                                                               up(out_off), up(s.pes))
        bc = abi.BatchC()
        bc.n_reads, bc.seq_bytes = len(n), int(seq_off[-1])
        bc.seq_off, bc.seq = d_seq_off.data_ptr(), d_seq.data_ptr()
        d_out = torch.zeros(int(out_off[-1]) * 88, dtype=torch.uint8, device=dev)
        d_out_n = torch.zeros(len(n), dtype=torch.int32, device=dev)
        d_status = torch.full((len(n) // 2,), -7, dtype=torch.int32, device=dev)
        d_nsw = torch.full((len(n) // 2,), -7, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream()
        device = refusal(lambda: eng.mate_rescue_device(
            d_pes.data_ptr(), bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_ooff.data_ptr(),
            d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(), d_nsw.data_ptr(), s.pairopt(),
            stream.cuda_stream))
        stream.synchronize()
        assert (d_status.cpu().numpy() == -7).all() and (d_nsw.cpu().numpy() == -7).all()  # nothing ran
        return host, device
    finally:
        eng.close()


def test_mate_rescue_refuses_gap_penalties_past_the_byte_limit():
    for opt in (dict(o_del=300), dict(e_ins=255, o_ins=1)):
        host, device = _rescue_refusals(opt)
        assert "mate rescue" in host and BYTE_WHY in host and "known only on the device" in host, host
        assert host.split(": ", 2)[-1] == device.split(": ", 2)[-1]


def test_word_gate_at_every_entry():
    """o_del + e_del = 65536: the context is created (seeding, extension, CIGARs and pair
    selection do not depend on this limit; bwagpu_create refuses nothing here), and each
    entry that would reach the align2 kernels refuses with the word reason"""
    f = A.families()["word-oe_del"]["out"]
    eng = engine(f.opt)   # creation succeeds
    assert WORD_WHY in refusal(lambda: eng.align2_batch(f.tasks, f.qpool, f.tpool))
    assert WORD_WHY in refusal(lambda: run_device(eng, f.tasks, f.qpool, f.tpool))
    host, device = _rescue_refusals(dict(o_del=65535, e_del=1))
    assert WORD_WHY in host and WORD_WHY in device
    # the pipeline entry (chaining's mem_seed_sw runs ksw_align2 on reads long enough for it)
    g = G.load_chain_gold("long")
    hdr, words = G.load_seed_bwt()
    sa_intv, sa, _, _ = G.load_seed_sa()
    eng.set_bwt(hdr, words, sa, sa_intv)
    seq_off = g["seq_off"][:5]
    assert int(np.diff(seq_off).max()) >= 750  # 5.5 ln(l) <= 0.05 l (bwamem.c:609-611) from about 740 bases on
    why = refusal(lambda: eng.seqs2chains(seq_off, g["seq"][:int(seq_off[-1])], g["seedopt"], g["split_factor"],
                                          g["copt"]))
    assert WORD_WHY in why, why
