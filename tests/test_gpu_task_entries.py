"""The four blocking entries that take a task list or a wire stream
(bwa-flow_amd/csrc/capi_tasks.hip: bwagpu_extend_batch, bwagpu_align2_batch,
bwagpu_reg2aln_batch, bwagpu_sw_stream) on ONE context: against each other in
both orders, extend_batch's context-owned buffers growing, a call refused in
validation between two good ones, and after every good call the byte counts of
last_stats in the closed forms of include/bwagpu.h with kernel_ms > 0.
Results are the golden values (the reference's own outputs; for the stream,
the oracle that tests/test_fpga_stream_oracle.py pins to them)."""
import numpy as np
import pytest

import golden_io as G
import oracle
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine
from test_fpga_stream_oracle import sub_batch

pytestmark = pytest.mark.gpu

K = 256            # tasks per call; the stream is 60 reads' records (735 extension tasks)
OPS, MD = 64, 512  # reg2aln output capacities per job


class Entries:
    """the inputs, golden outputs and one context; every good call is checked in full"""

    def __init__(self):
        refd = G.load_ref()
        opt, self.ct, self.cq, self.cexp, self.cops, self.cmds = G.load_cigar_set("cigar_c1_default")
        eopt, self.et, self.ewant, self.eq, self.etp = G.load_tasks("ksw_edge_default")
        aopt, self.at, self.awant, self.aq, self.atp = G.load_align2("align2_default")
        sopt, batch, _, _ = G.load_chain_set("c1_default")
        for o in (eopt, aopt, sopt):  # one context serves all four: the sets share their options
            assert all(np.array_equal(o[k], opt[k]) for k in opt)
        r = oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])
        self.words, self.nt, _, _ = oracle.fpga_pack(opt, r, sub_batch(batch, 0, 60))
        self.swant = oracle.fpga_sw(opt, r, self.words, self.nt)
        assert self.nt > 0
        self.eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])

    def stats(self, h2d, d2h):
        st = self.eng.last_stats()
        assert (st["h2d_bytes"], st["d2h_bytes"]) == (h2d, d2h)
        assert st["kernel_ms"] > 0
        return st

    def extend(self, k=K):
        t = self.et[:k]
        got = self.eng.extend_batch(t, self.eq, self.etp)
        g, w = got.view(np.int32).reshape(-1, 6), self.ewant[:len(t)].view(np.int32).reshape(-1, 6)
        assert np.array_equal(g, w), f"{int((g != w).any(axis=1).sum())} extend tasks differ"
        self.stats(abi.EXT_TASK_DTYPE.itemsize * len(t) + len(self.eq) + len(self.etp),
                   abi.EXT_RES_DTYPE.itemsize * len(t))
        return got

    def align2(self, k=K):
        t = self.at[:k]
        got = self.eng.align2_batch(t, self.aq, self.atp)
        assert G.kswr_mismatch(t, got, self.awant[:len(t)]) is None
        self.stats(abi.ALIGN2_TASK_DTYPE.itemsize * len(t) + len(self.aq) + len(self.atp),
                   abi.KSWR_DTYPE.itemsize * len(t))
        return got

    def reg2aln(self, k=K):
        t = self.ct[:k]
        n = len(t)
        out, cig, md = self.eng.reg2aln_batch(t, self.cq, OPS, MD)
        assert G.aln_mismatch(t, out, cig, md, self.cexp[:n], self.cops[:n], self.cmds[:n]) is None
        st = self.stats(abi.REG2ALN_TASK_DTYPE.itemsize * n + len(self.cq),
                        abi.ALN_DTYPE.itemsize * n + 4 * n * OPS + n * MD)
        assert st["ext_calls"] == n
        return out, cig, md

    def sw_stream(self):
        w = self.words
        got = self.eng.sw_stream(w, self.nt)
        assert got.shape == self.swant.shape and np.array_equal(got, self.swant)
        self.stats(4 * len(w), 20 * self.nt)
        return got


@pytest.fixture(scope="module")
def E():
    e = Entries()
    yield e
    e.eng.close()


def test_extend_batch_buffers_grow_and_are_reused(E):
    """the context's first extend_batch calls (this test runs first): the buffers reserved for 8 tasks
    (4 KiB at least, so 102 tasks' worth) are freed and reallocated for 256, then reused for 8"""
    assert E.eng.last_stats()["ext_calls"] == 0 and E.eng.last_stats()["kernel_ms"] == 0  # nothing has run yet
    for k in (8, K, 8):
        E.extend(k)


def test_the_four_entries_in_both_orders(E):
    order = [E.extend, E.align2, E.reg2aln, E.sw_stream]
    for call in order + order[::-1]:
        call()


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("entry", ["extend", "align2", "reg2aln", "sw_stream"])
def test_a_refused_call_between_two_good_ones(E, entry):
    call = getattr(E, entry)
    first = call()
    with pytest.raises(BwaGpuError) as ei:
        if entry == "extend":
            bad = E.et[:K].copy()
            bad["qoff"][K // 2] = len(E.eq) + 1  # a task outside its query pool
            E.eng.extend_batch(bad, E.eq, E.etp)
        elif entry == "align2":
            bad = E.at[:K].copy()
            bad["toff"][K // 2] = len(E.atp) + 1
            E.eng.align2_batch(bad, E.aq, E.atp)
        elif entry == "reg2aln":
            bad = E.ct[:K].copy()
            bad["qoff"][K // 2] = len(E.cq) + 1
            E.eng.reg2aln_batch(bad, E.cq, OPS, MD)
        else:
            bad = E.words.copy()
            bad[0] = len(bad) + 1  # the first record ends past the stream
            E.eng.sw_stream(bad, E.nt)
    assert ei.value.code == abi.E_INVAL
    assert _same(call(), first)
