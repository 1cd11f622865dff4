"""bwagpu_destroy frees every grow-only buffer of its context (bwa-flow_amd/csrc/ctx.h: the
buffers own their memory, destroy_ctx names none of them), after a context that has served the
task entries, chain2aln through submit / wait and through the device entry, and one staged
host call; and after a call that was refused in validation.  The counters of
bwagpu_debug_live_buffers are process-wide and other modules may hold contexts, so only the
difference to a baseline taken before the context is created is asserted.  Every call's result is
checked against its golden values, as tests/test_gpu_task_entries.py does."""
import gc

import numpy as np
import pytest

import golden_io as G
import post_io as P
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine, compact
from test_gpu_regs_post import _device_batch
from test_gpu_task_entries import MD, OPS, Entries

pytestmark = pytest.mark.gpu

K = 64       # tasks per call; the stream is 60 reads' records, as there
READS = 60   # of c1_default, through chain2aln


@pytest.fixture(scope="module")
def E():
    """the inputs and golden outputs; every test makes (and closes) a context of its own"""
    e = Entries()
    e.eng.close()
    _, batch, want, want_n = G.load_chain_set("c1_default")
    e.sub = batch.subset(range(READS))
    e.sub_n = want_n[:READS]
    e.sub_regs = want[:int(np.sum(e.sub_n))]
    yield e
    e.eng.close()


def fresh_context(E):
    """-> the live buffers and bytes before E's new context exists"""
    gc.collect()  # a context that an earlier module dropped without closing goes now, not in mid-test
    base = Engine.debug_live_buffers()
    E.eng = E.eng.clone()
    return base


def chain2aln_checked(E, regs, n, what):
    assert np.array_equal(n, E.sub_n), f"{what}: per-read region counts differ"
    bad = G.region_mismatch(compact(E.sub, regs, n), E.sub_regs)
    assert bad is None, f"{what}: {bad}"


def test_destroy_frees_every_buffer(E):
    import torch
    base = fresh_context(E)
    eng = E.eng
    E.extend(K)
    E.align2(K)
    E.reg2aln(K)
    E.sw_stream()
    eng.submit(0, E.sub)
    chain2aln_checked(E, *eng.wait(0, E.sub), "submit / wait")
    dev = torch.device("cuda", 0)
    bc, keep = _device_batch(torch, E.sub)
    out = torch.zeros(max(E.sub.n_seeds, 1) * abi.ALNREG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    n = torch.zeros(E.sub.n_reads, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    eng.chain2aln_device(bc, out.data_ptr(), n.data_ptr(), None, stream.cuda_stream)
    stream.synchronize()
    chain2aln_checked(E, out.cpu().numpy().view(abi.ALNREG_DTYPE), n.cpu().numpy(), "device entry")
    del keep
    # one staged host call (Staging): the post-processing of the same set's regions
    s = P.load("c1_default")
    assert s.genome == 0 and bytes(abi.opt_from_dict(s.opt)) == bytes(eng.opt)  # this context's reference and options
    eng.set_alt(s.alt)
    regs, cnt = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, 3, s.id0, s.popt)
    want_regs, want_n = s.want[3]
    assert np.array_equal(cnt, want_n)
    assert G.region_mismatch(G.dense(regs, s.off, cnt), want_regs) is None
    live, live_bytes = Engine.debug_live_buffers()
    print(f"live buffers: {base[0]} -> {live}, bytes: {base[1]} -> {live_bytes}")
    assert live - base[0] >= 20 and live_bytes > base[1]
    eng.close()
    assert Engine.debug_live_buffers() == base


def test_destroy_after_refused_call(E):
    base = fresh_context(E)
    first = E.reg2aln(K)
    bad = E.ct[:K].copy()
    k = int(np.nonzero(E.cexp["status"][:K] == abi.ALN_OK)[0][0])  # a job that is aligned: its qb / qe are checked
    bad["qe"][k] = bad["l_seq"][k] + 1
    with pytest.raises(BwaGpuError) as ei:
        E.eng.reg2aln_batch(bad, E.cq, OPS, MD)
    assert ei.value.code == abi.E_INVAL and "outside its read" in str(ei.value)
    again = E.reg2aln(K)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first, again))
    assert Engine.debug_live_buffers()[0] > base[0]
    E.eng.close()
    assert Engine.debug_live_buffers() == base
