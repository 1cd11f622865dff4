"""Shared by the GPU tests of the CIGAR kernel (test_gpu_cigar_device.py,
test_gpu_cigar_edges.py): one bwagpu_reg2aln_device call on sentinel-filled
device buffers, the comparisons of its outputs, and the (bucket, matrix class)
arithmetic of bwagpu_reg2aln_batch."""
import numpy as np

import golden_io as G
from bwagpu import abi
from bwagpu.engine import Engine

SENT = 0xA5


def engine(refd, opt):
    return Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    if b.size == 0:
        b = np.zeros(64, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


class DevCall:
    """one reg2aln_device call: __init__ uploads the inputs and pre-fills the outputs with the sentinel
    (and waits for that); launch() is the call alone, with no wait before or after it"""

    def __init__(self, torch, eng, tasks, qpool, max_ops, max_md, n_cap=None, n_on_device=None, stream=None,
                 launch=True):
        dev = torch.device("cuda", 0)
        self.eng, self.stream, self.qlen = eng, stream, len(qpool)
        self.n_cap = len(tasks) if n_cap is None else n_cap
        self.max_ops, self.max_md = max_ops, max_md
        self.d_tasks, self.d_q = to_dev(torch, tasks), to_dev(torch, qpool)
        rows = max(self.n_cap, 1)
        self.d_out = torch.full((rows * 40,), SENT, dtype=torch.uint8, device=dev)
        self.d_cig = torch.full((rows * max_ops * 4,), SENT, dtype=torch.uint8, device=dev)
        self.d_md = torch.full((rows * max_md,), SENT, dtype=torch.uint8, device=dev)
        self.d_n = None if n_on_device is None else to_dev(torch, np.array([n_on_device], np.int32))
        torch.cuda.synchronize()
        if launch:
            self.launch()

    def launch(self):
        self.eng.reg2aln_device(self.n_cap, self.d_tasks.data_ptr(), self.d_q.data_ptr(), self.qlen,
                                self.d_out.data_ptr(), self.d_cig.data_ptr(), self.d_md.data_ptr(), self.max_ops,
                                self.max_md, None if self.d_n is None else self.d_n.data_ptr(), self.stream)

    def results(self):
        rows = max(self.n_cap, 1)
        return (self.d_out.cpu().numpy().view(abi.ALN_DTYPE)[:self.n_cap],
                self.d_cig.cpu().numpy().view(np.uint32).reshape(rows, self.max_ops)[:self.n_cap],
                self.d_md.cpu().numpy().reshape(rows, self.max_md)[:self.n_cap])


def run_device(torch, eng, tasks, qpool, max_ops, max_md, **kw):
    c = DevCall(torch, eng, tasks, qpool, max_ops, max_md, **kw)
    torch.cuda.synchronize()
    return c.results()


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENT).all()


def same_as(tasks, got, want):
    """records (every field), CIGARs and MDs of `got` equal those of `want` (both (out, cig, md))"""
    out, cig, md = got
    w_out, w_cig, w_md = want
    bad = G.aln_mismatch(tasks, out, cig, md, *G.aln_expected_from(w_out, w_cig, w_md))
    if bad is None and out.tobytes() != np.ascontiguousarray(w_out).tobytes():
        bad = "records differ outside the compared fields"
    return bad


def zb_class(opt, l_pac, t):
    """(bucket, matrix class) of an alignable job: bwagpu_reg2aln_batch's arithmetic"""
    lq, rl = int(t["qe"] - t["qb"]), int(t["re"] - t["rb"])
    a, w = opt["a"], opt["w"]

    def infer(q, r):
        if lq == rl and lq * a - int(t["truesc"]) < (q + r - a) * 2:
            return 0
        return max(int((min(lq, rl) * a - int(t["truesc"]) - q) / r + 2.), abs(lq - rl))
    w2 = max(infer(opt["o_del"], opt["e_del"]), infer(opt["o_ins"], opt["e_ins"]))
    if w2 > w:
        w2 = min(w2, int(t["w"]))
    w2max = min(min(w2, 4 * w) * 4, 4 * w)
    half = (lq + 1) >> 1
    m0 = int(opt["mat"][0])
    mg = max(int((half * m0 - opt["o_ins"]) / opt["e_ins"] + 1.), int((half * m0 - opt["o_del"]) / opt["e_del"] + 1.), 1)
    dl = abs(rl - lq)
    wb = max(min((mg + dl + 1) >> 1, w2max), dl + 3)
    zb = min(lq, 2 * wb + 1) * rl
    cd = (lq + 64) >> 6
    return (cd - 1 if cd <= 4 else (4 if cd <= 8 else 5)), (0 if zb <= 8192 else (1 if zb <= 24576 else 2))
