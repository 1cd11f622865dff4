"""GPU tests of bwagpu_sam_text_device (the XA strings and mem_aln2sam on the device)
against the text the reference's own mem_sam_pe and mem_aln2sam wrote
(tests/golden/sam_text_<set>.npz), byte for byte; and of the whole device chain
mark_primary_device -> pair_select_device -> xa_select_device ->
reg2aln_jobs_device -> reg2aln_device -> sam_text_device on one stream, whose end
is the reference's SAM text."""
import ctypes as C

import numpy as np
import pytest

import pair_io as P
import rescue_io as R
import sam_io as S
from bwagpu import abi
from bwagpu.engine import Engine

pytestmark = pytest.mark.gpu

PAD, FILL = 64, 0xEE


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(d):
        key = (id(d.genome["pac"]), np.asarray(d.alt).tobytes())
        if key not in made:
            g = d.genome
            e = Engine(0, d.opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
            e.set_alt(d.alt)
            made[key] = e
        return made[key]

    yield get
    for e in made.values():
        e.close()


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    if b.size == 0:
        b = np.zeros(88, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


class Batch:
    """one batch in device memory up to the records: what bwagpu_sam_text_device reads"""

    def __init__(self, torch, tag, n, off, regs, sel, out_mapq, seq_off, seq, n_contigs, max_ops, max_md):
        self.torch, self.n_reads, self.n_regs = torch, len(n), len(regs)
        self.max_ops, self.max_md, self.n_contigs = max_ops, max_md, n_contigs
        self.job_cap = max(self.n_regs, 1)
        inp = S.read_inputs(tag, seq_off)
        c_off, c_names = S.contigs(n_contigs)
        self.host = dict(n=n, off=off, regs=regs, sel=sel, out_mapq=out_mapq, seq_off=seq_off, seq=seq)
        self.d = {k: to_dev(torch, v) for k, v in dict(
            off=off, regs=regs, n=n, sel=sel, out_mapq=out_mapq, seq_off=seq_off, seq=seq, qual=inp["qual"],
            name_off=inp["name_off"], names=inp["names"], comment_off=inp["comment_off"], comments=inp["comments"],
            contig_off=c_off, contig_names=c_names).items()}
        dev = torch.device("cuda", 0)
        i32 = lambda k: torch.full((max(k, 1),), -7, dtype=torch.int32, device=dev)  # noqa: E731
        self.d.update(xa_of=i32(self.n_regs), job_select=i32(self.n_regs), job_of=i32(self.n_regs), n_jobs=i32(2),
                      tasks=torch.zeros(self.job_cap * 48, dtype=torch.uint8, device=dev),
                      aln=torch.full((self.job_cap * 40,), 0xA5, dtype=torch.uint8, device=dev),
                      cigar=torch.full((self.job_cap * max_ops * 4,), 0xA5, dtype=torch.uint8, device=dev),
                      md=torch.full((self.job_cap * max_md,), 0xA5, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()  # the fills ran on torch's stream; the entries run on the context's or the caller's

    def p(self, k):
        return self.d[k].data_ptr()

    def records(self, eng, st=None):
        """xa_select_device -> reg2aln_jobs_device -> reg2aln_device on st"""
        eng.xa_select_device(self.n_reads, self.p("off"), self.p("regs"), self.p("n"), self.p("sel"), self.p("out_mapq"),
                             self.p("xa_of"), self.p("job_select"), None, st)
        eng.reg2aln_jobs_device(self.n_reads, self.p("off"), self.p("regs"), self.p("n"), self.p("job_select"),
                                self.p("seq_off"), self.job_cap, self.p("tasks"), self.p("job_of"), self.p("n_jobs"), st)
        eng.reg2aln_device(self.job_cap, self.p("tasks"), self.p("seq"), len(self.host["seq"]), self.p("aln"),
                           self.p("cigar"), self.p("md"), self.max_ops, self.max_md, self.p("n_jobs"), st)

    def prepare(self, flags=0, text_cap=0, qual=True, comments=True, rg=S.RG_ID):
        """the outputs of one sam_text_device call, each with sentinels on both sides, and its argument struct.
        The fills run on torch's stream: synchronize before a launch on another stream"""
        torch, dev = self.torch, self.torch.device("cuda", 0)
        buf = torch.full((text_cap + 2 * PAD,), FILL, dtype=torch.uint8, device=dev)
        off = torch.full((self.n_reads + 3,), -7, dtype=torch.int64, device=dev)
        status = torch.full((self.n_reads // 2 + 2,), -7, dtype=torch.int32, device=dev)
        text_n = torch.full((4,), -7, dtype=torch.int64, device=dev)
        t = abi.SamText()
        for k in ("reg_off:off", "regs", "n", "sel", "out_mapq", "xa_of", "job_of", "aln", "cigar", "md", "seq_off", "seq",
                  "name_off", "names", "contig_off", "contig_names"):
            f, _, src = k.partition(":")
            setattr(t, "dev_" + f, self.p(src or f))
        t.dev_qual = self.p("qual") if qual else None
        t.dev_comment_off, t.dev_comments = (self.p("comment_off"), self.p("comments")) if comments else (None, None)
        t.rg_id, t.flags, t.n_contigs, t.job_cap = rg, flags, self.n_contigs, self.job_cap
        t.max_ops, t.max_md, t.text_cap = self.max_ops, self.max_md, text_cap
        t.dev_text, t.dev_text_off = buf.data_ptr() + PAD, off.data_ptr() + 8
        t.dev_status, t.dev_text_n = status.data_ptr() + 4, text_n.data_ptr() + 8
        self.keep = (buf, off, status, text_n, t)

    def launch(self, eng, st=None, steps=None):
        """the call; or its steps one by one (0 count, 1 scan, 2 write)"""
        if steps is None:
            eng.sam_text_device(self.keep[4], self.n_reads, st)
        for step in steps or ():
            eng.sam_text_device(self.keep[4], self.n_reads, st, step=step)

    def text(self, eng, *a, **kw):
        """one call, waited for -> (off, text, status, text_n)"""
        self.prepare(*a, **kw)
        self.torch.cuda.synchronize()
        self.launch(eng)
        self.torch.cuda.synchronize()
        return self.result()

    def result(self):
        buf, off, status, text_n, t = self.keep
        b, o, s, tn = buf.cpu().numpy(), off.cpu().numpy(), status.cpu().numpy(), text_n.cpu().numpy()
        cap = int(t.text_cap)
        # nothing outside the arrays, and nothing of the text past what was written
        assert (b[:PAD] == FILL).all() and (b[PAD + cap:] == FILL).all()
        assert o[0] == -7 and o[-1] == -7 and s[0] == -7 and s[-1] == -7 and tn[0] == -7 and tn[-1] == -7
        o, s, tn = o[1:-1], s[1:-1], tn[1:3]
        assert o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] == tn[0] <= min(cap, tn[1])
        assert (b[PAD + int(tn[0]):] == FILL).all()
        text = b[PAD:PAD + int(tn[0])].tobytes()
        assert b"\0" not in text
        for r in range(self.n_reads):
            assert o[r] == o[r + 1] or text[o[r + 1] - 1:o[r + 1]] == b"\n", r
            assert (o[r] == o[r + 1]) == (s[r >> 1] != abi.SAM_DONE), r
        return o, text, s, tn


def batch_of(torch, name, key, max_ops=S.MAX_OPS, max_md=S.MAX_MD):
    d, seq_off, seq, runs = S.load(name)
    mode, flags = S.KEYS[key]
    b = Batch(torch, name, d.n, d.off, d.regs[mode], d.sel[mode], d.out_mapq[mode], seq_off, seq,
              len(d.genome["ann_len"]), max_ops, max_md)
    return d, b, runs[key], flags


RUNS = [(n, k) for n in S.SETS for k in S.keys_of(n)] + [("cases", k) for k in S.KEYS]


@pytest.mark.parametrize("name,key", RUNS, ids=[f"{n}-{k}" for n, k in RUNS])
def test_text_is_the_references(torch, engines, name, key):
    d, b, want, flags = batch_of(torch, name, key)
    eng = engines(d)
    b.records(eng)
    need = int(want.off[-1])
    assert want.n_full == want.n_reads  # otherwise the need comes from a first call
    off, text, status, tn = b.text(eng, flags, need)
    assert (status == abi.SAM_DONE).all() and tn.tolist() == [need, need]
    assert want.mismatch(off, text) is None


def test_mem_aln2sam_cases(torch, engines):
    """hand-built records: CIGARs of 1 to 200 ops, reads of 1 to 250 bases on both strands, positions of 1 and
    10 digits, MD of 1 and max_md - 1 bytes; with and without qualities"""
    a = S.load_aln()
    eng = engines(S.load("cases")[0])
    n = a["n"].astype(np.int32)
    b = Batch(torch, "aln", n, R.offsets(n), a["regs"].astype(abi.ALNREG_DTYPE), a["sel"].astype(abi.PAIRSEL_DTYPE),
              a["out_mapq"], a["seq_off"], a["seq"], int(a["n_contigs"][0]), S.ALN_MAX_OPS, S.ALN_MAX_MD)
    for k in ("xa_of", "job_of", "aln", "cigar", "md"):
        b.d[k] = to_dev(torch, a[k])
    for want, qual in ((a["with_qual"], True), (a["no_qual"], False)):
        need = int(want.off[-1])
        off, text, status, tn = b.text(eng, 0, need, qual=qual)
        assert (status == abi.SAM_DONE).all() and tn.tolist() == [need, need]
        assert want.mismatch(off, text) is None


def test_steps_alone_leave_what_the_call_leaves(torch, engines):
    """bwagpu_debug_sam_text_step, which the timing tool uses: count, scan and write one by one"""
    d, b, want, flags = batch_of(torch, "cases", "other")
    eng = engines(d)
    b.records(eng)
    b.prepare(flags, int(want.off[-1]))
    torch.cuda.synchronize()
    b.launch(eng, steps=(0, 1, 2))
    torch.cuda.synchronize()
    off, text, status, _ = b.result()
    assert (status == abi.SAM_DONE).all() and want.mismatch(off, text) is None


def strip(text: bytes, r: int, qual: bool, comment: bool) -> bytes:
    """the reference's lines of read r without QUAL and / or without the comment"""
    out = []
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if not qual:
            f[10] = b"*"
        if not comment and S.read_comment(r):
            assert f[-1] == S.read_comment(r)
            f = f[:-1]
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def test_no_qualities_no_comments_no_read_group(torch, engines):
    d, b, want, flags = batch_of(torch, "cases", "nopair")
    eng = engines(d)
    b.records(eng)
    for qual, comment in ((False, True), (True, False), (False, False)):
        exp = [strip(want.span(r), r, qual, comment) for r in range(d.n_reads)]
        off, text, status, _ = b.text(eng, flags, sum(map(len, exp)), qual=qual, comments=comment)
        assert (status == abi.SAM_DONE).all()
        assert [text[off[r]:off[r + 1]] for r in range(d.n_reads)] == exp
    tag = b"\tRG:Z:" + S.RG_ID
    exp = [want.span(r).replace(tag, b"") for r in range(d.n_reads)]
    for rg in (None, b""):
        off, text, _, _ = b.text(eng, flags, sum(map(len, exp)), rg=rg)
        assert [text[off[r]:off[r + 1]] for r in range(d.n_reads)] == exp


def test_pairs_that_need_the_host(torch, engines):
    """a pair that was not selected, a needed record with a bad status, a needed region without a job and a
    rid outside the contigs: each pair gets its status and empty spans, every other pair its text"""
    d, b, want, flags = batch_of(torch, "rep", "pair")
    eng = engines(d)
    sel = d.sel[0].copy()
    sel["status"][3] = abi.SEL_SKIPPED
    sel["status"][4] = abi.SEL_TOO_MANY
    b.d["sel"] = to_dev(torch, sel)
    b.records(eng)
    torch.cuda.synchronize()
    job_of = b.d["job_of"].cpu().numpy()
    aln = b.d["aln"].cpu().numpy().view(abi.ALN_DTYPE).copy()
    paired = [p for p in range(6, d.n_reads // 2) if sel["branch"][p] == abi.SEL_PAIRED][::2]
    hit = {}
    for p, what in zip(paired, ("no_cigar", "overflow", "refused", "no_job", "rid", "mate_job")):
        r = 2 * p + (what == "mate_job")
        k = int(sel["z"][p][r & 1])
        assert sel["status"][p] == abi.SEL_DONE and k >= 0
        j = int(job_of[d.off[r] + k])
        assert j >= 0
        if what in ("no_job", "mate_job"):
            job_of[d.off[r] + k] = -1
        elif what == "rid":
            aln["rid"][j] = b.n_contigs
        else:
            aln["status"][j] = dict(no_cigar=abi.ALN_NO_CIGAR, overflow=abi.ALN_OVERFLOW, refused=abi.ALN_REFUSED)[what]
        hit[p] = abi.SAM_NEEDS_HOST
    hit.update({3: abi.SAM_SKIPPED, 4: abi.SAM_SKIPPED})
    b.d["job_of"], b.d["aln"] = to_dev(torch, job_of), to_dev(torch, aln)
    exp = [b"" if (r >> 1) in hit else want.span(r) for r in range(d.n_reads)]
    need = sum(map(len, exp))
    off, text, status, tn = b.text(eng, flags, need)
    assert tn.tolist() == [need, need]
    assert status.tolist() == [hit.get(p, abi.SAM_DONE) for p in range(d.n_reads // 2)]
    assert [text[off[r]:off[r + 1]] for r in range(d.n_reads)] == exp


def test_text_cap_short(torch, engines):
    d, b, want, flags = batch_of(torch, "rep_sw2", "nopair")
    eng = engines(d)
    b.records(eng)
    need, nr = int(want.off[-1]), d.n_reads
    # one byte short: the last pair does not fit; cut inside pair 100 and at its exact end
    for cap, first_out in ((need - 1, nr // 2 - 1), (int(want.off[200]) + 1, 100), (int(want.off[202]), 101), (0, 0)):
        off, text, status, tn = b.text(eng, flags, cap)
        written = int(want.off[2 * first_out])
        assert tn.tolist() == [written, need]
        assert status.tolist() == [abi.SAM_DONE] * first_out + [abi.SAM_NO_ROOM] * (nr // 2 - first_out)
        assert text == want.text[:written] and np.array_equal(off[:2 * first_out + 1], want.off[:2 * first_out + 1])
        assert (off[2 * first_out:] == written).all()


def test_two_calls_on_two_streams(torch, engines):
    d1, b1, w1, f1 = batch_of(torch, "rep", "nopair")
    d2, b2, w2, f2 = batch_of(torch, "rep_sw2", "pair")
    e1, e2 = engines(d1), engines(d2)  # one context where the sets share a genome: its scratch is then shared
    b1.records(e1)
    b2.records(e2)
    b1.prepare(f1, int(w1.off[-1]))
    b2.prepare(f2, int(w2.off[-1]))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    b1.launch(e1, s1.cuda_stream)
    b2.launch(e2, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for b, w in ((b1, w1), (b2, w2)):
        off, text, status, _ = b.result()
        assert (status == abi.SAM_DONE).all() and w.mismatch(off, text) is None


@pytest.mark.parametrize("name", ["ends", "rep_sw2"])
def test_whole_chain_on_one_stream(torch, engines, name):
    """from the rescued regions to the SAM text with no host copy in between"""
    d, s = P.load(name), R.load(name)
    xd, seq_off, seq, runs = S.load(name)
    want = runs["pair"]
    eng = engines(xd)
    eng.set_regs_post(0)
    so = d.selopt()
    b = Batch(torch, name, d.n, d.off, d.regs, np.zeros(d.n_reads // 2, abi.PAIRSEL_DTYPE),
              np.full(len(d.regs), -7, np.int32), seq_off, seq, len(d.genome["ann_len"]), S.MAX_OPS, S.MAX_MD)
    dev = torch.device("cuda", 0)
    d_pes = to_dev(torch, d.pes)
    d_npri = torch.full((d.n_reads,), -7, dtype=torch.int32, device=dev)
    d_mstat = torch.full((d.n_reads,), -7, dtype=torch.int32, device=dev)
    b.prepare(0, int(want.off[-1]))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    eng.mark_primary_device(d.n_reads, b.p("off"), b.p("regs"), b.p("n"), d_npri.data_ptr(), d_mstat.data_ptr(),
                            2 * d.pair_id0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), d.n_reads, b.p("off"), b.p("regs"), b.p("n"), d_npri.data_ptr(), None,
                           b.p("sel"), b.p("out_mapq"), d.pair_id0, so, st)
    b.records(eng, st)
    b.launch(eng, st)
    stream.synchronize()
    off, text, status, tn = b.result()
    assert (status == abi.SAM_DONE).all() and tn[0] == tn[1] == want.off[-1]
    assert want.mismatch(off, text) is None
    assert text.count(b"\n") == int(want.n_lines.sum()) > d.n_reads - 1


def test_argument_errors_and_refused_flags(torch, engines):
    d, b, want, _ = batch_of(torch, "cases", "pair")
    eng = engines(d)
    b.records(eng)
    b.text(eng, 0, int(want.off[-1]))
    good = b.keep[4]
    lib = abi.load()

    def call(n=d.n_reads, ctx=eng.ctx, t=good, **kw):
        if kw:
            t2 = abi.SamText()
            C.memmove(C.byref(t2), C.byref(t), C.sizeof(t))
            for k, v in kw.items():
                setattr(t2, k, v)
            t = t2
        return lib.bwagpu_sam_text_device(ctx, C.byref(t) if t is not None else None, n, None)

    assert call() == abi.OK
    assert call(ctx=None) == abi.E_INVAL and call(t=None) == abi.E_INVAL
    assert call(n=-2) == abi.E_INVAL and call(n=3) == abi.E_INVAL
    for f, _ in abi.SamText._fields_:
        if f.startswith("dev_") and f not in ("dev_qual", "dev_comment_off", "dev_comments"):
            assert call(**{f: None}) == abi.E_INVAL, f
    assert call(dev_comments=None) == abi.E_INVAL and call(dev_comment_off=None, dev_comments=None) == abi.OK
    assert call(text_cap=-1) == abi.E_INVAL and call(max_ops=0) == abi.E_INVAL and call(max_md=0) == abi.E_INVAL
    assert call(job_cap=-1) == abi.E_INVAL and call(n_contigs=-1) == abi.E_INVAL
    assert call(rg_id=b"x" * (abi.SAM_MAX_RG + 1)) == abi.E_INVAL and call(rg_id=b"x" * abi.SAM_MAX_RG) == abi.OK
    for f in (abi.MEM_F_ALL, abi.MEM_F_NO_MULTI, abi.MEM_F_PRIMARY5, abi.MEM_F_KEEP_SUPP_MAPQ, abi.MEM_F_REF_HDR):
        assert call(flags=f) == abi.E_UNSUPPORTED, f
    assert b"MEM_F_REF_HDR" in lib.bwagpu_last_error(eng.ctx)
    assert call(flags=abi.MEM_F_NOPAIRING | 0x2 | 0x20 | 0x400) == abi.OK  # ignored bits
    assert call(n=0) == abi.OK
    torch.cuda.synchronize()
    assert b.keep[1].cpu().numpy()[1] == 0 and b.keep[3].cpu().numpy()[1:3].tolist() == [0, 0]
