"""Late-settled right sides and the dense certificate kernel (DESIGN.md §26;
Engine.ungapped_right, default on).  A right side that holds the ungapped
certificate behind a left side that needs the DP enters no list: after the
list's left launch spec_settle_right_kernel finishes its seed from the slot that
launch wrote.  The certificate's records come from a kernel that takes the
sides sixteen bases at a time, whichever side a pass belongs to.

Expected regions come from the CPU oracle (oracle.chain2aln("oracle", ...)) or
the golden vectors, and the expected numbers of settled and late-settled sides
from the certificate's conditions restated here in numpy on the batch's own
bases, never from the code under test:

* a hand-made batch on the golden genome, one exact seed per chain: the late
  class (left side with two mismatches, right side certified) with right sides
  of 1, 15, 16, 17, 31, 32, 33, 105, 127 and 129 bases, exact or with one
  mismatch, on both strands, beside one read of every other left/right class, a
  read under 16 bases, a right side cut by its contig's end, a right side with
  one mismatch in each of two passes (dead only in their sum), one whose score
  comes back to its maximum across a pass boundary, and a left side with an
  8-base deletion;
* the same batch under pen_clip3 = 0 (every right side takes the local branch)
  and 20 (the to-end branch), w = 10 (the deletion's left call triggers the
  band retry, so the seed's w is the doubled one), a scoring outside the 8-bit
  row-max key and extension form 2; each with the switch on and off;
* the device entry with its outputs prefilled;
* the golden chain sets at both switch values, the fixtures in a child process
  under BWAGPU_UNGAPPED_RIGHT=0;
* 4,096 reads of the C2 fixture: the certificate's counters per round equal to
  the parent kernel's (profiles/r13_c2_4096_parent_ungapped.json), and round
  A's settled plus late-settled sides equal to the restated conditions.  Round
  A's tasks follow from the batch alone (each chain's first seed in processing
  order); round B's depend on the selection, so round B is compared with the
  parent's recorded counts only.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_io as G
import oracle
from bwagpu import abi, workload
from bwagpu.engine import Batch, Engine, compact
from test_gpu_ungapped import make_engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
RIGHT_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 105, 127, 129)
FIELDS = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")


def run_device(eng, batch, prefill=False):
    """one batch through the device entry -> regs, n, bwagpu_debug_spec_ungapped's words [3 rounds][settled at
    sort time, their bases, left listed, right listed], bwagpu_debug_spec_ungapped_right's [3 rounds][settled
    after the left launch, their bases]"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev) for k in FIELDS}
    out = torch.full((max(batch.n_seeds, 1) * 88,), 0xFF if prefill else 0, dtype=torch.uint8, device=dev)
    nn = torch.full((max(batch.n_reads, 1),), -7 if prefill else 0, dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    c.seq_bytes = int(batch.seq_off[-1])
    for k in FIELDS:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), None, stream.cuda_stream)
    torch.cuda.synchronize()
    ctr = np.zeros(12, np.int64)
    assert eng.lib.bwagpu_debug_spec_ungapped(eng.ctx, C.c_void_p(stream.cuda_stream),
                                              ctr.ctypes.data_as(C.c_void_p)) == 0
    late = eng.ungapped_right_counters(stream.cuda_stream)
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], ctr.reshape(3, 4), late


def strands(refd):
    l_pac, pac = refd["l_pac"], refd["pac"]
    x = np.arange(l_pac, dtype=np.int64)
    fwd = ((pac[x >> 2].astype(np.int64) >> ((~x & 3) << 1)) & 3).astype(np.uint8)
    return np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])  # the 2-strand coordinate space


def planted(both, x0, n, mm=()):
    """n read bases aligned to the 2-strand coordinates x0 .. x0 + n - 1, with mismatches at the offsets mm"""
    fl = both[x0:x0 + n].copy()
    for p in mm:
        fl[p] = (fl[p] + 1) & 3
    return fl


def two_mm(n):
    return (n // 4, n // 2) if n >= 2 else ()


def specs():
    """name, left length, seed length, right length, left mismatches, right mismatches"""
    out = []
    for qr in RIGHT_LENGTHS:  # the late class: a left side with two mismatches, a certified right side
        out.append((f"late_{qr}_exact", 10, 19, qr, two_mm(10), ()))
        out.append((f"late_{qr}_mm1", 10, 19, qr, two_mm(10), (qr // 4,)))
    # one read of every other class
    out += [("none_none", 0, 60, 0, (), ()), ("none_cert", 0, 30, 40, (), (10,)), ("none_dp", 0, 30, 40, (), (10, 20)),
            ("cert_none", 40, 30, 0, (10,), ()), ("dp_none", 40, 30, 0, (10, 20), ()),
            ("cert_cert", 33, 30, 47, (), (46,)), ("cert_dp", 20, 30, 20, (5,), (5, 10)),
            ("dp_dp", 20, 30, 20, (5, 10), (5, 10))]
    out.append(("short_read", 4, 8, 3, (1, 2), ()))          # under 16 bases: the passes go base by base
    out.append(("sum_dead", 20, 30, 40, (5, 10), (12, 20)))  # one mismatch in the first pass, one in the second
    out.append(("tie", 20, 30, 18, (5, 10), (13,)))          # c = 13 at base 12, 9 at 13, 13 again at 17: am = 13
    return out


@pytest.fixture(scope="module")
def case():
    """-> refd, oracle.Ref, batch (one chain of one seed per read), per read: name, seed length, and per side
    the query bases and the aligned reference bases from the seed outwards with the target's length"""
    refd = G.load_ref()
    l_pac = refd["l_pac"]
    both = strands(refd)
    seqs, seeds, rids, info = [], [], [], []

    def add(name, c, rbeg, left, ln, right, ltl=1 << 20, rtl=1 << 20):
        ql, qr = len(left), len(right)
        seqs.append(np.concatenate([left, both[rbeg:rbeg + ln], right]))
        seeds.append((rbeg, ql, ln, ln, 0))
        rids.append(c)
        info.append((name, ln, (left[::-1], both[rbeg - ql:rbeg][::-1], ltl), (right, both[rbeg + ln:rbeg + ln + qr], rtl)))

    i = 0
    for name, ql, ln, qr, lmm, rmm in specs():
        for rev in (False, True):
            c = i % len(refd["ann_offset"])
            a0, al = int(refd["ann_offset"][c]), int(refd["ann_len"][c])
            f0 = a0 + 2000 + (7919 * i) % (al - 5000)  # the seed's first base, forward strand
            rbeg = 2 * l_pac - (f0 + ln) if rev else f0
            add(name + ("_rev" if rev else "_fwd"), c, rbeg, planted(both, rbeg - ql, ql, lmm), ln,
                planted(both, rbeg + ln, qr, rmm))
            i += 1
    # a right side cut by its contig's end: five target rows for twenty query bases (not certified), the bases
    # past the contig's end matching all the same
    a0, al = int(refd["ann_offset"][0]), int(refd["ann_len"][0])
    rbeg = a0 + al - 5 - 30
    add("contig_end", 0, rbeg, planted(both, rbeg - 20, 20, two_mm(20)), 30, planted(both, rbeg + 30, 20), rtl=5)
    # a left side with an 8-base deletion ten bases from the seed (the band retry under w = 10), a certified right side
    c = 1
    rbeg = int(refd["ann_offset"][c]) + 3000
    left = np.concatenate([both[rbeg - 78:rbeg - 18], both[rbeg - 10:rbeg]])
    seqs.append(np.concatenate([left, both[rbeg:rbeg + 30], both[rbeg + 30:rbeg + 70]]))
    seeds.append((rbeg, 70, 30, 30, 0))
    rids.append(c)
    info.append(("deletion", 30, (left[::-1], both[rbeg - 70:rbeg][::-1], 1 << 20),
                 (both[rbeg + 30:rbeg + 70], both[rbeg + 30:rbeg + 70], 1 << 20)))
    n = len(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    batch = Batch(off, np.concatenate(seqs), np.arange(n + 1), np.arange(n + 1), np.array(rids, np.int32),
                  np.zeros(n, np.float32), np.array(seeds, abi.SEED_DTYPE))
    assert int(np.diff(off).max()) <= 160 and n <= 80, "a few dozen reads, every one in the first length bin"
    ref = oracle.Ref(l_pac, refd["ann_offset"], refd["ann_len"], refd["pac"])
    return refd, ref, batch, info


def cert_fn(opt):
    """the certificate's conditions 1-5 for a side given as (query, aligned target, target length) behind a seed
    of ln bases"""
    mat = np.asarray(opt["mat"] if opt.get("mat") is not None else abi.fill_scmat(opt["a"], opt["b"]), np.int64).reshape(5, 5)
    max_mat = int(max(0, mat.max()))
    oe_min = min(opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"])
    opt_ok = (opt["zdrop"] <= 0 or opt["zdrop"] >= oe_min) and (opt["w"] >> 1) + (opt["w"] >> 2) > 0 and max_mat >= 1

    def cert(q, t, tlen, ln):
        return (len(q) >= 1 and opt_ok and ln * opt["a"] >= oe_min and tlen >= len(q)
                and int((max_mat - mat[t[:len(q)], np.minimum(q, 4)]).sum()) < oe_min)
    return cert


def expected(opt, info):
    """-> sides settled at sort time, late right sides, their bases, the reads' classes by name"""
    cert = cert_fn(opt)
    settled = late = late_q = 0
    classes = {}
    for name, ln, (lq, lt, ltl), (rq, rt, rtl) in info:
        cl, cr = cert(lq, lt, ltl, ln), cert(rq, rt, rtl, ln)
        in_l = len(lq) > 0 and not cl
        settled += int(cl) + int(cr and not in_l)
        late += int(cr and in_l)
        late_q += len(rq) if cr and in_l else 0
        classes[name] = ("none" if len(lq) == 0 else "cert" if cl else "dp", "none" if len(rq) == 0 else "cert" if cr else "dp")
    return settled, late, late_q, classes


def check(refd, ref, batch, info, opt, what, form=None, kernel=None, prefill=False):
    """the batch with the switch on and off -> the regions (the oracle's) per read, the classes"""
    oregs, on, ost = oracle.chain2aln("oracle", opt, ref, batch)
    want = compact(batch, oregs, on)
    settled, late, late_q, classes = expected(opt, info)
    eng = make_engine(refd, opt)
    assert eng.ungapped_right() == 1 and eng.ungapped() == 1, "both switches start on"
    if form is not None:
        eng.ext_form(form)
    if kernel is not None:
        assert eng.ext_kernel(160) == eng.EXT_KERNELS[kernel], eng.ext_kernel(160)
    ctrs, cells = {}, {}
    for on_off in (1, 0):
        eng.ungapped_right(on_off)
        assert eng.ungapped_right() == on_off
        regs, n, ctr, lt = run_device(eng, batch, prefill)
        print(f"{what}, switch {on_off}: expected settled {settled}, late {late} ({late_q} bases); per round [settled, "
              f"their bases, left listed, right listed] {ctr.tolist()}, [late settled, their bases] {lt.tolist()}")
        assert np.array_equal(n, on), f"{what}, switch {on_off}: {int((n != on).sum())} reads with a different region count"
        assert G.region_mismatch(compact(batch, regs, n), want) is None, f"{what}, switch {on_off}"
        assert int(ctr[:, 0].sum()) == settled, f"{what}, switch {on_off}: {int(ctr[:, 0].sum())} sides settled at sort time"
        if on_off:
            assert lt[0].tolist() == [late, late_q] and not lt[1:].any(), f"{what}: late counters {lt.tolist()}"
        else:
            assert not lt.any(), f"{what}: late counters {lt.tolist()} with the switch off"
        ctrs[on_off] = ctr
        regs, n = eng.chain2aln(batch)  # the host entry, whose statistics can be read
        assert np.array_equal(n, on) and G.region_mismatch(compact(batch, regs, n), want) is None, f"{what}, switch {on_off}"
        st = eng.last_stats()
        assert st["ext_calls"] == int(ost[2]) and st["cells"] <= int(ost[0]) and st["rows"] <= int(ost[1]), (st, ost)
        cells[on_off] = st["cells"]
    eng.close()
    assert cells[1] <= cells[0], f"{what}: cells {cells[1]} with the switch on, {cells[0]} off"
    # the switch takes the late right sides' DP cells away and nothing else (the left side's cells stay with the
    # seed): each such call ran at least one cell, and at most (qr + 1) columns on the rows of its window, which
    # for these one-seed chains reaches cal_max_gap(qr) past the query
    cert = cert_fn(opt)
    late_qr = [len(rq) for _, ln, (lq, lt, ltl), (rq, rt, rtl) in info
               if cert(rq, rt, rtl, ln) and len(lq) > 0 and not cert(lq, lt, ltl, ln)]
    assert len(late_qr) == late
    most = sum((qr + 1) * (qr + cal_max_gap(opt, qr)) for qr in late_qr)
    assert late <= cells[0] - cells[1] <= most, f"{what}: cells {cells[0]} off, {cells[1]} on, at most {most} apart"
    assert np.array_equal(ctrs[1][:, :3], ctrs[0][:, :3]), "settled sides, their bases and the left lists do not depend on the switch"
    assert (ctrs[0][:, 3] - ctrs[1][:, 3]).tolist() == [late, 0, 0], "the right lists are shorter by the late sides"
    assert on.min() == 1 and on.max() == 1, "one region per read"
    return want, classes


def test_hand_made_batch(case):
    refd, ref, batch, info = case
    opt = G.load_chain_set("c1_default")[0]
    want, classes = check(refd, ref, batch, info, opt, "default options", kernel=18)
    for l in ("none", "cert", "dp"):  # every left/right combination occurs
        for r in ("none", "cert", "dp"):
            assert (l, r) in classes.values(), (l, r)
    for name, cl in classes.items():
        if name.startswith("late_") or name == "deletion":
            assert cl == ("dp", "cert"), (name, cl)
    for name in ("contig_end", "sum_dead_fwd", "sum_dead_rev"):
        assert classes[name] == ("dp", "dp"), (name, classes[name])
    assert classes["tie_fwd"] == classes["short_read_fwd"] == classes["short_read_rev"] == ("dp", "cert")


VARIANTS = {"clip3_local": (dict(pen_clip3=0), None, None),   # gscore <= score always: the local branch
            "clip3_end": (dict(pen_clip3=20), None, None),    # the to-end branch wherever the side reaches its end
            "w_10": (dict(w=10), None, None),                 # the deletion's left call is tried again with w = 20
            "non_key8": (dict(a=2, b=5, o_del=7, e_del=2, o_ins=5, e_ins=3, pen_clip5=3, pen_clip3=9, w=30, zdrop=40),
                         None, 15),                           # spec_side4_kernel<32, 8, false>
            "form_2": (dict(), 2, 14)}                        # spec_side4_kernel<32, 5, true>


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hand_made_batch_variants(case, variant):
    refd, ref, batch, info = case
    delta, form, kernel = VARIANTS[variant]
    opt = dict(G.load_chain_set("c1_default")[0], **delta)
    if "a" in delta:
        opt["mat"] = abi.fill_scmat(opt["a"], opt["b"]).reshape(-1)
    want, classes = check(refd, ref, batch, info, opt, variant, form=form, kernel=kernel)
    names = [x[0] for x in info]
    reg = {nm: want[k] for k, nm in enumerate(names)}  # one region per read, in read order
    lens = np.diff(batch.seq_off)
    if variant in ("clip3_local", "clip3_end"):
        for nm in ("tie_fwd", "tie_rev"):
            assert classes[nm] == ("dp", "cert")
            k = names.index(nm)
            # local: the right side ends at its first maximum (13 bases); to-end: at the read's end
            assert int(reg[nm]["qe"]) == (20 + 30 + 13 if variant == "clip3_local" else int(lens[k])), (nm, reg[nm])
    if variant == "w_10":
        assert classes["deletion"] == ("dp", "cert")
        assert int(reg["deletion"]["w"]) == 20, f"the deletion's left side did not take the band retry: {reg['deletion']}"
        assert int(reg["tie_fwd"]["w"]) == 10


def test_prefilled_output(case):
    refd, ref, batch, info = case
    opt = G.load_chain_set("c1_default")[0]
    check(refd, ref, batch, info, opt, "prefilled output", prefill=True)


@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_chain_sets_on_and_off(name):
    refd = G.load_ref()
    opt, batch, want, want_n = G.load_chain_set(name)
    ref = oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])
    _, _, ost = oracle.chain2aln("oracle", opt, ref, batch)
    eng = make_engine(refd, opt)
    cells = {}
    for on in (1, 0):
        eng.ungapped_right(on)
        regs, n = eng.chain2aln(batch)
        assert np.array_equal(n, want_n), f"switch {on}: {int((n != want_n).sum())} reads with a different region count"
        assert G.region_mismatch(compact(batch, regs, n), want) is None, f"switch {on}"
        st = eng.last_stats()
        assert st["ext_calls"] == int(ost[2]) and st["cells"] <= int(ost[0]) and st["rows"] <= int(ost[1]), (on, st, ost)
        cells[on] = st["cells"]
        dregs, dn, ctr, lt = run_device(eng, batch)
        assert np.array_equal(dn, want_n) and G.region_mismatch(compact(batch, dregs, dn), want) is None
        print(f"{name}, switch {on}: cells {st['cells']}; settled {ctr.tolist()}, late {lt.tolist()}")
        assert on or not lt.any(), f"late counters {lt.tolist()} with the switch off"
        if on and name == "c1_default":
            assert lt[0, 0] > 0, "no late right side in c1_default: the test is vacuous"
    assert cells[1] <= cells[0]
    eng.close()


def test_variant_child_with_the_switch_off():
    """the fixtures' batches against the reference's regions in a child process (the library reads the knob once)"""
    env = dict(os.environ, BWAGPU_UNGAPPED_RIGHT="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "gpu_variant_child.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["c2"] and all(r["c2"]), r
    assert r["c5"] and all(r["c5"]), r


def cal_max_gap(opt, qlen):
    def tdiv(a, b):  # C's division
        return int(a / b)
    l = max(tdiv(qlen * opt["a"] - opt["o_del"], opt["e_del"]) + 1, tdiv(qlen * opt["a"] - opt["o_ins"], opt["e_ins"]) + 1, 1)
    return min(l, opt["w"] << 1)


def fetch_bases(ref, x0, n):
    """the bases at the 2-strand coordinates x0 .. x0 + n - 1 (one strand), from the pac"""
    x = np.arange(x0, x0 + n, dtype=np.int64)
    rev = x >= ref.l_pac
    f = np.where(rev, 2 * ref.l_pac - 1 - x, x)
    bs = (ref.pac[f >> 2].astype(np.int64) >> ((~f & 3) << 1)) & 3
    return np.where(rev, 3 - bs, bs)


def round_a_expected(opt, ref, b):
    """round A extends each chain's first seed in processing order (the largest score, of equal ones the last) in
    its chain's window (bwamem.c:648-668 with bns_fetch_seq's clipping to the contig) -> the sides that hold the
    certificate and settle at sort time, and the late right sides"""
    cert = cert_fn(opt)
    l_pac = int(ref.l_pac)
    settled = late = 0
    for rd in range(b.n_reads):
        lq = int(b.seq_off[rd + 1] - b.seq_off[rd])
        seq = b.seq[b.seq_off[rd]:b.seq_off[rd + 1]]
        for c in range(int(b.read_chain_off[rd]), int(b.read_chain_off[rd + 1])):
            sd = b.seeds[int(b.chain_seed_off[c]):int(b.chain_seed_off[c + 1])]
            if len(sd) == 0:
                continue
            lo = min(int(s["rbeg"]) - (int(s["qbeg"]) + cal_max_gap(opt, int(s["qbeg"]))) for s in sd)
            hi = max(int(s["rbeg"]) + int(s["len"]) + (lq - int(s["qbeg"]) - int(s["len"]))
                     + cal_max_gap(opt, lq - int(s["qbeg"]) - int(s["len"])) for s in sd)
            lo, hi = max(lo, 0), min(hi, 2 * l_pac)
            if lo < l_pac < hi:
                if int(sd[0]["rbeg"]) < l_pac:
                    hi = l_pac
                else:
                    lo = l_pac
            rid = int(b.chain_rid[c])
            a0, al = int(ref.ann_offset[rid]), int(ref.ann_len[rid])
            if int(sd[0]["rbeg"]) >= l_pac:
                a0 = 2 * l_pac - (a0 + al)
            lo, hi = max(lo, a0), min(hi, a0 + al)
            k = max(range(len(sd)), key=lambda t: (int(sd[t]["score"]), t))
            rbeg, qb, ln = int(sd[k]["rbeg"]), int(sd[k]["qbeg"]), int(sd[k]["len"])
            qr = lq - qb - ln
            cl = cert(seq[:qb][::-1], fetch_bases(ref, rbeg - qb, qb)[::-1], rbeg - lo, ln) if qb else False
            cr = cert(seq[qb + ln:], fetch_bases(ref, rbeg + ln, qr), hi - (rbeg + ln), ln) if qr else False
            in_l = qb > 0 and not cl
            settled += int(cl) + int(cr and not in_l)
            late += int(cr and in_l)
    return settled, late


def test_c2_fixture_counters_match_the_parent_kernel():
    """4,096 reads of the C2 fixture: the dense kernel's records give the parent kernel's counts"""
    opt, ref, rbs = workload.load_fixture()
    sub = rbs[0].batch.subset(range(4096))
    assert int(np.diff(sub.seq_off).max()) <= 160
    oref = oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac)
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, sub)
    want = compact(sub, oregs, on)
    with open(os.path.join(REPO, "profiles", "r13_c2_4096_parent_ungapped.json")) as f:
        parent = np.array(json.load(f)["rounds"], np.int64)  # [3][settled, their bases, left listed, right listed]
    settled_a, late_a = round_a_expected(opt, ref, sub)
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    for on_off in (1, 0):
        eng.ungapped_right(on_off)
        regs, n, ctr, lt = run_device(eng, sub)
        print(f"switch {on_off}: [settled, their bases, left listed, right listed] {ctr.tolist()}, parent "
              f"{parent.tolist()}; late {lt.tolist()}; round A restated: settled {settled_a}, late {late_a}")
        assert np.array_equal(n, on) and G.region_mismatch(compact(sub, regs, n), want) is None, f"switch {on_off}"
        assert np.array_equal(ctr[:, :3], parent[:, :3]), f"switch {on_off}: settled sides, bases or left lists differ"
        assert np.array_equal(ctr[:, 3] + lt[:, 0], parent[:, 3]), f"switch {on_off}: right listed + late"
        assert int(ctr[0, 0]) == settled_a and int(lt[0, 0]) == (late_a if on_off else 0)
        assert int(ctr[0, 0] + lt[0, 0]) == settled_a + (late_a if on_off else 0)
    eng.close()
