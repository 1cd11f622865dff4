"""The ungapped certificate on the device (Engine.ungapped, default on;
DESIGN.md §24): a side of a phased extension task whose diagonal loses less
than the cheapest gap open is settled when the side lists are sorted and never
enters a list.

Expected regions come from the golden vectors or the CPU oracle
(oracle.chain2aln("oracle", ...)), and the expected number of settled sides
from the certificate's conditions restated here in numpy on the batch's own
bases, never from the code under test:

* the four golden chain sets with the switch on and off (c5_mixed among them:
  its second length bin is not phased and stays as it was);
* a hand-made batch on the golden genome, one exact seed per chain: side
  lengths 0, 1, 63, 64 and 105, both strands, flanks that are exact, carry
  three Ns (P = oe_min - 1), one mismatch and one N (P = oe_min), one or two
  mismatches or a 1-base deletion, in all four left/right combinations of
  certified and DP, and a read at a contig start whose left target is shorter
  than its query;
* the same batch under zdrop = 3 and w = 1 (the certificate's conditions 4 and
  5 fail: nothing is settled), zdrop = oe_min, a scoring outside the 8-bit
  row-max key (spec_side4_kernel<32, 8, false>) and extension form 2.
"""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import oracle
from bwagpu import abi
from bwagpu.engine import Batch, Engine, compact

pytestmark = pytest.mark.gpu

LN = 30  # seed length
KINDS = ("exact", "n3", "mm1n1", "mm1", "mm2", "del1")


def make_engine(refd, opt):
    return Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])


def run_device(eng, batch):
    """one batch through the device entry -> regs, n, the certificate's counters
    (bwagpu_debug_spec_ungapped: per round A, B, C the settled sides, their
    query lengths, the left and the right sides left on the phased lists)"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    fields = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev) for k in fields}
    out = torch.zeros(max(batch.n_seeds, 1) * 88, dtype=torch.uint8, device=dev)
    nn = torch.zeros(max(batch.n_reads, 1), dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    c.seq_bytes = int(batch.seq_off[-1])
    for k in fields:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), None, stream.cuda_stream)
    torch.cuda.synchronize()
    ctr = np.zeros(12, np.int64)
    assert eng.lib.bwagpu_debug_spec_ungapped(eng.ctx, C.c_void_p(stream.cuda_stream),
                                              ctr.ctypes.data_as(C.c_void_p)) == 0
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], ctr.reshape(3, 4)


@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_chain_sets_on_and_off(name):
    refd = G.load_ref()
    opt, batch, want, want_n = G.load_chain_set(name)
    ref = oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"])
    _, _, ost = oracle.chain2aln("oracle", opt, ref, batch)
    eng = make_engine(refd, opt)
    assert eng.ungapped() == 1 and eng.row_bound() == 1, "both switches start on"
    cells = {}
    for on in (1, 0):
        eng.ungapped(on)
        assert eng.ungapped() == on
        regs, n = eng.chain2aln(batch)
        assert np.array_equal(n, want_n), f"switch {on}: {int((n != want_n).sum())} reads with a different region count"
        assert G.region_mismatch(compact(batch, regs, n), want) is None, f"switch {on}"
        st = eng.last_stats()
        assert st["ext_calls"] == int(ost[2]), f"switch {on}: {st['ext_calls']} calls, the oracle makes {int(ost[2])}"
        assert st["cells"] <= int(ost[0]) and st["rows"] <= int(ost[1])
        cells[on] = st["cells"]
        dregs, dn, ctr = run_device(eng, batch)
        assert np.array_equal(dn, want_n) and G.region_mismatch(compact(batch, dregs, dn), want) is None
        print(f"{name}, switch {on}: cells {st['cells']} rows {st['rows']} calls {st['ext_calls']}; per round "
              f"[settled, their bases, left listed, right listed] {ctr.tolist()}")
        assert (ctr[:, 0].sum() > 0) == bool(on), f"switch {on}: {int(ctr[:, 0].sum())} sides settled"
    assert cells[1] < cells[0], f"cells {cells[1]} with the certificate, {cells[0]} without"
    # with the row bound off the certificate is off too: the counts are the oracle's own
    eng.ungapped(1)
    eng.row_bound(0)
    regs, n = eng.chain2aln(batch)
    st = eng.last_stats()
    assert G.region_mismatch(compact(batch, regs, n), want) is None
    assert (st["cells"], st["rows"], st["ext_calls"]) == tuple(int(x) for x in ost[:3])
    eng.close()


def flank(both, x0, n, kind):
    """n read bases aligned to the 2-strand coordinates x0 .. x0 + n - 1 (del1:
    to n + 1 of them, one left out in the middle; the caller passes an x0 that
    keeps the end next to the seed in place)"""
    if n == 0:
        return both[x0:x0].copy()
    if kind == "del1":
        d = n // 2
        return np.concatenate([both[x0:x0 + d], both[x0 + d + 1:x0 + n + 1]])
    fl = both[x0:x0 + n].copy()
    pos = [n // 4, n // 2, (3 * n) // 4]
    mm = {"exact": 0, "n3": 0, "mm1n1": 1, "mm1": 1, "mm2": 2, "del1": 0}[kind]
    ns = {"n3": 3, "mm1n1": 1}.get(kind, 0)
    for p in pos[:mm]:
        fl[p] = (fl[p] + 1) & 3
    for p in pos[mm:mm + ns]:
        fl[p] = 4
    return fl


def specs():
    """(left length, right length, left kind, right kind)"""
    out = [(20, 20, kl, kr) for kl in KINDS for kr in KINDS]  # every left/right combination of certified and DP
    some = [("exact", "exact"), ("mm1", "mm2"), ("mm2", "mm1"), ("n3", "mm1n1"), ("mm1n1", "n3"), ("del1", "exact"),
            ("exact", "del1")]
    for ql, qr in [(63, 64), (64, 63), (105, 12), (12, 105), (0, 40), (40, 0), (63, 0), (0, 64), (105, 0)]:
        out += [(ql, qr, kl if ql else "exact", kr if qr else "exact") for kl, kr in some]
    for ql, qr in [(1, 1), (1, 64), (63, 1), (0, 1), (1, 0), (0, 0)]:  # one base: exact or a mismatch
        out += [(ql, qr, kl if ql != 1 else kl1, kr if qr != 1 else kr1)
                for kl, kr, kl1, kr1 in [("exact", "exact", "exact", "mm1"), ("mm2", "n3", "mm1", "exact")]]
    return out


@pytest.fixture(scope="module")
def case():
    """-> refd, oracle.Ref, batch (one chain of one seed per read), per read:
    the left and right flanks' aligned reference bases and query bases (for the
    expected certificate), the left target length where the contig start cuts it"""
    refd = G.load_ref()
    l_pac, pac = refd["l_pac"], refd["pac"]
    x = np.arange(l_pac, dtype=np.int64)
    fwd = ((pac[x >> 2].astype(np.int64) >> ((~x & 3) << 1)) & 3).astype(np.uint8)
    both = np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])  # the 2-strand coordinate space
    seqs, seeds, rids, sides = [], [], [], []
    for i, (ql, qr, kl, kr) in enumerate(specs()):
        c = i % len(refd["ann_offset"])
        a0, al = int(refd["ann_offset"][c]), int(refd["ann_len"][c])
        f0 = a0 + 2000 + (7919 * i) % (al - 5000)  # the seed's first base, forward strand
        rev = i % 2 == 1
        rbeg = 2 * l_pac - (f0 + LN) if rev else f0
        left = flank(both, rbeg - ql - (1 if kl == "del1" and ql else 0), ql, kl)
        right = flank(both, rbeg + LN, qr, kr)
        seqs.append(np.concatenate([left, both[rbeg:rbeg + LN], right]))
        seeds.append((rbeg, ql, LN, LN, 0))
        rids.append(c)
        # diagonal pairs, from the seed outwards: (query, target); the target runs far past every query here
        sides.append(((left[::-1], both[rbeg - ql:rbeg][::-1], 1 << 20), (right, both[rbeg + LN:rbeg + LN + qr], 1 << 20)))
    # a read at a contig start: its left flank matches the bases in front of the contig, which are no
    # part of the chain's window; the left call has 5 target rows for 20 query bases
    a1 = int(refd["ann_offset"][1])
    rbeg, ql, qr = a1 + 5, 20, 20
    seqs.append(both[rbeg - ql:rbeg + LN + qr].copy())
    seeds.append((rbeg, ql, LN, LN, 0))
    rids.append(1)
    sides.append(((both[rbeg - ql:rbeg][::-1], both[rbeg - ql:rbeg][::-1], 5),
                  (both[rbeg + LN:rbeg + LN + qr], both[rbeg + LN:rbeg + LN + qr], 1 << 20)))
    n = len(seqs)
    assert n <= 256
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    batch = Batch(off, np.concatenate(seqs), np.arange(n + 1), np.arange(n + 1), np.array(rids, np.int32),
                  np.zeros(n, np.float32), np.array(seeds, abi.SEED_DTYPE))
    assert int(np.diff(off).max()) <= 160, "every read in the first length bin"
    ref = oracle.Ref(l_pac, refd["ann_offset"], refd["ann_len"], pac)
    return refd, ref, batch, sides


def expected_settled(opt, sides):
    """the certificate's conditions 1-5 on the batch's own bases -> the sides
    settled at sort time (a certified right side behind a left side that needs
    the DP stays on its list) and how many reads fall in each left/right class"""
    mat = np.asarray(opt["mat"] if opt.get("mat") is not None else abi.fill_scmat(opt["a"], opt["b"]), np.int64).reshape(5, 5)
    max_mat = int(max(0, mat.max()))
    oe_min = min(opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"])
    opt_ok = (LN * opt["a"] >= oe_min and (opt["zdrop"] <= 0 or opt["zdrop"] >= oe_min)
              and (opt["w"] >> 1) + (opt["w"] >> 2) > 0)

    def cert(q, t, tlen):
        return len(q) >= 1 and opt_ok and tlen >= len(q) and int((max_mat - mat[t, q]).sum()) < oe_min

    settled, classes = 0, {}
    for (lq, lt, ltl), (rq, rt, rtl) in sides:
        cl, cr = cert(lq, lt, ltl), cert(rq, rt, rtl)
        settled += int(cl) + int(cr and (len(lq) == 0 or cl))
        key = ("none" if len(lq) == 0 else "cert" if cl else "dp", "none" if len(rq) == 0 else "cert" if cr else "dp")
        classes[key] = classes.get(key, 0) + 1
    return settled, classes


def check(refd, ref, batch, sides, opt, what, form=None, kernel=None):
    oregs, on, ost = oracle.chain2aln("oracle", opt, ref, batch)
    want, classes = expected_settled(opt, sides)
    eng = make_engine(refd, opt)
    if form is not None:
        eng.ext_form(form)
    if kernel is not None:
        assert eng.ext_kernel(160) == eng.EXT_KERNELS[kernel], eng.ext_kernel(160)
    regs, n, ctr = run_device(eng, batch)
    print(f"{what}: classes {classes}; expected settled {want}; per round [settled, their bases, left listed, "
          f"right listed] {ctr.tolist()}")
    assert np.array_equal(n, on), f"{what}: {int((n != on).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    assert int(ctr[:, 0].sum()) == want, f"{what}: {int(ctr[:, 0].sum())} sides settled, {want} expected"
    regs, n = eng.chain2aln(batch)  # the host entry, whose statistics can be read
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    st = eng.last_stats()
    assert st["ext_calls"] == int(ost[2]) and st["cells"] <= int(ost[0]) and st["rows"] <= int(ost[1]), (st, ost)
    eng.close()
    return classes


def test_hand_made_batch(case):
    refd, ref, batch, sides = case
    opt = G.load_chain_set("c1_default")[0]
    classes = check(refd, ref, batch, sides, opt, "default options", kernel=18)
    for l in ("none", "cert", "dp"):  # every left/right combination occurs
        for r in ("none", "cert", "dp"):
            assert classes.get((l, r), 0) > 0, (l, r)


VARIANTS = {"zdrop_3": (dict(zdrop=3), None, 18),          # condition 4 fails: nothing settled
            "w_1": (dict(w=1), None, 18),                  # condition 5 fails: nothing settled
            "zdrop_oe_min": (dict(zdrop=7), None, 18),     # condition 4 at its edge
            "non_key8": (dict(a=2, b=5, o_del=7, e_del=2, o_ins=5, e_ins=3, pen_clip5=3, pen_clip3=9, w=30, zdrop=40),
                         None, 15),                        # spec_side4_kernel<32, 8, false>
            "form_2": (dict(), 2, 14)}                     # spec_side4_kernel<32, 5, true>


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hand_made_batch_variants(case, variant):
    refd, ref, batch, sides = case
    delta, form, kernel = VARIANTS[variant]
    opt = dict(G.load_chain_set("c1_default")[0], **delta)
    if "a" in delta:
        opt["mat"] = abi.fill_scmat(opt["a"], opt["b"]).reshape(-1)
    check(refd, ref, batch, sides, opt, variant, form=form, kernel=kernel)
    if variant in ("zdrop_3", "w_1"):
        assert expected_settled(opt, sides)[0] == 0
