"""GPU parity of the region post-processing (bwagpu_regs_post*,
bwagpu_set_regs_post): mem_sort_dedup_patch and the is_alt flag on the
device (flags 1|2; BWAGPU_POST_PRIMARY is refused), byte for byte against the
reference's own
results (tests/golden/post_*.npz), through the host entry, the device entry
behind bwagpu_chain2aln_device, and the switch of the submit / seqs2regions
entries; hand-built cases; the error paths."""
import numpy as np
import pytest

import golden_io as G
import post_io as P
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine, compact

pytestmark = pytest.mark.gpu

_engines = {}


def engine(opt, genome=0, alt=None) -> Engine:
    """one context per (genome, scoring options), shared by the module's tests"""
    key = (genome, tuple(int(opt[k]) for k in G.OPT_KEYS), bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        g = P.genome(genome)
        _engines[key] = Engine(0, opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    e = _engines[key]
    e.set_alt(alt)
    e.set_regs_post(0)
    return e


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def check(got_regs, got_n, want, what):
    want_regs, want_n = want
    assert np.array_equal(got_n, want_n), f"{what}: per-read counts differ at reads " \
        f"{np.nonzero(got_n != want_n)[0][:8].tolist()}"
    bad = G.region_mismatch(got_regs, want_regs)
    assert bad is None, f"{what}: {bad}"


@pytest.mark.parametrize("flags", [3])
@pytest.mark.parametrize("name", P.POST_SETS)
def test_regs_post_matches_the_reference(name, flags):
    s = P.load(name)
    eng = engine(s.opt, s.genome, s.alt)
    regs, n = eng.regs_post(s.seq_off, s.seq, s.off, s.regs, s.n, flags, s.id0, s.popt)
    check(P.dense(regs, s.off, n), n, s.want[flags], f"{name} flags {flags}")
    st = eng.last_stats()
    assert st["kernel_ms"] > 0
    if s.coverage["regs_patched"]:
        assert st["ext_calls"] >= s.coverage["regs_patched"]


def _device_batch(torch, batch):
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev)
         for k in ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")}
    bc = abi.BatchC()
    bc.n_reads, bc.n_chains, bc.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    bc.seq_bytes = int(batch.seq_off[-1])
    for k in t:
        setattr(bc, k, t[k].data_ptr())
    return bc, t


@pytest.mark.parametrize("name", ["c1_default", "sv"])
def test_chain2aln_device_then_regs_post_device(name):
    """on the same stream, in place on what bwagpu_chain2aln_device wrote: the slot
    layout (dev_reg_off = NULL), then the same regions packed densely with offsets"""
    torch = pytest.importorskip("torch")
    s = P.load(name)
    batch = s.batch if s.batch is not None else G.load_chain_set(name)[1]
    eng = engine(s.opt, s.genome, s.alt)
    dev = torch.device("cuda", 0)
    bc, keep = _device_batch(torch, batch)
    out = torch.zeros(max(batch.n_seeds, 1) * 88, dtype=torch.uint8, device=dev)
    n = torch.zeros(batch.n_reads, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    eng.chain2aln_device(bc, out.data_ptr(), n.data_ptr(), None, stream.cuda_stream)
    stream.synchronize()
    raw, raw_n = out.cpu().numpy().view(abi.ALNREG_DTYPE).copy(), n.cpu().numpy().copy()
    assert np.array_equal(raw_n, s.n) and G.region_mismatch(compact(batch, raw, raw_n), s.regs) is None
    eng.chain2aln_device(bc, out.data_ptr(), n.data_ptr(), None, stream.cuda_stream)
    eng.regs_post_device(bc, None, out.data_ptr(), n.data_ptr(), 3, s.id0, s.popt, stream.cuda_stream)
    stream.synchronize()
    got_n = n.cpu().numpy()
    check(compact(batch, out.cpu().numpy().view(abi.ALNREG_DTYPE), got_n), got_n, s.want[3], f"{name} slot layout")
    # dense offsets
    d_regs = torch.from_numpy(s.regs.view(np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(s.off.copy()).to(dev)
    d_n = torch.from_numpy(s.n.copy()).to(dev)
    eng.regs_post_device(bc, d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), 3, s.id0, s.popt,
                         stream.cuda_stream)
    stream.synchronize()
    got_n = d_n.cpu().numpy()
    check(P.dense(d_regs.cpu().numpy().view(abi.ALNREG_DTYPE), s.off, got_n), got_n, s.want[3], f"{name} dense")
    del keep


def test_switch_on_chain2aln_and_submit_wait():
    """bwagpu_set_regs_post: chain2aln and submit / wait_dense return what the plain
    call followed by regs_post returns; flags 0 restores the plain output byte for byte"""
    s = P.load("c1_default")
    opt, batch, raw_want, raw_n_want = G.load_chain_set("c1_default")
    eng = engine(opt, 0, s.alt)
    raw, raw_n = eng.chain2aln(batch)
    plain = compact(batch, raw, raw_n)
    assert G.region_mismatch(plain, raw_want) is None
    off = G.offsets(raw_n)
    for flags in (1, 3):
        want_regs, want_n = eng.regs_post(batch.seq_off, batch.seq, off, plain, raw_n, flags, 4242, s.popt)
        want = (P.dense(want_regs, off, want_n), want_n)
        eng.set_regs_post(flags, 4242, s.popt)
        regs, n = eng.chain2aln(batch)
        check(compact(batch, regs, n), n, want, f"chain2aln, flags {flags}")
        eng.set_regs_post(flags, 4242, s.popt)
        eng.submit(1, batch)
        dregs, dn = eng.wait_dense(1, batch)
        check(dregs.copy(), dn.copy(), want, f"submit / wait_dense, flags {flags}")
        assert eng.last_stats(1)["d2h_bytes"] < 88 * int(raw_n.sum()) + 8 * batch.n_reads + 4
        eng.set_regs_post(0)
        regs, n = eng.chain2aln(batch)
        assert np.array_equal(n, raw_n) and regs.tobytes() == raw.tobytes()


def test_switch_on_seqs2regions():
    cg = G.load_chain_gold("c1")
    eng = engine(cg["opt"], 0, cg["is_alt"])
    hdr, words = G.load_seed_bwt()
    sa_intv, sa, _, _ = G.load_seed_sa()
    eng.set_bwt(hdr, words, sa, sa_intv)
    nr = 600
    seq_off, seq = cg["seq_off"][:nr + 1], cg["seq"][:int(cg["seq_off"][nr])]
    raw_n, raw = eng.seqs2regions(seq_off, seq, cg["seedopt"], cg["split_factor"], cg["copt"])
    off = G.offsets(raw_n)
    popt = abi.default_postopt()
    want_regs, want_n = eng.regs_post(seq_off, seq, off, raw, raw_n, 3, 99, popt)
    eng.set_regs_post(3, 99, popt)
    n, regs = eng.seqs2regions(seq_off, seq, cg["seedopt"], cg["split_factor"], cg["copt"])
    check(regs, n, (P.dense(want_regs, off, want_n), want_n), "seqs2regions")
    assert int(want_n.sum()) < int(raw_n.sum())
    eng.set_regs_post(0)
    n, regs = eng.seqs2regions(seq_off, seq, cg["seedopt"], cg["split_factor"], cg["copt"])
    assert np.array_equal(n, raw_n) and regs.tobytes() == raw.tobytes()


# ---------------------------------------------------------------- hand-built cases
def _reg(rb, re, qb, qe, rid=0, score=None, **kw):
    r = np.zeros(1, abi.ALNREG_DTYPE)
    r["rb"], r["re"], r["qb"], r["qe"], r["rid"] = rb, re, qb, qe, rid
    r["score"] = r["truesc"] = (qe - qb) if score is None else score
    r["w"] = 100
    r["secondary"] = -1
    for k, v in kw.items():
        r[k] = v
    return r


def _hand(eng, reads, flags=1, l_seq=100):
    """reads: a list of per-read region lists -> per-read surviving regions"""
    n = np.array([len(r) for r in reads], np.int32)
    off = G.offsets(n)
    regs = np.concatenate([x for r in reads for x in r]) if n.sum() else np.zeros(0, abi.ALNREG_DTYPE)
    seq_off = np.arange(len(reads) + 1, dtype=np.int64) * l_seq
    seq = np.zeros(int(seq_off[-1]), np.uint8)
    out, m = eng.regs_post(seq_off, seq, off, regs, n, flags)
    return [out[o:o + k] for o, k in zip(off, m)], regs


def test_hand_built_cases():
    eng = engine(abi.default_opt())
    # empty batch
    out, n = eng.regs_post(np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int64),
                           np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32), 3)
    assert len(out) == 0 and len(n) == 0
    a = _reg(1000, 1100, 0, 100)
    hi = _reg(5000, 5100, 0, 100, score=90)     # ends later, lower score
    lo = _reg(4998, 5098, 0, 100, score=95)     # 98 % overlap with hi, higher score
    tie_a = _reg(7000, 7100, 0, 100, score=80, seedcov=1)
    tie_b = _reg(7001, 7101, 0, 100, score=80, seedcov=2)  # later in re order: line 465's `<` keeps it
    other = _reg(1001, 1101, 0, 100, rid=1)     # 99 % overlap with a, on another contig
    twin = _reg(1000, 1100, 0, 100, rid=1)      # a's score, rb and qb on another contig
    got, _ = _hand(eng, [[], [a], [a, a.copy()], [hi, lo], [tie_a, tie_b], [a, other], [lo, hi], [a, twin]])
    assert len(got[0]) == 0
    assert len(got[1]) == 1 and got[1].tobytes() == a.tobytes()  # n = 1: untouched, n_comp stays 0
    assert len(got[2]) == 1                                      # two identical regions give one
    one = a.copy()
    one["n_comp_is_alt"] = 1
    assert got[2].tobytes() == one.tobytes()
    assert len(got[3]) == 1 and got[3]["score"][0] == 95 and got[3]["rb"][0] == 4998
    assert len(got[6]) == 1 and got[6]["score"][0] == 95
    assert len(got[4]) == 1 and got[4]["seedcov"][0] == 2 and got[4]["re"][0] == 7101
    assert len(got[5]) == 2                                      # different rid never interact
    assert sorted(got[5]["rid"].tolist()) == [0, 1] and (got[5]["n_comp_is_alt"] == 1).all()
    assert len(got[7]) == 1  # ... except in the second pass, whose identical-hit test reads no rid (bwamem.c:489)
    # flags 2 with no ALT table sets no bit
    eng.set_alt(None)
    got, _ = _hand(eng, [[a], [a, other]], flags=3)
    assert all((g["n_comp_is_alt"] >> np.uint32(30) == 0).all() for g in got)
    eng.set_alt(np.array([0, 1, 0], np.uint8))
    got, _ = _hand(eng, [[other], [a, other]], flags=2)
    assert got[0]["n_comp_is_alt"][0] == 1 << 30
    assert sorted((got[1]["n_comp_is_alt"] >> np.uint32(30)).tolist()) == [0, 1] and len(got[1]) == 2


def test_errors_launch_nothing():
    eng = engine(abi.default_opt())
    a = _reg(1000, 1100, 0, 100)
    _hand(eng, [[a, a.copy()]])  # a finished pass: its stats are what must stay
    before = eng.last_stats()
    regs = np.concatenate([a, a])
    seq_off = np.array([0, 100], np.int64)
    seq = np.zeros(2000, np.uint8)

    def code(*args, **kw):
        with pytest.raises(BwaGpuError) as e:
            eng.regs_post(*args, **kw)
        return e.value.code

    assert code(np.array([0, 1024], np.int64), seq, [0], regs, [2], 1) == abi.E_UNSUPPORTED
    assert code(seq_off, seq, [0], regs, [-1], 1) == abi.E_INVAL                    # negative count
    assert code(np.array([0, 100, 200], np.int64), seq, [0, 1], np.concatenate([regs, a]), [2, 2], 1) == abi.E_INVAL
    assert code(seq_off, seq, [-1], regs, [2], 1) == abi.E_INVAL                    # span before the array
    bad = regs.copy()
    bad["qe"][1] = 101
    assert code(seq_off, seq, [0], bad, [2], 1) == abi.E_INVAL                      # qe outside the read
    bad["qe"][1], bad["qb"][1] = 100, -1
    assert code(seq_off, seq, [0], bad, [2], 1) == abi.E_INVAL
    assert code(seq_off, seq, [0], regs, [2], 8) == abi.E_INVAL                     # unknown flag
    assert code(seq_off, seq, [0], regs, [2], 7) == abi.E_UNSUPPORTED               # BWAGPU_POST_PRIMARY: reserved
    with pytest.raises(BwaGpuError) as e:
        eng.set_regs_post(4)
    assert e.value.code == abi.E_UNSUPPORTED
    assert code(np.array([100, 0], np.int64), seq, [0], regs, [2], 1) == abi.E_INVAL
    assert eng.last_stats() == before
