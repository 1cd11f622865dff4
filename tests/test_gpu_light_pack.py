"""The packed light selection: spec_select_light runs the reads with at most
eight seeds and eight chains eight per wave, in groups of eight lanes
(Engine.light_pack(1), the default; 0: every light read has a wave of its own).

Expected regions come from the CPU oracle (oracle.chain2aln("oracle", ...)) or
the golden vectors, never from the code under test; every case runs with the
switch at 1 and at 0:

* batches of 1, 7, 8, 9 and 17 reads cut from the C2 fixture (a partial last
  octet, one octet exactly, one read over);
* one octet of fixture reads with 0, 1, 7, 8 and 9 seeds and a heavy read
  (> 64 seeds), and one with eight chains beside nine (fixture reads, and a
  read cut down to one seed in each of eight and of nine chains): the narrow
  reads beside the wider ones of their wave must give what they give alone;
* every golden chain set (pad seeds, flagged chain windows, other scoring and
  band options);
* BWAGPU_EMU_STRICT=0 in a child process (tests/gpu_variant_child.py): there
  the final pass finds seeds without a result, also in narrow reads;
* the first 4,096 reads of the fixture's first batch through the device entry:
  the round-B and round-C task counts and the inline extensions are those of
  the run with the switch at 0 (the emulation predicts the same).
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
from bwagpu.engine import Batch, Engine, compact, unflatten

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = [1, 0]


@pytest.fixture(scope="module")
def fixture():
    """-> opt, GoldenRef, oracle.Ref, the C2 fixture's first batch, its seeds and chains per read"""
    opt, ref, rbs = workload.load_fixture()
    b = rbs[0].batch
    nch = np.diff(b.read_chain_off)
    ns = np.diff(b.chain_seed_off[b.read_chain_off])
    return opt, ref, oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac), b, ns, nch


def make_engine(opt, ref, knob):
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    eng.light_pack(knob)
    assert eng.light_pack() == knob
    return eng


def check_oracle(eng, opt, oref, batch, what):
    """the batch through the host entry against the oracle -> per-read region arrays"""
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, batch)
    regs, n = eng.chain2aln(batch)
    assert np.array_equal(n, on), f"{what}: {int((n != on).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    return unflatten(batch, regs, n)


def test_knob_range(fixture):
    opt, ref = fixture[0], fixture[1]
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    eng.light_pack(1)
    assert eng.light_pack(-1) == 1 and eng.light_pack(0) == 1 and eng.light_pack() == 0
    assert eng.light_pack(5) == 0 and eng.light_pack() == 1  # any other value counts as on
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("n_reads", [1, 7, 8, 9, 17])
def test_octet_edges(fixture, n_reads, knob):
    opt, ref, oref, b, ns, nch = fixture
    # from the first read on that has a seed: a batch of one read is not an empty one
    first = int(np.flatnonzero(ns > 0)[0])
    sub = b.subset(range(first, first + n_reads))
    eng = make_engine(opt, ref, knob)
    check_oracle(eng, opt, oref, sub, f"{n_reads} reads, light_pack {knob}")
    eng.close()


def pick(mask, k=0):
    """the k-th read of the fixture batch with the property"""
    idx = np.flatnonzero(mask)
    assert len(idx) > k, "the fixture has no such read"
    return int(idx[k])


def one_seed_per_chain(b, read, n_chains):
    """the read cut down to the first seed of each of its first n_chains chains"""
    c0 = int(b.read_chain_off[read])
    assert int(b.read_chain_off[read + 1]) - c0 >= n_chains
    chains = np.arange(c0, c0 + n_chains)
    lq = int(b.seq_off[read + 1] - b.seq_off[read])
    return Batch(np.array([0, lq]), b.seq[b.seq_off[read]:b.seq_off[read + 1]].copy(), np.array([0, n_chains]),
                 np.arange(n_chains + 1), b.chain_rid[chains].astype(np.int32),
                 b.chain_frac_rep[chains].astype(np.float32), b.seeds[b.chain_seed_off[chains]].copy())


def concat(batches):
    """the batches' reads in one batch, in order"""
    seq_off, rco, cso = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)]
    for x in batches:
        seq_off.append(np.asarray(x.seq_off[1:], np.int64) + seq_off[-1][-1])
        rco.append(np.asarray(x.read_chain_off[1:], np.int64) + rco[-1][-1])
        cso.append(np.asarray(x.chain_seed_off[1:], np.int64) + cso[-1][-1])
    return Batch(np.concatenate(seq_off), np.concatenate([x.seq for x in batches]), np.concatenate(rco),
                 np.concatenate(cso), np.concatenate([x.chain_rid for x in batches]).astype(np.int32),
                 np.concatenate([x.chain_frac_rep for x in batches]).astype(np.float32),
                 np.concatenate([x.seeds for x in batches]))


def mixed_octets(b, ns, nch):
    """-> (name, batch of eight reads: one wave's octet, its narrow reads' positions)"""
    light = nch <= 8
    seeds = b.subset([pick(ns == 0), pick((ns == 1) & light), pick((ns == 7) & light), pick((ns == 8) & light),
                      pick((ns == 9) & light), pick(ns > 64), pick((ns == 8) & light, 1), pick((ns == 2) & light)])
    many = pick((nch >= 9) & (ns <= 64))
    chains = concat([b.subset([pick((nch == 8) & (ns <= 64)), pick((nch == 9) & (ns <= 64))]),
                     one_seed_per_chain(b, many, 8), one_seed_per_chain(b, many, 9), one_seed_per_chain(b, many, 7),
                     b.subset([pick((ns == 3) & light), pick((ns == 8) & light), pick((ns == 1) & light, 1)])])
    return [("seeds", seeds, [0, 1, 2, 3, 6, 7]), ("chains", chains, [2, 4, 5, 6, 7])]


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("which", [0, 1])
def test_width_edges_in_one_wave(fixture, which, knob):
    opt, ref, oref, b, ns, nch = fixture
    name, octet, narrow = mixed_octets(b, ns, nch)[which]
    assert octet.n_reads == 8
    ons = np.diff(octet.chain_seed_off[octet.read_chain_off])
    onch = np.diff(octet.read_chain_off)
    if which == 0:
        assert ons.tolist()[:5] == [0, 1, 7, 8, 9] and ons[5] > 64
    else:
        assert onch.tolist()[:5] == [8, 9, 8, 9, 7] and ons.tolist()[2:5] == [8, 9, 7]
    assert all(ons[i] <= 8 and onch[i] <= 8 for i in narrow)
    eng = make_engine(opt, ref, knob)
    per_read = check_oracle(eng, opt, oref, octet, f"octet '{name}', light_pack {knob}")
    # the narrow reads alone: a wave of narrow reads only
    alone = octet.subset(narrow)
    per_alone = check_oracle(eng, opt, oref, alone, f"octet '{name}' narrow reads alone, light_pack {knob}")
    for k, i in enumerate(narrow):
        assert per_read[i].tobytes() == per_alone[k].tobytes(), f"octet '{name}': read {i} differs beside wider reads"
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_golden_chain_sets(name, knob):
    refd = G.load_ref()
    opt, batch, want, want_n = G.load_chain_set(name)
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    eng.light_pack(knob)
    regs, n = eng.chain2aln(batch)
    assert np.array_equal(n, want_n), f"{int((n != want_n).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), want) is None
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
def test_strict_emulation_off(knob):
    """BWAGPU_EMU_STRICT=0: the final pass meets seeds without a result; a
    narrow read's miss goes the one-read-per-wave way (the inline extension, or
    the redo list for the C5 fixture's long reads)"""
    env = dict(os.environ, BWAGPU_EMU_STRICT="0", BWAGPU_LIGHT_PACK=str(knob))
    p = subprocess.run([sys.executable, os.path.join(HERE, "gpu_variant_child.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["c2"] and all(r["c2"]), r
    assert r["c5"] and all(r["c5"]), r


def run_device(eng, batch):
    """one batch through the device entry -> regs, n, bwagpu_debug_spec_counters' eight words"""
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
    sc = np.zeros(8, np.int64)
    assert eng.lib.bwagpu_debug_spec_counters(eng.ctx, C.c_void_p(stream.cuda_stream),
                                              sc.ctypes.data_as(C.c_void_p)) == 0
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], sc


def test_predictions_unchanged(fixture):
    """4,096 fixture reads: the same tasks in every round and no more inline
    extensions than with one read per wave; regions from the oracle"""
    opt, ref, oref, b, ns, nch = fixture
    sub = b.subset(range(4096))
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, sub)
    want = compact(sub, oregs, on)
    counters = {}
    for knob in KNOBS:
        eng = make_engine(opt, ref, knob)
        regs, n, sc = run_device(eng, sub)
        eng.close()
        assert np.array_equal(n, on), f"light_pack {knob}: {int((n != on).sum())} reads with a different region count"
        assert G.region_mismatch(compact(sub, regs, n), want) is None, f"light_pack {knob}"
        counters[knob] = sc
    print("spec counters, light_pack 1:", counters[1].tolist(), " 0:", counters[0].tolist())
    assert counters[1][1] > 0, "the emulate pass left no round-B task: nothing compared"
    for w, what in ((0, "round-A tasks"), (1, "round-B tasks"), (2, "round-C tasks"), (4, "inline extensions"),
                    (5, "heavy reads"), (6, "reads left to the redo pass")):
        assert counters[1][w] == counters[0][w], f"{what}: {int(counters[1][w])} packed, {int(counters[0][w])} not"
