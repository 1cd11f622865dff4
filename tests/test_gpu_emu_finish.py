"""The emulate selection pass finishes decided light reads (Engine.emu_finish(1),
the default): a light read it leaves no round-B task gets its
regions there, the others are listed, and the final light pass takes only the
list.  0: the final pass takes every light read, as before.

Expected regions come from the CPU oracle (oracle.chain2aln("oracle", ...)),
the golden vectors or the fixture's recorded digest, never from the code under
test; every case runs with the switch at 1 and at 0:

* batches of 1, 7, 8, 9 and 17 fixture reads, with light_pack 1 and 0;
* list shapes through the device entry, out_n prefilled with -7 and out with
  0xFF: every read finished, every read listed, one mixed octet (each read as in
  a batch alone), a batch without chains, one read without a seed;
* a list count or a finished bit that survives a batch: listed, finished and
  listed again on one context and stream;
* every golden chain set;
* tests/gpu_variant_child.py under BWAGPU_EMU_STRICT=0, BWAGPU_LIGHT_RISKY_FIRST=1
  and BWAGPU_LIGHT_PACK=0;
* the first 4,096 fixture reads: the same tasks, inline extensions and DP work
  with the switch on and off, and bwagpu_debug_spec_finish's counts against
  bounds restated in numpy;
* the whole first fixture batch against its recorded digest.
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
K_LIGHT, K_PACK = 64, 8  # kSelLight, kPackW (csrc/engine.h, csrc/spec.hip)


@pytest.fixture(scope="module")
def fixture():
    """-> opt, GoldenRef, oracle.Ref, the C2 fixture's first batch, its seeds and chains per read, the
    reference's regions per read"""
    opt, ref, rbs = workload.load_fixture()
    b = rbs[0].batch
    nch = np.diff(b.read_chain_off)
    ns = np.diff(b.chain_seed_off[b.read_chain_off])
    return opt, ref, oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac), b, ns, nch, rbs[0].reg_n.astype(np.int64)


def make_engine(opt, ref, knob, light_pack=None):
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    eng.emu_finish(knob)
    assert eng.emu_finish() == knob
    if light_pack is not None:
        eng.light_pack(light_pack)
    return eng


def check_oracle(eng, opt, oref, batch, what):
    """the batch through the host entry against the oracle -> per-read region arrays"""
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, batch)
    regs, n = eng.chain2aln(batch)
    assert np.array_equal(n, on), f"{what}: {int((n != on).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    return unflatten(batch, regs, n)


def pick(mask, k=0):
    """the k-th read of the fixture batch with the property"""
    idx = np.flatnonzero(mask)
    assert len(idx) > k, "the fixture has no such read"
    return int(idx[k])


def run_device(eng, batch):
    """one batch through the device entry, out_n prefilled with -7 and out with 0xFF -> regs, n,
    bwagpu_debug_spec_counters' eight words, bwagpu_debug_spec_finish's four, the four stats words"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    fields = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev) for k in fields}
    out = torch.full((max(batch.n_seeds, 1) * 88,), 0xFF, dtype=torch.uint8, device=dev)
    nn = torch.full((max(batch.n_reads, 1),), -7, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    c.seq_bytes = int(batch.seq_off[-1])
    for k in fields:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), stats.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    sc, fc = np.zeros(8, np.int64), np.zeros(4, np.int64)
    assert eng.lib.bwagpu_debug_spec_counters(eng.ctx, C.c_void_p(stream.cuda_stream),
                                              sc.ctypes.data_as(C.c_void_p)) == 0
    assert eng.lib.bwagpu_debug_spec_finish(eng.ctx, C.c_void_p(stream.cuda_stream),
                                            fc.ctypes.data_as(C.c_void_p)) == 0
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], sc, fc, stats.cpu().numpy()


def check_device(eng, opt, oref, batch, what):
    """the batch through the device entry against the oracle -> per-read region arrays, the finish counters"""
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, batch)
    regs, n, _, fc, _ = run_device(eng, batch)
    assert np.array_equal(n, on), f"{what}: region counts {n.tolist()[:32]} against {on.tolist()[:32]}"
    assert G.region_mismatch(compact(batch, regs, n), compact(batch, oregs, on)) is None, what
    return unflatten(batch, regs, n), fc


def test_knob_range(fixture):
    opt, ref = fixture[0], fixture[1]
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    assert eng.emu_finish() == 1 or os.environ.get("BWAGPU_EMU_FINISH", "")[:1] == "0"  # default on
    eng.emu_finish(1)
    assert eng.emu_finish(-1) == 1 and eng.emu_finish(0) == 1 and eng.emu_finish() == 0
    assert eng.emu_finish(5) == 0 and eng.emu_finish() == 1  # any other value counts as on
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("light_pack", [1, 0])
@pytest.mark.parametrize("n_reads", [1, 7, 8, 9, 17])
def test_octet_edges(fixture, n_reads, light_pack, knob):
    opt, ref, oref, b, ns = fixture[:5]
    # from the first read on that has a seed: a batch of one read is not an empty one
    first = int(np.flatnonzero(ns > 0)[0])
    sub = b.subset(range(first, first + n_reads))
    eng = make_engine(opt, ref, knob, light_pack)
    check_oracle(eng, opt, oref, sub, f"{n_reads} reads, light_pack {light_pack}, emu_finish {knob}")
    eng.close()


def classes(ns, nch, reg_n):
    """masks over the fixture's reads: narrow, wide light, and of the light ones those that are surely
    finished (every chain has one seed: round A extends every chain's first seed) and surely pending (the
    reference extends more seeds than the read has chains, so one that is not a chain's first)"""
    light = (ns <= K_LIGHT) & (nch <= K_LIGHT)
    narrow = (ns <= K_PACK) & (nch <= K_PACK)
    sure_fin = light & (ns == nch)
    sure_pend = light & (reg_n > nch)
    return light, narrow, sure_fin, sure_pend


def finished_batch(b, ns, nch, reg_n):
    light, narrow, sure_fin, _ = classes(ns, nch, reg_n)
    return b.subset([pick(narrow & sure_fin & (ns > 0), k) for k in range(9)])


def listed_batch(b, ns, nch, reg_n):
    light, narrow, _, sure_pend = classes(ns, nch, reg_n)
    return b.subset([pick(narrow & sure_pend, k) for k in range(9)])


@pytest.mark.parametrize("knob", KNOBS)
def test_every_read_finished(fixture, knob):
    opt, ref, oref, b, ns, nch, reg_n = fixture
    eng = make_engine(opt, ref, knob)
    _, fc = check_device(eng, opt, oref, finished_batch(b, ns, nch, reg_n), f"nine finished reads, emu_finish {knob}")
    eng.close()
    print("finish counters:", fc.tolist())
    assert fc.tolist() == ([9, 0, 0, 9] if knob else [0, 0, 0, 0])


@pytest.mark.parametrize("knob", KNOBS)
def test_every_read_listed(fixture, knob):
    opt, ref, oref, b, ns, nch, reg_n = fixture
    eng = make_engine(opt, ref, knob)
    _, fc = check_device(eng, opt, oref, listed_batch(b, ns, nch, reg_n), f"nine listed reads, emu_finish {knob}")
    eng.close()
    print("finish counters:", fc.tolist())
    assert fc.tolist() == ([0, 0, 9, 9] if knob else [0, 0, 0, 0])


@pytest.mark.parametrize("knob", KNOBS)
def test_mixed_octet(fixture, knob):
    opt, ref, oref, b, ns, nch, reg_n = fixture
    light, narrow, sure_fin, sure_pend = classes(ns, nch, reg_n)
    wide = light & ~narrow
    octet = b.subset([pick(narrow & sure_fin & (ns > 0)), pick(narrow & sure_pend), pick(wide & sure_fin & (ns >= 9)),
                      pick(wide & sure_pend), pick(ns > K_LIGHT), pick(ns == 0), pick(narrow & (ns == 3)),
                      pick(narrow & (ns == 8))])
    assert octet.n_reads == 8
    eng = make_engine(opt, ref, knob)
    per_read, fc = check_device(eng, opt, oref, octet, f"mixed octet, emu_finish {knob}")
    print("finish counters:", fc.tolist())
    if knob:
        assert fc[3] == 7 and fc[0] + fc[1] + fc[2] == 7  # the heavy read is not a light one
        assert fc[0] >= 2 and fc[1] >= 1 and fc[2] >= 2  # finished: narrow, empty; wide.  listed: one of each width
    for i in range(8):
        alone, _ = check_device(eng, opt, oref, octet.subset([i]), f"mixed octet's read {i} alone, emu_finish {knob}")
        assert per_read[i].tobytes() == alone[0].tobytes(), f"read {i} differs beside the others"
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("n_reads", [1, 9])
def test_no_chains(fixture, n_reads, knob):
    """no chain in the batch: no emulate pass runs, and the final pass takes every read"""
    opt, ref, oref, b, ns, nch, reg_n = fixture
    sub = b.subset([pick(nch == 0, k) for k in range(n_reads)])
    assert sub.n_chains == 0 and sub.n_seeds == 0
    eng = make_engine(opt, ref, knob)
    _, n, _, fc, _ = run_device(eng, sub)
    eng.close()
    assert n.tolist() == [0] * n_reads
    assert fc.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("knob", KNOBS)
def test_stale_state(fixture, knob):
    """listed, finished, listed again on one context and stream: the list count and the finished bits are
    per batch"""
    opt, ref, oref, b, ns, nch, reg_n = fixture
    lst, fin = listed_batch(b, ns, nch, reg_n), finished_batch(b, ns, nch, reg_n)
    eng = make_engine(opt, ref, knob)
    for step, (sub, want) in enumerate([(lst, [0, 0, 9, 9]), (fin, [9, 0, 0, 9]), (lst, [0, 0, 9, 9])]):
        _, fc = check_device(eng, opt, oref, sub, f"step {step}, emu_finish {knob}")
        assert fc.tolist() == (want if knob else [0, 0, 0, 0]), f"step {step}"
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_golden_chain_sets(name, knob):
    refd = G.load_ref()
    opt, batch, want, want_n = G.load_chain_set(name)
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    eng.emu_finish(knob)
    regs, n = eng.chain2aln(batch)
    assert np.array_equal(n, want_n), f"{int((n != want_n).sum())} reads with a different region count"
    assert G.region_mismatch(compact(batch, regs, n), want) is None
    eng.close()


@pytest.mark.parametrize("var", ["BWAGPU_EMU_STRICT=0", "BWAGPU_LIGHT_RISKY_FIRST=1", "BWAGPU_LIGHT_PACK=0"])
def test_variants(var):
    """the other forms of the two light passes with the switch on, each in a child process (the library
    reads these knobs once): the fixtures' batches against the reference's regions"""
    k, v = var.split("=")
    env = dict(os.environ, BWAGPU_EMU_FINISH="1", **{k: v})
    p = subprocess.run([sys.executable, os.path.join(HERE, "gpu_variant_child.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["c2"] and all(r["c2"]), r
    assert r["c5"] and all(r["c5"]), r


def test_counters_and_work(fixture):
    """4,096 fixture reads: the same tasks in every round, the same inline extensions and the same DP work
    with the switch on and off; regions from the oracle; the finish counters within what the batch and the
    oracle's region counts bound"""
    opt, ref, oref, b, ns, nch, reg_n = fixture
    k = 4096
    sub = b.subset(range(k))
    oregs, on, _ = oracle.chain2aln("oracle", opt, oref, sub)
    want = compact(sub, oregs, on)
    light, narrow, sure_fin, sure_pend = classes(ns[:k], nch[:k], on.astype(np.int64))
    res = {}
    for knob in KNOBS:
        eng = make_engine(opt, ref, knob)
        regs, n, sc, fc, st = run_device(eng, sub)
        eng.close()
        assert np.array_equal(n, on), f"emu_finish {knob}: {int((n != on).sum())} reads with a different region count"
        assert G.region_mismatch(compact(sub, regs, n), want) is None, f"emu_finish {knob}"
        res[knob] = (sc, fc, st)
        print(f"emu_finish {knob}: spec counters {sc.tolist()}, finish counters {fc.tolist()}, stats {st.tolist()}")
    for w, what in ((0, "round-A tasks"), (1, "round-B tasks"), (2, "round-C tasks"), (4, "inline extensions"),
                    (5, "heavy reads"), (6, "reads left to the redo pass")):
        assert res[1][0][w] == res[0][0][w], f"{what}: {int(res[1][0][w])} on, {int(res[0][0][w])} off"
    assert res[1][2][:3].tolist() == res[0][2][:3].tolist(), "cells, rows, calls"
    assert res[1][2][3] == 0 and res[0][2][3] == 0
    assert res[1][2][0] > 0
    fc = res[1][1]
    assert res[0][1].tolist() == [0, 0, 0, 0]
    assert fc[0] + fc[1] + fc[2] == fc[3]
    assert fc[3] == int(light.sum())
    assert fc[0] + fc[1] >= int(sure_fin.sum())
    assert fc[2] >= int(sure_pend.sum())
    assert fc[2] < fc[3], "every read listed: nothing compared"


def test_whole_batch():
    """all 66,668 reads of the fixture's first batch: the list-driven stride loop runs more than one unit
    per wave"""
    opt, ref, rbs = workload.load_fixture()
    eng = make_engine(opt, ref, 1)
    assert rbs[0].check(*eng.chain2aln(rbs[0].batch))
    eng.close()
