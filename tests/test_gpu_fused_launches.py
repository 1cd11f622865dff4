"""Fused launches of a batch's chain2aln (Engine.fused_launches,
a bit mask, default 5: bit 2 measured no gain and starts off): 1 = the side lists' sort in two launches per round (the
certificate kernel counts, the scatter scans), 2 = the late right sides on the
side stream beside the right launch, 4 = heavy reads without a pair matrix
inside the matrix scan's launch.  Mask 0 is the launch sequence without them.

Every case runs at mask 0, at 7, at the default 5 and with each bit alone, through the device
entry with its outputs prefilled.  Regions must be the CPU oracle's
(oracle.chain2aln("oracle", ...)) at every mask, byte for byte, and the
counters (bwagpu_debug_spec_counters, _spec_ungapped, _spec_ungapped_right,
_spec_short) must not depend on the mask.

* the sort stage: hand-made batches on the golden genome, one chain of one seed
  per read, so round A's first-bin list has one task per read: 0 (a batch
  without chains), 1, 255, 256, 257 and 2,049 tasks; every side in one key;
  sides of every length a 150 bp read leaves beside a 19-base seed (0 .. 131
  bases, keys 124 .. 255; a shorter seed would reach a few keys more, which the
  two_bins case's sides of 160 bases and the one_key case pass on either side
  of); a read over
  160 bp beside them (two bins are sorted); ext_short_fill at 0 with short sides
  present (the lists' short-run boundaries matter); the certificate off and the
  row bound off (the count kernel feeds the fused scatter).  These cases tie
  the fused histogram to the lists through the regions and the list counters
  (left / right listed, their long parts), which must equal mask 0's; they do
  not read the histogram itself;
* the late class of tests/test_gpu_ungapped_right.py, rebuilt here, through a
  context with a side stream.  A context whose caller stream leaves it no side
  stream cannot be forced through the API: that order is the one of bit 2 off,
  which every case runs;
* heavy reads without a matrix: a read of 4,097 seeds, five reads of 4,096
  seeds whose matrices pass the pool (2^20 words and the buffer's quarter of
  slack on a fresh context: 4 x 266,112 fit, the fifth does not), a matrix read
  and light reads beside them; the same in a child
  process under BWAGPU_EMU_STRICT=0, where the final pass meets a seed without a
  result and hands the read to the redo pass;
* the golden chain sets and 4,096 reads of the C2 fixture at masks 0, 7 and 5.

Run as a script (`python test_gpu_fused_launches.py --child`) it is that child:
it prints one JSON line.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np

if __name__ == "__main__":  # the child process: no pytest, no conftest
    _repo = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    for _p in (os.path.join(_repo, "bwa-flow_amd", "python"), os.path.join(_repo, "oracle"),
               os.path.join(_repo, "tests")):
        sys.path.insert(0, _p)

import golden_io as G  # noqa: E402
import oracle  # noqa: E402
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Batch, Engine, compact  # noqa: E402
from test_gpu_heavy_select import concat, cut_read, seeds_per_read  # noqa: E402

MASKS = (0, 7, 5, 1, 2, 4)
FIELDS = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
RIGHT_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 105, 127, 129)


def run_device(eng, batch):
    """one batch through the device entry, outputs prefilled -> regs, n, the counters as one dict of lists"""
    import torch
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(batch, k)).view(np.uint8).copy()).to(dev) for k in FIELDS}
    out = torch.full((max(batch.n_seeds, 1) * 88,), 0xFF, dtype=torch.uint8, device=dev)
    nn = torch.full((max(batch.n_reads, 1),), -7, dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = batch.n_reads, batch.n_chains, batch.n_seeds
    c.seq_bytes = int(batch.seq_off[-1])
    for k in FIELDS:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), None, stream.cuda_stream)
    torch.cuda.synchronize()
    ctr = {}
    for name, words in (("spec_counters", 8), ("spec_ungapped", 12), ("spec_ungapped_right", 6), ("spec_short", 9)):
        w = np.zeros(words, np.int64)
        assert getattr(eng.lib, "bwagpu_debug_" + name)(eng.ctx, C.c_void_p(stream.cuda_stream),
                                                       w.ctypes.data_as(C.c_void_p)) == 0
        ctr[name] = w.tolist()
    regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:batch.n_seeds]
    return regs, nn.cpu().numpy()[:batch.n_reads], ctr


def run_masks(eng, batch, want, want_n, what, masks=MASKS):
    """the batch at every mask: the oracle's regions, byte for byte, and one set of counters -> those counters"""
    assert eng.fused_launches() == 5, "the mask starts at 5"
    first = None
    for m in masks:
        eng.fused_launches(m)
        assert eng.fused_launches() == m
        regs, n, ctr = run_device(eng, batch)
        assert np.array_equal(n, want_n), f"{what}, mask {m}: {int((n != want_n).sum())} reads with a different region count"
        got = compact(batch, regs, n)
        assert G.region_mismatch(got, want) is None, f"{what}, mask {m}"
        assert got.tobytes() == want.tobytes(), f"{what}, mask {m}: regions not byte-identical to the oracle's"
        if first is None:
            first = ctr
            print(f"{what}, mask {m}: {ctr}")
        assert ctr == first, f"{what}: counters at mask {m} {ctr}, at mask {masks[0]} {first}"
    eng.fused_launches(5)
    return first


# ----------------------------------------------------------------- hand-made batches on the golden genome
def strands(refd):
    l_pac, pac = refd["l_pac"], refd["pac"]
    x = np.arange(l_pac, dtype=np.int64)
    fwd = ((pac[x >> 2].astype(np.int64) >> ((~x & 3) << 1)) & 3).astype(np.uint8)
    return np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])  # the 2-strand coordinate space


def planted(both, x0, n, mm=()):
    fl = both[x0:x0 + n].copy()
    for p in mm:
        fl[p] = (fl[p] + 1) & 3
    return fl


def two_mm(n):
    return (n // 4, n // 2) if n >= 2 else ()


@functools.lru_cache(maxsize=None)
def golden():
    refd = G.load_ref()
    return refd, oracle.Ref(refd["l_pac"], refd["ann_offset"], refd["ann_len"], refd["pac"]), strands(refd)


def hand_batch(spec):
    """spec: (left length, seed length, right length, left mismatches, right mismatches) per read -> a batch of
    one chain of one exact seed per read, on both strands by turns"""
    refd, _, both = golden()
    l_pac = refd["l_pac"]
    seqs, seeds, rids = [], [], []
    for i, (ql, ln, qr, lmm, rmm) in enumerate(spec):
        c = i % len(refd["ann_offset"])
        a0, al = int(refd["ann_offset"][c]), int(refd["ann_len"][c])
        f0 = a0 + 2000 + (7919 * i) % (al - 5000)
        rbeg = 2 * l_pac - (f0 + ln) if i & 1 else f0
        seqs.append(np.concatenate([planted(both, rbeg - ql, ql, lmm), both[rbeg:rbeg + ln],
                                    planted(both, rbeg + ln, qr, rmm)]))
        seeds.append((rbeg, ql, ln, ln, 0))
        rids.append(c)
    n = len(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    return Batch(off, np.concatenate(seqs), np.arange(n + 1), np.arange(n + 1), np.array(rids, np.int32),
                 np.zeros(n, np.float32), np.array(seeds, abi.SEED_DTYPE))


def dp_side(n):
    """mismatches that keep a side of n bases on its list: two of them cost 2 (a + b) = 10 >= o + e = 7"""
    return two_mm(n)


def n_tasks_spec(n):
    """n reads whose sides (various lengths, some certified, most not) all lie in the first length bin"""
    out = []
    for i in range(n):
        ql, qr = 3 + (37 * i) % 60, 2 + (53 * i) % 68
        out.append((ql, 19 + i % 11, qr, dp_side(ql) if (i + 1) % 5 else (), dp_side(qr) if (i + 1) % 7 else (1,)))
    return out


def late_spec():
    """the late-class batch of tests/test_gpu_ungapped_right.py: a left side with two mismatches in front of a
    certified right side, beside a read of every other left / right class"""
    out = []
    for qr in RIGHT_LENGTHS:
        out.append((10, 19, qr, two_mm(10), ()))
        out.append((10, 19, qr, two_mm(10), (qr // 4,)))
        out.append((10, 19, qr, two_mm(10), ()))  # (twice: hand_batch alternates the strands)
        out.append((10, 19, qr, two_mm(10), (qr // 4,)))
    out += [(0, 60, 0, (), ()), (0, 30, 40, (), (10,)), (0, 30, 40, (), (10, 20)), (40, 30, 0, (10,), ()),
            (40, 30, 0, (10, 20), ()), (33, 30, 47, (), (46,)), (20, 30, 20, (5,), (5, 10)),
            (20, 30, 20, (5, 10), (5, 10)), (4, 8, 3, (1, 2), ()), (20, 30, 40, (5, 10), (12, 20)),
            (20, 30, 18, (5, 10), (13,))]
    return out


SORT_CASES = {
    "tasks_1": lambda: n_tasks_spec(1),
    "tasks_255": lambda: n_tasks_spec(255),
    "tasks_256": lambda: n_tasks_spec(256),
    "tasks_257": lambda: n_tasks_spec(257),
    "tasks_2049": lambda: n_tasks_spec(2049),   # more than one task per scatter thread per pass
    "one_key": lambda: [(20, 30, 20, (5, 10), (5, 10))] * 600,  # all cursor traffic on one word per side
    # a 150 bp read beside a 19-base seed: every split of the 131 other bases, so every key such a read can produce
    "every_key": lambda: [(ql, 19, 131 - ql, dp_side(ql), dp_side(131 - ql)) for ql in range(132)] * 2,
    # a read of 200 bp: the second length bin's lists are sorted too
    "two_bins": lambda: n_tasks_spec(300) + [(90, 20, 90, dp_side(90), dp_side(90)), (0, 40, 160, (), dp_side(160))],
}


@functools.lru_cache(maxsize=None)
def hand_case(name):
    batch = hand_batch(late_spec() if name == "late" else SORT_CASES[name]())
    refd, ref, _ = golden()
    opt = G.load_chain_set("c1_default")[0]
    regs, n, _ = oracle.chain2aln("oracle", opt, ref, batch)
    want = compact(batch, regs, n)
    want.setflags(write=False)
    n.setflags(write=False)
    return opt, batch, want, n


def golden_engine(opt):
    refd = golden()[0]
    return Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])


# ----------------------------------------------------------------- heavy reads without a pair matrix
def repeat_read(b, r, times):
    """read r alone with its chains `times` times over"""
    one = b.subset([r])
    nch = one.n_chains
    cso = [np.zeros(1, np.int64)]
    for _ in range(times):
        cso.append(one.chain_seed_off[1:].astype(np.int64) + cso[-1][-1])
    return Batch(one.seq_off, one.seq, np.array([0, nch * times]), np.concatenate(cso), np.tile(one.chain_rid, times),
                 np.tile(one.chain_frac_rep, times), np.tile(one.seeds, times))


@functools.lru_cache(maxsize=None)
def heavy_case():
    """-> opt, the fixture's reference, the batch, the oracle's regions and counts.  Read 0 a matrix read, then
    light reads, a read of 4,097 seeds (no matrix at any pool size), five reads of 4,096 seeds (four matrices
    of 2 x 133,056 words fit a fresh context's pool of 2^20 words and a quarter, the fifth does not) and light
    reads again"""
    opt, ref, rbs = workload.load_fixture()
    b = rbs[0].batch
    ns = seeds_per_read(b)
    big = int(np.argmax(ns))
    assert int(ns[big]) == 1167
    wide = repeat_read(b, big, 4)
    mid = int(np.nonzero((ns > 200) & (ns < 600))[0][0])
    light = [int(r) for r in np.nonzero((ns > 0) & (ns <= 64))[0][:12]]
    parts = [b.subset([mid]), b.subset(light[:6]), cut_read(wide, 0, 4097)]
    parts += [cut_read(wide, 0, 4096) for _ in range(5)] + [b.subset(light[6:])]
    sub = concat(parts)
    got = seeds_per_read(sub).tolist()
    assert got[7] == 4097 and got[8:13] == [4096] * 5 and sub.n_reads == 19
    pool = (1 << 20) + (1 << 18)  # max(2^20, 16 n_seeds) words asked for, and the growing buffer's quarter on top
    assert 16 * sub.n_seeds < 1 << 20 and 4 * 266112 + 968 <= pool < 5 * 266112, "the pool's size and the matrices'"
    R = oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac)
    regs, n, _ = oracle.chain2aln("oracle", opt, R, sub, n_threads=4)
    want = compact(sub, regs, n)
    want.setflags(write=False)
    n.setflags(write=False)
    return opt, ref, sub, want, n


def child():
    """BWAGPU_EMU_STRICT=0: the heavy case at every mask through the device entry -> mismatches, counters"""
    opt, ref, sub, want, want_n = heavy_case()
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    out = {}
    for m in MASKS:
        eng.fused_launches(m)
        regs, n, ctr = run_device(eng, sub)
        bad = None if np.array_equal(n, want_n) else "region counts"
        bad = bad or G.region_mismatch(compact(sub, regs, n), want)
        out[str(m)] = [bad, ctr["spec_counters"]]
    eng.close()
    return out


if __name__ == "__main__":
    print(json.dumps(child()))
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def test_no_chains():
    """a first-bin list of 0 tasks: reads without a chain, no extension round at all"""
    refd, ref, both = golden()
    opt = G.load_chain_set("c1_default")[0]
    seqs = [both[5000 + 200 * i:5000 + 200 * i + 100] for i in range(5)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    batch = Batch(off, np.concatenate(seqs), np.zeros(6, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32),
                  np.zeros(0, np.float32), np.zeros(0, abi.SEED_DTYPE))
    regs, n, _ = oracle.chain2aln("oracle", opt, ref, batch)
    assert not n.any()
    eng = golden_engine(opt)
    run_masks(eng, batch, compact(batch, regs, n), n, "no chains")
    eng.close()


@pytest.mark.parametrize("name", sorted(SORT_CASES))
def test_sort_stage(name):
    opt, batch, want, want_n = hand_case(name)
    eng = golden_engine(opt)
    ctr = run_masks(eng, batch, want, want_n, name)
    eng.close()
    assert ctr["spec_counters"][0] == batch.n_reads, "round A: a task per read"
    ung = np.array(ctr["spec_ungapped"]).reshape(3, 4)
    assert ung[0, 2] > 0 and ung[0, 3] > 0, "no side left on a list: the sort is not exercised"
    if name == "two_bins":
        assert int(np.diff(batch.seq_off).max()) > 160


@pytest.mark.parametrize("knob", ["short_fill_0", "ungapped_off", "row_bound_off"])
def test_sort_stage_knobs(knob):
    """short_fill_0: every short side takes the short phase, so the scatter's SPC_LLONG / SPC_RLONG words
    decide where each launch's second run begins; the other two: no certificate kernel, the count kernel
    feeds the fused scatter"""
    # (short_fill_0 on the sides of every length up to 131: both lists have sides on either side of the threshold)
    opt, batch, want, want_n = hand_case("every_key" if knob == "short_fill_0" else "tasks_2049")
    eng = golden_engine(opt)
    if knob == "short_fill_0":
        eng.ext_short_fill(0)
    elif knob == "ungapped_off":
        eng.ungapped(0)
    else:
        eng.row_bound(0)
    ctr = run_masks(eng, batch, want, want_n, knob)
    eng.close()
    short = ctr["spec_short"]
    if knob == "short_fill_0":
        assert short[0] > 0, "no side ran in the short phase"
        assert 0 < short[2] < short[1] and 0 < short[4] < short[3], f"round A's short runs: {short}"
    else:
        assert not np.array(ctr["spec_ungapped"]).reshape(3, 4)[:, 0].any(), "the certificate settled a side"


def test_late_sides_with_a_side_stream():
    opt, batch, want, want_n = hand_case("late")
    eng = golden_engine(opt)
    assert eng.ungapped_right() == 1
    ctr = run_masks(eng, batch, want, want_n, "late class")
    eng.close()
    late = np.array(ctr["spec_ungapped_right"]).reshape(3, 2)
    # the forty late_* reads at the least (cost 10 on the left, at most 5 on the right, against o + e = 7)
    assert late[0, 0] >= 4 * len(RIGHT_LENGTHS) and late[0, 1] >= 2 * 2 * sum(RIGHT_LENGTHS), late.tolist()


def test_heavy_reads_without_a_matrix():
    opt, ref, sub, want, want_n = heavy_case()
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    ctr = run_masks(eng, sub, want, want_n, "heavy reads")
    eng.close()
    sc = ctr["spec_counters"]
    ns = seeds_per_read(sub)
    assert sc[5] == 7, f"{sc[5]} heavy reads"
    assert sc[7] == int(ns[0]) + 4 * 4096, f"{sc[7]} matrix columns: the first read's and four reads' of 4,096 seeds"


def test_heavy_reads_with_strict_emulation_off():
    env = dict(os.environ, BWAGPU_EMU_STRICT="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print(r)
    assert all(r[str(m)][0] is None for m in MASKS), r
    assert all(r[str(m)][1] == r["0"][1] for m in MASKS), f"counters differ between masks: {r}"
    assert r["0"][1][6] > 0, "no read went to the redo pass: the fold's final pass met no miss"


@pytest.mark.parametrize("name", G.CHAIN_SETS)
def test_chain_sets(name):
    refd = golden()[0]
    opt, batch, want, want_n = G.load_chain_set(name)
    eng = golden_engine(opt)
    run_masks(eng, batch, want, want_n, name, masks=(0, 7, 5))
    eng.close()


def test_c2_fixture_4096_reads():
    opt, ref, rbs = workload.load_fixture()
    sub = rbs[0].batch.subset(range(4096))
    R = oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac)
    regs, n, _ = oracle.chain2aln("oracle", opt, R, sub, n_threads=4)
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    run_masks(eng, sub, compact(sub, regs, n), n, "C2, 4,096 reads", masks=(0, 7, 5))
    eng.close()
