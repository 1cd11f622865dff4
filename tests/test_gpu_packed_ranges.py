"""GPU: the packed 16-bit extension (extend_quad) and the 32-bit wave kernels
at the edges of the host-side range gates that admit work to them (pure.h
quad_bound_ok / quad_rows_ok / quad_key8_ok / wave_bound_ok, applied by
task_host.h extend_plan and spec_plan.h ext_plan).

Expected values come from the CPU oracle and, for the bare tasks, from
tests/golden/ksw_range.npz (the reference's own ksw_extend2); nothing expected
comes from the code under test, and every comparison is exact.

* bare tasks: every family of tests/range_cases.py, the last admitted value
  ("in": the packed kernel, as tests/cpp/task_host_asan.cpp pins) and the first
  refused one ("out": the wave kernels), with the packed path on and off and
  the row bound on and off;
* the 32-bit ceiling: hb = 2^21 - 1 is exact, 2^21 is refused with
  E_UNSUPPORTED and the engine serves the next batch;
* mem_chain2aln at the plan's gates: option sets on both sides of
  quad_scores_ok(o, 256) and quad_rows_ok(o, tb_bytes), on the spec, quad and
  pair paths, with the kernel in use asserted first and with reads whose
  extension climbs to lq * a in each length bin's kernel.
"""
import numpy as np
import pytest

import golden_io as G
import oracle
import range_cases as R
from bwagpu import abi
from bwagpu.engine import Batch, BwaGpuError, Engine, compact
from conftest import set_c2a_path

pytestmark = pytest.mark.gpu

FLAT = R.flat()
BARE = [(n, s, f) for n, s, f in FLAT if (n, s) != ("wave32", "out")]  # that one is refused: its own test


@pytest.fixture(scope="module")
def refd():
    return G.load_ref()


@pytest.fixture(scope="module")
def gold():
    return G.load_range()


@pytest.fixture(params=["quad", "wave"])
def ext_path(request):
    """bare ksw_extend2 lists: the packed kernel where a task passes the gates
    (default), or the wave kernels only (bwagpu_debug_ext_form(1))"""
    lib = abi.load()
    prev = lib.bwagpu_debug_ext_form(0 if request.param == "quad" else 1)
    yield request.param
    lib.bwagpu_debug_ext_form(prev)


def make_engine(refd, opt):
    return Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])


def six(r):
    return r.view(np.int32).reshape(-1, 6)


def assert_six(tasks, got, want, what):
    bad = np.nonzero((six(got) != six(want)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)}/{len(tasks)} tasks differ; first #{bad[0]} {tasks[bad[0]]}: " \
                          f"got {got[bad[0]]} want {want[bad[0]]}"


@pytest.mark.parametrize("name,side,f", BARE, ids=[f"{n}-{s}" for n, s, _ in BARE])
def test_bare_tasks_at_the_gates(refd, gold, name, side, f, ext_path):
    want, cells = oracle.extend("oracle", f.opt, f.tasks, f.qpool, f.tpool)
    gopt, gtasks, gwant, _, _ = gold[(name, side)]
    assert np.array_equal(gtasks, f.tasks)
    eng = make_engine(refd, f.opt)
    for bound in (1, 0):
        eng.row_bound(bound)
        got = eng.extend_batch(f.tasks, f.qpool, f.tpool)
        what = f"{name}-{side} ({f.gate}), {ext_path}, row bound {bound}"
        assert_six(f.tasks, got, want, what + ", vs the oracle")
        assert_six(f.tasks, got, gwant, what + ", vs the reference's recorded results")
        st = eng.last_stats()
        if bound:  # calls end early, never late
            assert st["cells"] <= cells[0] and st["rows"] <= cells[1], what
        else:
            assert st["cells"] == cells[0] and st["rows"] == cells[1], what
    eng.close()


def test_wave_ceiling_refused_and_engine_lives(refd, ext_path):
    """hb = 2^21 overflows the wave kernels' int key H << 10 | j: extend_plan
    refuses the batch (wave_bound_ok, pure.h); the next batch is served"""
    fams = R.families()
    out, ok = fams["wave32"]["out"], fams["ceiling_a1"]["in"]
    eng = make_engine(refd, out.opt)
    with pytest.raises(BwaGpuError) as e:
        eng.extend_batch(out.tasks, out.qpool, out.tpool)
    assert e.value.code == abi.E_UNSUPPORTED and "2^21" in str(e.value)
    mixed = ok.tasks.copy()  # one such task among good ones refuses the batch too
    mixed["h0"][7] = (1 << 21) - int(mixed["qlen"][7])
    with pytest.raises(BwaGpuError) as e:
        eng.extend_batch(mixed, ok.qpool, ok.tpool)
    assert e.value.code == abi.E_UNSUPPORTED
    want, _ = oracle.extend("oracle", ok.opt, ok.tasks, ok.qpool, ok.tpool)
    assert_six(ok.tasks, eng.extend_batch(ok.tasks, ok.qpool, ok.tpool), want, "the batch after a refusal")
    eng.close()


# ------------------------------------------------------------------ mem_chain2aln at the plan's gates
def _opt(a=1, b=4, e=1):
    return dict(a=a, b=b, o_del=6, e_del=e, o_ins=6, e_ins=e, pen_clip5=5, pen_clip3=5, w=100, zdrop=100,
                mat=abi.fill_scmat(a, b))


SIDE_OCT, SIDE_QUAD, SIDE_WIDE, EXT2 = ("spec_side4_kernel<16, 10, true>", "spec_side4_kernel<32, 5, true>",
                                        "spec_side4_kernel<32, 8, false>", "spec_ext2_kernel<5>")
# name -> options, and the first bin's kernel on the spec and quad paths (spec_plan.h's table; the
# pair path always runs spec_ext2_kernel<5>).  The batches' longest read has 257 bases:
#   a7      quad_scores_ok: 256 * 7 = 1792, (1792 << 3) + 128 < 32768; not key8 (160 * 7 > 255)
#   a8      (2048 << 4) + 128 = 32896: refused
#   e54     tb_bytes_for = 272 (band cap 5): (272 + 256) * 54 = 28512 < 28672; key8
#   e55     528 * 55 = 29040: refused by quad_rows_ok
#   a7_e54  the band cap grows with the scores: 304 row bytes, 560 * 54 = 30240: refused by
#           quad_rows_ok though a7 and e54 each pass (tests/cpp/ext_plan_asan.cpp has all five)
PLAN_SETS = {
    "a7": (_opt(a=7), SIDE_WIDE, SIDE_WIDE),
    "a8": (_opt(a=8), EXT2, EXT2),
    "e54": (_opt(e=54), SIDE_OCT, SIDE_QUAD),
    "e55": (_opt(e=55), EXT2, EXT2),
    "a7_e54": (_opt(a=7, e=54), EXT2, EXT2),
}
PLAN_CASES = [(0, "a7"), (0, "a8"), (250, "a7"), (250, "a8"), (250, "e54"), (250, "e55"), (0, "a7_e54"),
              (250, "a7_e54")]
CLIMB_LENS = (160, 161, 256, 257)  # both sides of the first two length bins' limits (kSpecBinLen)


def _base(pac, x):
    return (int(pac[x >> 2]) >> ((~x & 3) << 1)) & 3


def climbing_reads(sref):
    """16 error-free forward-strand reads cut from the genome, four of each length in
    CLIMB_LENS, one chain of one seed each: the whole read, or 19 bases at its start, its end
    or its middle -- the extensions from the short seeds match to the read's end, so H climbs
    to lq * a in the kernel of the read's length bin"""
    seq, seq_off, seeds, rid = [], [0], [], []
    k = 0
    for lq in CLIMB_LENS:
        for qb, ln in ((0, lq), (0, 19), (lq - 19, 19), (lq // 2, 19)):
            c = k % len(sref.ann_offset)
            pos = int(sref.ann_offset[c]) + 5000 + 1000 * k
            assert pos + lq + 2000 < int(sref.ann_offset[c]) + int(sref.ann_len[c])
            seq.append(np.array([_base(sref.pac, pos + i) for i in range(lq)], np.uint8))
            seq_off.append(seq_off[-1] + lq)
            seeds.append((pos + qb, qb, ln, ln, 0))
            rid.append(c)
            k += 1
    n = len(rid)
    return Batch(np.array(seq_off), np.concatenate(seq), np.arange(n + 1), np.arange(n + 1), np.array(rid, np.int32),
                 np.zeros(n, np.float32), np.array(seeds, abi.SEED_DTYPE))


def concat(batches):
    seq_off, rco, cso = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)]
    for x in batches:
        seq_off.append(np.asarray(x.seq_off[1:], np.int64) + seq_off[-1][-1])
        rco.append(np.asarray(x.read_chain_off[1:], np.int64) + rco[-1][-1])
        cso.append(np.asarray(x.chain_seed_off[1:], np.int64) + cso[-1][-1])
    return Batch(np.concatenate(seq_off), np.concatenate([x.seq for x in batches]), np.concatenate(rco),
                 np.concatenate(cso), np.concatenate([x.chain_rid for x in batches]).astype(np.int32),
                 np.concatenate([x.chain_frac_rep for x in batches]).astype(np.float32),
                 np.concatenate([x.seeds for x in batches]))


_plan_cache: dict = {}


def plan_case(len_mode, name):
    """-> synthetic genome, batch, oracle regions / counts / stats: computed once a case"""
    from bwagpu.synth import SynthRef, synth_batch
    if "ref" not in _plan_cache:
        _plan_cache["ref"] = SynthRef(77, 2_000_000, 3)
    sref = _plan_cache["ref"]
    if ("batch", len_mode) not in _plan_cache:
        b = concat([synth_batch(sref, 31 + len_mode, 150, len_mode, 19), climbing_reads(sref)])
        _plan_cache[("batch", len_mode)] = b
    b = _plan_cache[("batch", len_mode)]
    if (len_mode, name) not in _plan_cache:
        R_ = oracle.Ref(sref.l_pac, sref.ann_offset, sref.ann_len, sref.pac)
        _plan_cache[(len_mode, name)] = oracle.chain2aln("oracle", PLAN_SETS[name][0], R_, b, n_threads=4)
    return sref, b, _plan_cache[(len_mode, name)]


@pytest.mark.parametrize("path", ["spec", "quad", "pair"])
@pytest.mark.parametrize("len_mode,name", PLAN_CASES)
def test_chain2aln_at_the_plan_gates(len_mode, name, path, monkeypatch):
    sref, b, (oregs, on, ost) = plan_case(len_mode, name)
    opt, k_spec, k_quad = PLAN_SETS[name]
    lq_max = int(np.diff(b.seq_off).max())
    assert lq_max == 257
    # the climbing reads (the batch's last 16): the oracle's best region of each spans the
    # read with score lq * a, so some extension's H reached it
    want = compact(b, oregs, on)
    nr = b.n_reads
    first = np.concatenate([[0], np.cumsum(on)])
    for r in range(nr - 16, nr):
        lq = int(b.seq_off[r + 1] - b.seq_off[r])
        regs = want[first[r]:first[r + 1]]
        assert len(regs) and int(regs["score"].max()) == lq * opt["a"] and lq in CLIMB_LENS
    restore = set_c2a_path(path, monkeypatch)
    try:
        eng = Engine(0, opt, sref.l_pac, sref.ann_offset, sref.ann_len, pac=sref.pac)
        assert eng.ext_kernel(lq_max) == {"spec": k_spec, "quad": k_quad, "pair": EXT2}[path]
        for bound in (1, 0):
            eng.row_bound(bound)
            regs, n = eng.chain2aln(b)
            what = f"{name}, reads of mode {len_mode}, path {path}, row bound {bound}"
            assert np.array_equal(n, on), f"{what}: {int((n != on).sum())} reads with a different region count"
            assert G.region_mismatch(compact(b, regs, n), want) is None, what
            st = eng.last_stats()
            got_c, want_c = (st["cells"], st["rows"], st["ext_calls"]), tuple(int(x) for x in ost[:3])
            if bound:
                assert got_c[2] == want_c[2] and got_c[0] <= want_c[0] and got_c[1] <= want_c[1], (what, got_c, want_c)
            else:
                assert got_c == want_c, what
        eng.close()
    finally:
        restore()
