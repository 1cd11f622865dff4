"""The heavy reads' selection passes (spec_pairs_kernel / spec_scan_kernel:
reads of more than 64 seeds or chains, with pair matrices) against the oracle.

The input is every heavy read of the C2 fixture's two batches with light reads
in between: one batch small enough for the CPU oracle to give the expected
regions in well under a second.  Its reads cover a matrix staged in LDS and
one read from global memory (the reads of 694 seeds and more), 64-seed blocks
whose in-block decisions resolve in one round and one of full serial depth.
Copies of the largest read cut at the 64-seed word boundaries run the same
way.  With BWAGPU_EMU_STRICT=0 (a child process: the library reads it once)
the final pass meets extended seeds without a result, so the serial in-block
loop and the inline extension run too.

Run as a script (`python test_gpu_heavy_select.py --child`) it is that child:
it prints one JSON line.
"""
import ctypes
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

N_LIGHT = 100                              # light reads per fixture batch, one after each of the first heavy reads
CUTS = (65, 127, 128, 129, 192, 193)       # seeds: around the first, second and third word boundary


def seeds_per_read(b: Batch) -> np.ndarray:
    off = b.chain_seed_off[b.read_chain_off]
    return (off[1:] - off[:-1]).astype(np.int64)


def heavy_reads(b: Batch) -> np.ndarray:
    nch = np.diff(b.read_chain_off.astype(np.int64))
    return np.nonzero((seeds_per_read(b) > 64) | (nch > 64))[0]


def concat(parts) -> Batch:
    seq_off, rco, cso = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)]
    for p in parts:
        seq_off.append(p.seq_off[1:].astype(np.int64) + seq_off[-1][-1])
        rco.append(p.read_chain_off[1:].astype(np.int64) + rco[-1][-1])
        cso.append(p.chain_seed_off[1:].astype(np.int64) + cso[-1][-1])
    return Batch(np.concatenate(seq_off), np.concatenate([p.seq for p in parts]), np.concatenate(rco),
                 np.concatenate(cso), np.concatenate([p.chain_rid for p in parts]),
                 np.concatenate([p.chain_frac_rep for p in parts]), np.concatenate([p.seeds for p in parts]))


def cut_read(b: Batch, r: int, n_seeds: int) -> Batch:
    """read r alone, cut to its first n_seeds seeds: the trailing chains are
    dropped and the last kept chain loses its trailing seeds; the offsets are
    rebuilt by hand"""
    c0, c1 = int(b.read_chain_off[r]), int(b.read_chain_off[r + 1])
    cso, rid, fr = [0], [], []
    for c in range(c0, c1):
        if cso[-1] == n_seeds:
            break
        n = min(int(b.chain_seed_off[c + 1] - b.chain_seed_off[c]), n_seeds - cso[-1])
        cso.append(cso[-1] + n)
        rid.append(b.chain_rid[c])
        fr.append(b.chain_frac_rep[c])
    assert cso[-1] == n_seeds
    seeds = []
    for i, c in enumerate(range(c0, c0 + len(rid))):
        a = int(b.chain_seed_off[c])
        seeds.append(b.seeds[a:a + cso[i + 1] - cso[i]])
    lq = int(b.seq_off[r + 1] - b.seq_off[r])
    return Batch(np.array([0, lq]), b.seq[b.seq_off[r]:b.seq_off[r + 1]], np.array([0, len(rid)]), np.array(cso),
                 np.array(rid, np.int32), np.array(fr, np.float32), np.concatenate(seeds))


@functools.lru_cache(maxsize=None)
def case(name: str):
    """-> (opt, GoldenRef, input batch, expected regions (compact), expected counts, heavy reads in it)"""
    opt, ref, rbs = workload.load_fixture()
    R = oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac)
    if name == "subset":
        parts, n_heavy = [], 0
        for rb in rbs:
            b = rb.batch
            hv = heavy_reads(b)
            heavy = set(hv.tolist())
            light = [r for r in range(0, b.n_reads, max(b.n_reads // (2 * N_LIGHT), 1)) if r not in heavy][:N_LIGHT]
            order = []
            for i, r in enumerate(hv.tolist()):
                order.append(r)
                if i < len(light):
                    order.append(light[i])
            parts.append(b.subset(order))
            n_heavy += len(hv)
        sub = concat(parts)
    else:
        b = rbs[0].batch
        big = int(np.argmax(seeds_per_read(b)))
        sub = concat([cut_read(b, big, n) for n in CUTS])
        n_heavy = len(CUTS)
    want, want_n, _ = oracle.chain2aln("oracle", opt, R, sub, n_threads=4)
    want = compact(sub, want, want_n)
    want.setflags(write=False)
    want_n.setflags(write=False)
    return opt, ref, sub, want, want_n, n_heavy


def mismatch(sub, regs, n, want, want_n):
    if not np.array_equal(n, want_n):
        return f"{int((n != want_n).sum())} reads with a different region count"
    return G.region_mismatch(compact(sub, regs, n), want)


def run_host(name: str):
    opt, ref, sub, want, want_n, _ = case(name)
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    try:
        return mismatch(sub, *eng.chain2aln(sub), want, want_n)
    finally:
        eng.close()


if __name__ == "__main__":
    print(json.dumps({k: run_host(k) for k in ("subset", "cuts")}))
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


def test_subset_is_the_issue_s_input():
    _, _, sub, _, _, n_heavy = case("subset")
    ns = seeds_per_read(sub)
    assert n_heavy == 348 and sub.n_reads == n_heavy + 2 * N_LIGHT
    assert int((ns > 64).sum()) >= 340 and int(ns.max()) == 1167
    # matrices beyond the 64 KiB of LDS staging (2 * tri_off(ns) words) and within it
    assert {694, 716, 850, 1014, 1167} <= set(ns.tolist()) and int((ns == 545).sum()) >= 1
    assert 55_000 <= sub.n_seeds <= 70_000


def test_subset_parity():
    assert run_host("subset") is None


def test_word_boundary_cuts():
    _, _, sub, _, _, _ = case("cuts")
    assert tuple(seeds_per_read(sub).tolist()) == CUTS
    assert run_host("cuts") is None


def test_strict_emulation_off():
    """BWAGPU_EMU_STRICT=0: no round-B task for an uncertain skip, so the final
    pass finds extended seeds without a result: the serial in-block loop with
    the inline extension"""
    env = dict(os.environ, BWAGPU_EMU_STRICT="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r == {"subset": None, "cuts": None}, r


def test_repeat_run_and_no_inline_extension():
    """two launches on one context through the device entry: the second reuses
    the scratch (matrices, seedcov marks); on the default path no extension is
    left for the final pass to compute inline (counter 4)"""
    torch = pytest.importorskip("torch")
    opt, ref, sub, want, want_n, n_heavy = case("subset")
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    dev = torch.device("cuda:0")
    fields = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(sub, k)).view(np.uint8).copy()).to(dev) for k in fields}
    out = torch.zeros(sub.n_seeds * 88, dtype=torch.uint8, device=dev)
    nn = torch.zeros(sub.n_reads, dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = sub.n_reads, sub.n_chains, sub.n_seeds
    c.seq_bytes = int(sub.seq_off[-1])
    for k in fields:
        setattr(c, k, t[k].data_ptr())
    stream = torch.cuda.current_stream()
    sc = np.zeros(8, np.int64)
    for i in range(2):
        out.zero_()
        nn.zero_()
        eng.chain2aln_device(c, out.data_ptr(), nn.data_ptr(), None, stream.cuda_stream)
        torch.cuda.synchronize()
        regs = out.cpu().numpy().view(abi.ALNREG_DTYPE)[:sub.n_seeds]
        assert mismatch(sub, regs, nn.cpu().numpy()[:sub.n_reads], want, want_n) is None, f"launch {i}"
        assert eng.lib.bwagpu_debug_spec_counters(eng.ctx, ctypes.c_void_p(stream.cuda_stream),
                                                  sc.ctypes.data_as(ctypes.c_void_p)) == 0
        assert sc[4] == 0, f"launch {i}: {int(sc[4])} inline extensions"
        assert sc[5] == n_heavy
    eng.close()
