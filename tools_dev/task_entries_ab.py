#!/usr/bin/env python3
"""Wall time and kernel_ms of the four blocking task entries in one process, on
the workloads of their own benches: bwagpu_extend_batch (ext_bench.py:
c1_default's tasks x 20), bwagpu_align2_batch (align2_bench.py: 32,768 mate
rescue tasks), bwagpu_reg2aln_batch (reg2aln_bench.py: the regions of 33,334
synthetic 2x150 pairs), bwagpu_sw_stream (stream_bench.py: the C2 fixture's
first batch).  No parity check: the GPU tests do that.  The library is
BWAGPU_LIB's, so two trees are compared by running this once per process and
side.  One JSON line: per entry the median of --reps timed calls after --warm.

    BWAGPU_LIB=.../libbwagpu.so python tools_dev/task_entries_ab.py [--reps K] [--warm W] [--only NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("bwa-flow_amd/python", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import golden_io as G  # noqa: E402
import oracle  # noqa: E402
from bwagpu import abi, synth, workload  # noqa: E402
from bwagpu.engine import Engine, unflatten  # noqa: E402


def timed(eng, call, reps, warm):
    for _ in range(warm):
        call()
    walls, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
        kms.append(eng.last_stats()["kernel_ms"])
    return dict(wall_ms=round(1e3 * float(np.median(walls)), 4), kernel_ms=round(float(np.median(kms)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    want = a.only.split(",") if a.only else ["extend", "align2", "reg2aln", "stream"]
    out = {"lib": os.environ.get("BWAGPU_LIB", "(tree)"), "reps": a.reps, "warm": a.warm}
    refd = G.load_ref()
    if "extend" in want:
        opt, tasks, _, qp, tp = G.load_tasks("c1_default")
        big = np.tile(tasks, 20)
        eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
        out["extend"] = dict(n=len(big), **timed(eng, lambda: eng.extend_batch(big, qp, tp), a.reps, a.warm))
        eng.close()
    if "align2" in want:
        t, qp, tp = synth.mate_rescue_tasks(np.random.default_rng(1234), 32768, qlens=(100, 150, 250), win=(300, 700),
                                            xtra_mode="matesw")
        eng = Engine(0, abi.default_opt(), refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
        out["align2"] = dict(n=len(t), **timed(eng, lambda: eng.align2_batch(t, qp, tp), a.reps, a.warm))
        eng.close()
    if "reg2aln" in want:
        ref = synth.SynthRef(42, 46_709_983, 1)
        b = synth.synth_batch(ref, 1000, 33334, 150)
        eng = Engine(0, abi.default_opt(), ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
        regs, n = eng.chain2aln(b)
        jobs = [(g["rb"], g["re"], b.seq_off[r], b.seq_off[r + 1] - b.seq_off[r], g["qb"], g["qe"], g["truesc"],
                 g["w"], 0) for r, p in enumerate(unflatten(b, regs, n)) for g in p]
        t = np.array(jobs, dtype=abi.REG2ALN_TASK_DTYPE)
        out["reg2aln"] = dict(n=len(t), **timed(eng, lambda: eng.reg2aln_batch(t, b.seq, 64, 512), a.reps, a.warm))
        eng.close()
    if "stream" in want:
        opt, ref, bs = workload.load_fixture()
        r = oracle.Ref(ref.l_pac, ref.ann_offset, ref.ann_len, ref.pac)
        words, nt, _, _ = oracle.fpga_pack(opt, r, bs[0].batch)
        eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
        out["stream"] = dict(n=int(nt), **timed(eng, lambda: eng.sw_stream(words, nt), a.reps, a.warm))
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
