#!/usr/bin/env python3
"""Host wall time of the two entries whose host-side passes live in
batch_host.h and seed_host.h, in one process: a blocking bwagpu_chain2aln on
the C2 fixture's first batch (the staging copy and check on eight threads), and
bwagpu_seqs2regions on the golden reads of c5_mixed — as they are (one thread)
and tiled to just over 2^22 bases (the eight-thread validation and staging
pass).  No parity check: the GPU tests do that.  The library is BWAGPU_LIB's,
so two trees are compared by running this once per process and side.  One JSON
line: per entry the median of --reps timed calls after --warm.

    BWAGPU_LIB=.../libbwagpu.so python tools_dev/batch_entries_ab.py [--reps K] [--warm W]
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
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine  # noqa: E402


def timed(call, reps, warm):
    for _ in range(warm):
        call()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(walls)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    a = ap.parse_args()
    out = {"lib": os.environ.get("BWAGPU_LIB", "(tree)"), "reps": a.reps, "warm": a.warm}

    opt, ref, bs = workload.load_fixture()
    b = bs[0].batch
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    out["chain2aln"] = dict(n_reads=int(b.n_reads), n_seeds=int(b.n_seeds),
                            wall_ms=timed(lambda: eng.chain2aln(b), a.reps, a.warm))
    eng.close()

    refd = G.load_ref()
    opt, batch, _, _ = G.load_chain_set("c5_mixed")
    eng = Engine(0, opt, refd["l_pac"], refd["ann_offset"], refd["ann_len"], pac=refd["pac"])
    hdr, words = G.load_seed_bwt()
    sa_intv, sa, _, _ = G.load_seed_sa()
    eng.set_bwt(hdr, words, sa, sa_intv)
    copt = abi.default_chainopt()
    so, seq = np.asarray(batch.seq_off, np.int64), np.asarray(batch.seq, np.uint8)
    out["seqs2regions"] = dict(n_reads=len(so) - 1, bases=int(so[-1]), wall_ms=timed(
        lambda: eng.seqs2regions(so, seq, (19, 10, 20), 1.5, copt, copy=False), a.reps, a.warm))
    k = (1 << 22) // int(so[-1]) + 1
    lens = np.tile(np.diff(so), k)
    so_k, seq_k = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.tile(seq[:so[-1]], k)
    out["seqs2regions_tiled"] = dict(n_reads=len(so_k) - 1, bases=int(so_k[-1]), wall_ms=timed(
        lambda: eng.seqs2regions(so_k, seq_k, (19, 10, 20), 1.5, copt, copy=False), a.reps, a.warm))
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
