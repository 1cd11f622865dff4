#!/usr/bin/env python3
"""The region post-processing pass on one resident c2_refseed batch
(tests/golden/c2_refseed.npz, 66,668 reads): bwagpu_regs_post_device per batch
by HIP events, beside the reference's mem_sort_dedup_patch over the same regions
on 1 and 16 host threads (oracle/_ref/libbwaref.so through ctypes: the per-read
call overhead of ctypes is inside those figures), and the D2H bytes of a
submit/wait with and without the switch.  Flags 1|2 (BWAGPU_POST_PRIMARY is not
built).  -> profiles/post_bench.json

    python tools_dev/post_bench.py [--reps 30] [--out profiles/post_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"),
          HERE):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine, compact  # noqa: E402


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=float(np.median(v)), min=float(v[0]), p10=float(v[len(v) // 10]),
                p90=float(v[(len(v) * 9) // 10]), max=float(v[-1]), n=len(v))


def cpu_reference(opt, ref, b, regs, n, alt, threads):
    """wall seconds of mem_sort_dedup_patch + the is_alt loop over every read"""
    from gen_post_fixture import RefPost
    refd = dict(l_pac=ref.l_pac, ann_offset=ref.ann_offset, ann_len=ref.ann_len, pac=ref.pac)
    rp = RefPost(opt, (10000, 0.95, 0.50), refd, alt)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    work = regs.copy()
    seq = b.seq.copy()
    base, qbase = work.ctypes.data, seq.ctypes.data
    so = b.seq_off
    todo = [r for r in range(b.n_reads) if n[r] > 1]

    def run(lo, hi):
        f, o, bns, pac = rp.lib.mem_sort_dedup_patch, C.byref(rp.o), C.byref(rp.bns), rp.pac.ctypes.data
        for r in todo[lo:hi]:
            f(o, bns, pac, qbase + int(so[r]), int(n[r]), base + 88 * int(off[r]))

    step = (len(todo) + threads - 1) // threads
    th = [threading.Thread(target=run, args=(k * step, (k + 1) * step)) for k in range(threads)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "post_bench.json"))
    a = ap.parse_args()
    opt, ref, bs = workload.load_fixture()
    b = bs[0].batch
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    alt = np.zeros(len(ref.ann_len), np.uint8)
    alt[len(alt) - 1] = 1
    eng.set_alt(alt)
    flags = abi.POST_DEDUP_PATCH | abi.POST_MARK_ALT
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(getattr(b, k)).view(np.uint8).copy()).to(dev)
         for k in ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")}
    bc = abi.BatchC()
    bc.n_reads, bc.n_chains, bc.n_seeds = b.n_reads, b.n_chains, b.n_seeds
    bc.seq_bytes = int(b.seq_off[-1])
    for k in t:
        setattr(bc, k, t[k].data_ptr())
    raw = torch.zeros(b.n_seeds * 88, dtype=torch.uint8, device=dev)
    raw_n = torch.zeros(b.n_reads, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    eng.chain2aln_device(bc, raw.data_ptr(), raw_n.data_ptr(), None, s.cuda_stream)
    s.synchronize()
    work, work_n = raw.clone(), raw_n.clone()
    ms = []
    with torch.cuda.stream(s):
        for k in range(a.warmup + a.reps):
            work.copy_(raw)
            work_n.copy_(raw_n)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            eng.regs_post_device(bc, None, work.data_ptr(), work_n.data_ptr(), flags, 0, None, s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
    n_in, n_out = raw_n.cpu().numpy(), work_n.cpu().numpy()
    regs_in = raw.cpu().numpy().view(abi.ALNREG_DTYPE)
    # D2H with and without the switch (bwagpu_last_stats of a submit / wait)
    d2h = {}
    for name, f in (("switch_off", 0), ("switch_on", flags)):
        eng.set_regs_post(f)
        eng.submit(0, b)
        eng.wait_dense(0, b)
        d2h[name] = int(eng.last_stats(0)["d2h_bytes"])
    eng.set_regs_post(0)
    res = dict(workload="tests/golden/c2_refseed.npz batch 0, resident", reads=int(b.n_reads), flags=int(flags),
               regions_in=int(n_in.sum()), regions_out=int(n_out.sum()), reads_with_2_or_more=int((n_in > 1).sum()),
               regs_post_device_ms=spread(ms), d2h_bytes=d2h)
    try:
        dense = compact(b, regs_in, n_in)
        res["reference_cpu_s"] = {f"threads_{k}": cpu_reference(opt, ref, b, dense, n_in, alt, k) for k in (1, 16)}
        res["reference_cpu_note"] = "mem_sort_dedup_patch per read through ctypes (call overhead included), reads with n > 1"
    except Exception as e:  # no reference library beside the tree
        res["reference_cpu_s"] = {"error": repr(e)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
