#!/usr/bin/env python3
"""mem_pestat and the mate rescue loop on one resident c2_refseed batch
(tests/golden/c2_refseed.npz batch 0: 33,334 interleaved 2x150 bp pairs),
post-processed on the device (bwagpu_regs_post_device, flags 1|2):
bwagpu_pestat_device and bwagpu_mate_rescue_device per batch by HIP events, the
rescue split into plan / ksw_align2 / replay (bwagpu_debug_rescue_times), the
tasks speculated against the tasks used, and the rounds; beside the reference's
mem_pestat plus the loop of bwamem_pair.c:271-277 over the same pairs on one
host thread (oracle/_ref/libbwaref.so through ctypes: only the time inside
mem_pestat and mem_matesw is counted).  -> profiles/rescue_bench.json

    python tools_dev/rescue_bench.py [--reps 30] [--out profiles/rescue_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"),
          HERE):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine  # noqa: E402

HEADROOM = 8


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return dict(median=float(np.median(v)), min=float(v[0]), p10=float(v[len(v) // 10]),
                p90=float(v[(len(v) * 9) // 10]), max=float(v[-1]), n=len(v))


def cpu_reference(opt, ref, b, regs_by_read, alt):
    """seconds inside the reference's mem_pestat and mem_matesw over every pair, one thread"""
    from gen_rescue_fixture import RefPair, libc
    po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
              mask_level_redun=0.95, mask_level=0.50)
    refd = dict(l_pac=ref.l_pac, ann_offset=ref.ann_offset, ann_len=ref.ann_len, pac=ref.pac)
    rp = RefPair(opt, po, refd, alt)
    t0 = time.perf_counter()
    pes = rp.pestat(regs_by_read)
    t_pestat = time.perf_counter() - t0
    so, seq = b.seq_off, b.seq
    t_sw, calls, n_sw = 0.0, 0, 0
    for p in range(len(regs_by_read) // 2):
        a = [regs_by_read[2 * p], regs_by_read[2 * p + 1]]
        ms = [seq[so[2 * p + 1]:so[2 * p + 2]], seq[so[2 * p]:so[2 * p + 1]]]
        v = [rp.to_v(a[0]), rp.to_v(a[1])]
        for i in range(2):
            if not len(a[i]):
                continue
            cand = a[i][a[i]["score"] >= a[i]["score"][0] - po["pen_unpaired"]][:po["max_matesw"]]
            for j in range(len(cand)):
                t0 = time.perf_counter()
                n_sw += rp.matesw(pes, cand[j:j + 1], ms[i], v[1 - i])
                t_sw += time.perf_counter() - t0
                calls += 1
        libc.free(v[0].a)
        libc.free(v[1].a)
    return dict(mem_pestat_s=t_pestat, mem_matesw_s=t_sw, mem_matesw_calls=calls, ksw_align2_calls=int(n_sw),
                threads=1, note="time inside the reference's calls through ctypes; the loop's Python is not counted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rescue_bench.json"))
    a = ap.parse_args()
    opt, ref, bs = workload.load_fixture()
    b = bs[0].batch
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    alt = np.zeros(len(ref.ann_len), np.uint8)
    eng.set_alt(alt)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(dev)  # noqa: E731
    t = {k: up(getattr(b, k)) for k in ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid",
                                         "chain_frac_rep", "seeds")}
    bc = abi.BatchC()
    bc.n_reads, bc.n_chains, bc.n_seeds = b.n_reads, b.n_chains, b.n_seeds
    bc.seq_bytes = int(b.seq_off[-1])
    for k in t:
        setattr(bc, k, t[k].data_ptr())
    nr = b.n_reads
    regs = torch.zeros(b.n_seeds * 88, dtype=torch.uint8, device=dev)
    n = torch.zeros(nr, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    eng.chain2aln_device(bc, regs.data_ptr(), n.data_ptr(), None, s.cuda_stream)
    eng.regs_post_device(bc, None, regs.data_ptr(), n.data_ptr(), abi.POST_DEDUP_PATCH | abi.POST_MARK_ALT, 0, None,
                         s.cuda_stream)
    s.synchronize()
    h_n = n.cpu().numpy().view(np.int32).copy()
    slot = b.read_seed_off().astype(np.int64)  # the slot layout: read r's regions start at its first seed slot
    d_off = up(slot)
    out_off = np.concatenate([[0], np.cumsum(h_n.astype(np.int64) + HEADROOM)]).astype(np.int64)
    d_ooff = up(out_off)
    d_pes = torch.zeros(128, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(int(out_off[-1]) * 88, dtype=torch.uint8, device=dev)
    d_out_n = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_status = torch.zeros(nr // 2, dtype=torch.int32, device=dev)
    d_nsw = torch.zeros(nr // 2, dtype=torch.int32, device=dev)
    po = abi.default_pairopt()
    ms_pes, ms_res, parts = [], [], []
    with torch.cuda.stream(s):
        for k in range(a.warmup + a.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            eng.pestat_device(nr, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(), d_pes.data_ptr(), po, s.cuda_stream)
            e1.record(s)
            eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(),
                                   d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(),
                                   d_nsw.data_ptr(), po, s.cuda_stream)
            e2.record(s)
            e2.synchronize()
            if k >= a.warmup:
                ms_pes.append(e0.elapsed_time(e1))
                ms_res.append(e1.elapsed_time(e2))
                parts.append(eng.debug_rescue_times())
    st = eng.last_stats()
    status, n_sw = d_status.cpu().numpy().view(np.int32), d_nsw.cpu().numpy().view(np.int32)
    pes = d_pes.cpu().numpy().view(abi.PESTAT_DTYPE)
    res = dict(workload="tests/golden/c2_refseed.npz batch 0, resident, post-processed on the device (flags 3)",
               reads=int(nr), pairs=int(nr // 2), regions_in=int(h_n.sum()),
               regions_out=int(d_out_n.cpu().numpy().view(np.int32).sum()),
               pes=[dict(low=int(x["low"]), high=int(x["high"]), failed=int(x["failed"]), avg=float(x["avg"]),
                         std=float(x["std"])) for x in pes],
               pestat_device_ms=spread(ms_pes), mate_rescue_device_ms=spread(ms_res),
               plan_ms=spread([x["plan_ms"] for x in parts]), align2_ms=spread([x["align2_ms"] for x in parts]),
               apply_ms=spread([x["apply_ms"] for x in parts]), rounds=int(parts[-1]["rounds"]),
               tasks_speculated=int(st["ext_calls"]), tasks_used=int(n_sw[n_sw > 0].sum()),
               pairs_by_status={str(k): int((status == k).sum()) for k in range(4)},
               pairs_with_sw=int((n_sw > 0).sum()), output_headroom=HEADROOM)
    try:
        h_regs = regs.cpu().numpy().view(abi.ALNREG_DTYPE)
        by_read = [h_regs[slot[r]:slot[r] + h_n[r]].copy() for r in range(nr)]
        res["reference_cpu"] = cpu_reference(opt, ref, b, by_read, alt)
    except Exception as e:  # no reference library beside the tree
        res["reference_cpu"] = {"error": repr(e)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
