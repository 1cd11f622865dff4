#!/usr/bin/env python3
"""bwagpu_reg2aln_device against bwagpu_reg2aln_batch on the workload of
tools_dev/reg2aln_bench.py (the regions of one C2-shaped batch: 66.7k synthetic
2x150 reads vs a chr21-sized synthetic reference), the two forms alternating in
one process.

The device form, inputs and outputs resident: HIP events around the call
(call to stream completion), the host's wait at the bin table's read-back, the
span of the bin kernels alone (bwagpu_debug_reg2aln_times).  The batch form:
wall time and kernel_ms.  The device form's outputs are compared with the
batch form's.  One JSON line; --out also writes it to a file.

    python tools_dev/reg2aln_device_bench.py [--pairs N] [--warmup W] [--reps K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(REPO, "bwa-flow_amd", "python"))

from bwagpu import abi  # noqa: E402
from bwagpu.engine import Engine, unflatten  # noqa: E402
from bwagpu.synth import SynthRef, synth_batch  # noqa: E402


def spread(x):
    x = np.asarray(x, float)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()),
                p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=33334)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-kernel-ms", type=float, default=None,
                    help="kernel_ms of tools_dev/reg2aln_bench.py on the parent commit, same machine and job")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    opt = abi.default_opt()
    ref = SynthRef(42, 46_709_983, 1)
    b = synth_batch(ref, 1000, a.pairs, a.len)
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    regs, n = eng.chain2aln(b)
    jobs = []
    for r, p in enumerate(unflatten(b, regs, n)):
        for g in p:
            jobs.append((g["rb"], g["re"], b.seq_off[r], b.seq_off[r + 1] - b.seq_off[r], g["qb"], g["qe"],
                         g["truesc"], g["w"], 0))
    tasks = np.array(jobs, dtype=abi.REG2ALN_TASK_DTYPE)
    qpool = np.ascontiguousarray(b.seq, np.uint8)
    nj, max_ops, max_md = len(tasks), 64, 512
    dev = torch.device("cuda", 0)
    d_tasks = torch.from_numpy(tasks.view(np.uint8).copy()).to(dev)
    d_q = torch.from_numpy(qpool).to(dev)
    d_out = torch.zeros(nj * 40, dtype=torch.uint8, device=dev)
    d_cig = torch.zeros(nj * max_ops * 4, dtype=torch.uint8, device=dev)
    d_md = torch.zeros(nj * max_md, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, dev_host_ms, wait_ms, bins_ms, walls, kms = [], [], [], [], [], []
    eng.debug_reg2aln_times()  # switches the timing of the device form on
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        out, cig, md = eng.reg2aln_batch(tasks, qpool, max_ops, max_md)
        wall = 1e3 * (time.perf_counter() - t0)
        km = eng.last_stats()["kernel_ms"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        eng.reg2aln_device(nj, d_tasks.data_ptr(), d_q.data_ptr(), len(qpool), d_out.data_ptr(), d_cig.data_ptr(),
                           d_md.data_ptr(), max_ops, max_md, None, stream.cuda_stream)
        e1.record(stream)
        stream.synchronize()
        host = 1e3 * (time.perf_counter() - t0)
        tm = eng.debug_reg2aln_times()
        if it >= a.warmup:
            walls.append(wall)
            kms.append(km)
            dev_ms.append(e0.elapsed_time(e1))
            dev_host_ms.append(host)
            wait_ms.append(tm["wait_ms"])
            bins_ms.append(tm["bins_ms"])
    g_out = d_out.cpu().numpy().view(abi.ALN_DTYPE)
    g_cig = d_cig.cpu().numpy().view(np.uint32).reshape(nj, max_ops)
    g_md = d_md.cpu().numpy().reshape(nj, max_md)
    same = g_out.tobytes() == out.tobytes()
    ok = out["status"] == abi.ALN_OK
    cols = np.arange(max_ops)[None, :] < out["n_cigar"][:, None]
    same = same and bool(((g_cig == cig) | ~cols)[ok].all())
    cols = np.arange(max_md)[None, :] < out["md_len"][:, None]
    same = same and bool(((g_md == md) | ~cols)[ok].all())
    res = dict(metric="reg2aln_device vs reg2aln_batch", jobs=nj, reads=int(b.n_reads), warmup=a.warmup, reps=a.reps,
               device_call_to_completion_ms=spread(dev_ms), device_call_to_completion_host_clock_ms=spread(dev_host_ms),
               device_readback_wait_ms=spread(wait_ms),
               device_readback_wait_share=float(np.median(wait_ms) / np.median(dev_ms)),
               device_bin_kernels_ms=spread(bins_ms), batch_wall_ms=spread(walls), batch_kernel_ms=spread(kms),
               # the batch form's kernel_ms has modes: the span is compared with its lowest one
               # here, and with the parent commit's own run when that is given
               bins_over_batch_kernel_p10=float(np.median(bins_ms) / np.percentile(kms, 10)),
               parent_batch_kernel_ms=a.parent_kernel_ms,
               bins_over_parent_batch_kernel=(float(np.median(bins_ms) / a.parent_kernel_ms)
                                              if a.parent_kernel_ms else None),
               device_faster_than_batch_wall=bool(np.median(dev_ms) < np.median(walls)),
               status=np.bincount(g_out["status"], minlength=5).tolist(), outputs_equal_batch_form=bool(same))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
