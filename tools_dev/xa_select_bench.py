#!/usr/bin/env python3
"""mem_gen_alt's selection on one resident c2_refseed batch
(tests/golden/c2_refseed.npz batch 0: 33,334 interleaved 2x150 bp pairs) after
the device chain up to bwagpu_pair_select_device (pair_bench.py's set-up):
  (a) bwagpu_xa_select_device alone, by HIP events;
  (b) the CIGAR jobs its job_select asks for beside those of out_mapq alone;
  (c) the tail xa_select_device -> reg2aln_jobs_device -> reg2aln_device to
      stream completion, beside the same tail fed with out_mapq (no XA hits).
The device's xa_of and job_select are compared with the numpy restatement of
tests/xa_io.py over the whole batch.
-> profiles/xa_select_bench.json

    python tools_dev/xa_select_bench.py [--reps 30] [--out profiles/xa_select_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
for p in (os.path.join(REPO, "bwa-flow_amd", "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"),
          HERE):
    sys.path.insert(0, p)

import torch  # noqa: E402

import xa_io as X  # noqa: E402
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine  # noqa: E402
from pair_bench import HEADROOM, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "xa_select_bench.json"))
    a = ap.parse_args()
    opt, ref, bs = workload.load_fixture()
    b = bs[0].batch
    eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
    eng.set_alt(np.zeros(len(ref.ann_len), np.uint8))
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
    st = s.cuda_stream
    # the chain up to the pair selection, once
    eng.chain2aln_device(bc, regs.data_ptr(), n.data_ptr(), None, st)
    eng.regs_post_device(bc, None, regs.data_ptr(), n.data_ptr(), abi.POST_DEDUP_PATCH | abi.POST_MARK_ALT, 0, None, st)
    s.synchronize()
    h_n = n.cpu().numpy().view(np.int32).copy()
    d_off = up(b.read_seed_off().astype(np.int64))
    out_off = np.concatenate([[0], np.cumsum(h_n.astype(np.int64) + HEADROOM)]).astype(np.int64)
    d_ooff = up(out_off)
    n_slots = int(out_off[-1])
    i32 = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device=dev)  # noqa: E731
    d_pes = torch.zeros(128, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n_slots * 88, dtype=torch.uint8, device=dev)
    d_out_n, d_status, d_nsw = i32(nr), i32(nr // 2), i32(nr // 2)
    po, so = abi.default_pairopt(), abi.default_selopt()
    eng.pestat_device(nr, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(), d_pes.data_ptr(), po, st)
    eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(), d_ooff.data_ptr(),
                           d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(), d_nsw.data_ptr(), po, st)
    d_npri, d_mstat, d_mapq = i32(nr), i32(nr), i32(n_slots, -1)
    d_sel = torch.zeros(nr // 2 * 64, dtype=torch.uint8, device=dev)
    eng.mark_primary_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_npri.data_ptr(),
                            d_mstat.data_ptr(), 0, so, st)
    eng.pair_select_device(d_pes.data_ptr(), nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(),
                           d_npri.data_ptr(), d_status.data_ptr(), d_sel.data_ptr(), d_mapq.data_ptr(), 0, so, st)
    s.synchronize()
    h_out_n = d_out_n.cpu().numpy().view(np.int32).copy()
    cap = int(h_out_n.sum())
    max_ops, max_md = 64, 512
    d_xa, d_jsel, d_job_of, d_nj = i32(n_slots, -1), i32(n_slots, -1), i32(n_slots, -1), i32(2)
    d_tasks = torch.zeros(cap * 48, dtype=torch.uint8, device=dev)
    d_aln = torch.zeros(cap * 40, dtype=torch.uint8, device=dev)
    d_cig = torch.zeros(cap * max_ops * 4, dtype=torch.uint8, device=dev)
    d_md = torch.zeros(cap * max_md, dtype=torch.uint8, device=dev)

    def xa():
        eng.xa_select_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_sel.data_ptr(),
                             d_mapq.data_ptr(), d_xa.data_ptr(), d_jsel.data_ptr(), None, st)

    def cigars(select):
        eng.reg2aln_jobs_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), select.data_ptr(),
                                t["seq_off"].data_ptr(), cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(),
                                st)
        eng.reg2aln_device(cap, d_tasks.data_ptr(), t["seq"].data_ptr(), bc.seq_bytes, d_aln.data_ptr(),
                           d_cig.data_ptr(), d_md.data_ptr(), max_ops, max_md, d_nj.data_ptr(), st)

    def timed(fn):
        ms = []
        with torch.cuda.stream(s):
            for k in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                e1.synchronize()
                if k >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
        return spread(ms)

    res = dict(workload="tests/golden/c2_refseed.npz batch 0, resident, after the device chain up to pair_select_device",
               reads=int(nr), pairs=int(nr // 2), regions=cap, max_regions_per_read=int(h_out_n.max()))
    res["xa_select_device_ms"] = timed(xa)
    res["tail_without_xa_ms"] = timed(lambda: cigars(d_mapq))
    jobs_plain = d_nj.cpu().numpy().tolist()
    aln = d_aln.cpu().numpy().view(abi.ALN_DTYPE)[:jobs_plain[0]]
    res["jobs_of_out_mapq"] = dict(jobs=jobs_plain[1], by_status={str(k): int((aln["status"] == k).sum()) for k in range(5)})
    res["tail_with_xa_ms"] = timed(lambda: (xa(), cigars(d_jsel)))
    jobs_xa = d_nj.cpu().numpy().tolist()
    aln = d_aln.cpu().numpy().view(abi.ALN_DTYPE)[:jobs_xa[0]]
    res["jobs_of_job_select"] = dict(jobs=jobs_xa[1], by_status={str(k): int((aln["status"] == k).sum()) for k in range(5)})
    res["tail_note"] = ("each tail between two events on the stream, the host wait inside reg2aln_device (its bin table) "
                        "included")
    # the whole batch against the restatement
    sel = d_sel.cpu().numpy().view(abi.PAIRSEL_DTYPE)
    h_regs = d_out.cpu().numpy().view(abi.ALNREG_DTYPE)
    h_mapq = d_mapq.cpu().numpy()
    w_xa, w_job, ev = X.xa_model(out_off[:-1], h_regs, h_out_n, sel, h_mapq)
    res["equal_to_restatement"] = bool(np.array_equal(d_xa.cpu().numpy(), w_xa) and np.array_equal(d_jsel.cpu().numpy(), w_job))
    res["selection"] = dict(ev, pairs_by_status={str(k): int((sel["status"] == k).sum()) for k in range(3)},
                            regions_with_a_record=int((h_mapq >= 0).sum()), xa_hits=int((w_xa >= 0).sum()),
                            mate_records_without_a_record=int((w_job >= 0).sum() - ((h_mapq >= 0) | (w_xa >= 0)).sum()))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
