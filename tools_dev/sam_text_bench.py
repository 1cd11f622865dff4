#!/usr/bin/env python3
"""The SAM text of one resident c2_refseed batch (tests/golden/c2_refseed.npz batch 0:
33,334 interleaved 2x150 bp pairs) after the whole device chain (xa_select_bench.py's
set-up, then xa_select_device -> reg2aln_jobs_device -> reg2aln_device):
bwagpu_sam_text_device's three steps, each between HIP events on the stream
(bwagpu_debug_sam_text_step), the bytes written, the write pass's GB/s beside the
HBM bandwidth a streaming kernel reaches on this device, and the share of pairs
that keep the CPU path.  Names, qualities, comments and the read group are those
of tests/sam_io.py.
-> profiles/sam_text_bench.json

    python tools_dev/sam_text_bench.py [--reps 30] [--out profiles/sam_text_bench.json]
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

import sam_io as S  # noqa: E402
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine  # noqa: E402
from pair_bench import HEADROOM, spread  # noqa: E402

ACHIEVABLE_GBS = 6300.0  # a streaming float4 copy on this device


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sam_text_bench.json"))
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
    # the chain up to the records, once
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
    cap = int(d_out_n.cpu().numpy().view(np.int32).sum())
    max_ops, max_md = 64, 512
    d_xa, d_jsel, d_job_of, d_nj = i32(n_slots, -1), i32(n_slots, -1), i32(n_slots, -1), i32(2)
    d_tasks = torch.zeros(cap * 48, dtype=torch.uint8, device=dev)
    d_aln = torch.zeros(cap * 40, dtype=torch.uint8, device=dev)
    d_cig = torch.zeros(cap * max_ops * 4, dtype=torch.uint8, device=dev)
    d_md = torch.zeros(cap * max_md, dtype=torch.uint8, device=dev)
    eng.xa_select_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_sel.data_ptr(),
                         d_mapq.data_ptr(), d_xa.data_ptr(), d_jsel.data_ptr(), None, st)
    eng.reg2aln_jobs_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_jsel.data_ptr(),
                            t["seq_off"].data_ptr(), cap, d_tasks.data_ptr(), d_job_of.data_ptr(), d_nj.data_ptr(), st)
    eng.reg2aln_device(cap, d_tasks.data_ptr(), t["seq"].data_ptr(), bc.seq_bytes, d_aln.data_ptr(), d_cig.data_ptr(),
                       d_md.data_ptr(), max_ops, max_md, d_nj.data_ptr(), st)
    s.synchronize()
    jobs = d_nj.cpu().numpy().tolist()

    inp = S.read_inputs("c2", b.seq_off.astype(np.int64))
    c_off, c_names = S.contigs(len(ref.ann_len))
    keep = {k: up(v) for k, v in dict(inp, contig_off=c_off, contig_names=c_names).items()}
    d_toff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
    d_tstat = i32(nr // 2, -1)
    d_tn = torch.zeros(2, dtype=torch.int64, device=dev)
    x = abi.SamText()
    x.dev_reg_off, x.dev_regs, x.dev_n = d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr()
    x.dev_sel, x.dev_out_mapq, x.dev_xa_of = d_sel.data_ptr(), d_mapq.data_ptr(), d_xa.data_ptr()
    x.dev_job_of, x.dev_aln, x.dev_cigar, x.dev_md = d_job_of.data_ptr(), d_aln.data_ptr(), d_cig.data_ptr(), d_md.data_ptr()
    x.dev_seq_off, x.dev_seq, x.dev_qual = t["seq_off"].data_ptr(), t["seq"].data_ptr(), keep["qual"].data_ptr()
    x.dev_name_off, x.dev_names = keep["name_off"].data_ptr(), keep["names"].data_ptr()
    x.dev_comment_off, x.dev_comments = keep["comment_off"].data_ptr(), keep["comments"].data_ptr()
    x.dev_contig_off, x.dev_contig_names = keep["contig_off"].data_ptr(), keep["contig_names"].data_ptr()
    x.rg_id, x.flags, x.n_contigs, x.job_cap, x.max_ops, x.max_md = S.RG_ID, 0, len(ref.ann_len), cap, max_ops, max_md
    x.dev_text_off, x.dev_status, x.dev_text_n = d_toff.data_ptr(), d_tstat.data_ptr(), d_tn.data_ptr()
    # a first call without room gives the need
    x.text_cap, x.dev_text = 0, None
    eng.sam_text_device(x, nr, st)
    s.synchronize()
    need = int(d_tn.cpu().numpy()[1])
    d_text = torch.zeros(need, dtype=torch.uint8, device=dev)
    x.text_cap, x.dev_text = need, d_text.data_ptr()

    steps = [[], [], [], []]
    with torch.cuda.stream(s):
        for k in range(a.warmup + a.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(s)
            for step in range(3):
                eng.sam_text_device(x, nr, st, step=step)
                ev[step + 1].record(s)
            ev[3].synchronize()
            if k >= a.warmup:
                for step in range(3):
                    steps[step].append(ev[step].elapsed_time(ev[step + 1]))
                steps[3].append(ev[0].elapsed_time(ev[3]))
    by_step = d_text.cpu().numpy().tobytes()
    d_text.zero_()
    eng.sam_text_device(x, nr, st)
    s.synchronize()
    status = d_tstat.cpu().numpy()
    tn = d_tn.cpu().numpy().tolist()
    text = d_text.cpu().numpy().tobytes()
    res = dict(workload="tests/golden/c2_refseed.npz batch 0, resident, after the device chain up to reg2aln_device",
               reads=int(nr), pairs=int(nr // 2), jobs=jobs[1], max_ops=max_ops, max_md=max_md,
               count_ms=spread(steps[0]), scan_ms=spread(steps[1]), write_ms=spread(steps[2]), sum_ms=spread(steps[3]),
               bytes_written=tn[0], bytes_needed=tn[1], lines=text.count(b"\n"),
               steps_equal_whole_call=bool(by_step == text),
               pairs_by_status={str(k): int((status == k).sum()) for k in range(4)},
               share_of_pairs_with_a_status=float((status != 0).mean()))
    w = float(np.median(steps[2]))
    res["write_pass_GBs"] = tn[0] / w / 1e6
    res["achievable_write_GBs"] = ACHIEVABLE_GBS
    res["note"] = ("the write pass stores lane-parallel bytes; the LDS-staged form with aligned dword stores was not "
                   "built.  The reference's host mem_aln2sam was not timed on this batch.")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
