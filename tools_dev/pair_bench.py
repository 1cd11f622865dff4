#!/usr/bin/env python3
"""Primary marking and pair selection on one resident c2_refseed batch
(tests/golden/c2_refseed.npz batch 0: 33,334 interleaved 2x150 bp pairs) after
the device's post-processing, mem_pestat and mate rescue:
bwagpu_mark_primary_device and bwagpu_pair_select_device per batch by HIP
events (the regions are restored from a device copy before every run: both
passes work in place), beside the reference's mem_mark_primary_se, mem_pair and
mem_approx_mapq_se over the same regions on one host thread
(oracle/_ref/libbwaref.so through ctypes: only the time inside the three
functions is counted, the glue between them is Python and is not).
-> profiles/pair_bench.json

    python tools_dev/pair_bench.py [--reps 30] [--out profiles/pair_bench.json]
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


class TimedLib:
    """the reference library with the seconds spent inside each function"""

    def __init__(self, lib):
        self._lib, self.seconds, self.calls = lib, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            t0 = time.perf_counter()
            r = fn(*a)
            self.seconds[name] = self.seconds.get(name, 0.0) + time.perf_counter() - t0
            self.calls[name] = self.calls.get(name, 0) + 1
            return r
        return call


def cpu_reference(opt, ref, regs_by_read, pes, alt):
    """-> (the restated reference's record per pair, seconds inside its three functions on one thread)"""
    from gen_pair_fixture import COVERAGE_KEYS, RefSel
    po = dict(max_ins=10000, max_matesw=50, pen_unpaired=17, min_seed_len=19, max_chain_gap=10000,
              mask_level_redun=0.95, mask_level=0.50)
    refd = dict(l_pac=ref.l_pac, ann_offset=ref.ann_offset, ann_len=ref.ann_len, pac=ref.pac)
    rs = RefSel(opt, po, refd, alt)
    rs.lib = tl = TimedLib(rs.lib)
    branch = [0, 0]
    recs = []
    for p in range(len(regs_by_read) // 2):
        m, npri = zip(*[rs.mark(regs_by_read[2 * p + i], 2 * p + i) for i in range(2)])
        rec, _, _ = rs.select(list(m), list(npri), pes, p, False, dict.fromkeys(COVERAGE_KEYS, 0))
        branch[int(rec["branch"])] += 1
        recs.append(rec)
    keys = ("mem_mark_primary_se", "mem_pair", "mem_approx_mapq_se")
    times = dict({k + "_s": tl.seconds.get(k, 0.0) for k in keys}, **{k + "_calls": tl.calls.get(k, 0) for k in keys},
                 total_s=sum(tl.seconds.get(k, 0.0) for k in keys), pairs_paired=branch[1], pairs_no_pairing=branch[0],
                 threads=1, note="time inside the reference's calls through ctypes (its call overhead included); "
                                 "the glue of mem_sam_pe between them is Python and is not counted")
    return np.array(recs, abi.PAIRSEL_DTYPE), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_bench.json"))
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
    st = s.cuda_stream
    eng.chain2aln_device(bc, regs.data_ptr(), n.data_ptr(), None, st)
    eng.regs_post_device(bc, None, regs.data_ptr(), n.data_ptr(), abi.POST_DEDUP_PATCH | abi.POST_MARK_ALT, 0, None, st)
    s.synchronize()
    h_n = n.cpu().numpy().view(np.int32).copy()
    d_off = up(b.read_seed_off().astype(np.int64))  # the slot layout
    out_off = np.concatenate([[0], np.cumsum(h_n.astype(np.int64) + HEADROOM)]).astype(np.int64)
    d_ooff = up(out_off)
    d_pes = torch.zeros(128, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(int(out_off[-1]) * 88, dtype=torch.uint8, device=dev)
    d_out_n = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_status = torch.zeros(nr // 2, dtype=torch.int32, device=dev)
    d_nsw = torch.zeros(nr // 2, dtype=torch.int32, device=dev)
    po = abi.default_pairopt()
    eng.pestat_device(nr, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(), d_pes.data_ptr(), po, st)
    eng.mate_rescue_device(d_pes.data_ptr(), bc, d_off.data_ptr(), regs.data_ptr(), n.data_ptr(), d_ooff.data_ptr(),
                           d_out.data_ptr(), d_out_n.data_ptr(), d_status.data_ptr(), d_nsw.data_ptr(), po, st)
    s.synchronize()
    rescued = d_out.clone()  # the passes work in place: every run starts from this copy
    h_out_n = d_out_n.cpu().numpy().view(np.int32).copy()
    d_npri = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_mstat = torch.zeros(nr, dtype=torch.int32, device=dev)
    d_sel = torch.zeros(nr // 2 * 64, dtype=torch.uint8, device=dev)
    d_mapq = torch.zeros(int(out_off[-1]), dtype=torch.int32, device=dev)
    so = abi.default_selopt()
    ms_mark, ms_sel = [], []
    with torch.cuda.stream(s):
        for k in range(a.warmup + a.reps):
            d_out.copy_(rescued)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record(s)
            eng.mark_primary_device(nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(), d_npri.data_ptr(),
                                    d_mstat.data_ptr(), 0, so, st)
            e1.record(s)
            eng.pair_select_device(d_pes.data_ptr(), nr, d_ooff.data_ptr(), d_out.data_ptr(), d_out_n.data_ptr(),
                                   d_npri.data_ptr(), d_status.data_ptr(), d_sel.data_ptr(), d_mapq.data_ptr(), 0, so, st)
            e2.record(s)
            e2.synchronize()
            if k >= a.warmup:
                ms_mark.append(e0.elapsed_time(e1))
                ms_sel.append(e1.elapsed_time(e2))
    sel = d_sel.cpu().numpy().view(abi.PAIRSEL_DTYPE)
    mstat = d_mstat.cpu().numpy().view(np.int32)
    h_npri = d_npri.cpu().numpy().view(np.int32)
    pes = d_pes.cpu().numpy().view(abi.PESTAT_DTYPE).copy()
    res = dict(workload="tests/golden/c2_refseed.npz batch 0, resident, after regs_post (flags 3), pestat and mate rescue "
                        "on the device",
               reads=int(nr), pairs=int(nr // 2), regions=int(h_out_n.sum()),
               reads_with_2_or_more_regions=int((h_out_n >= 2).sum()), max_regions_per_read=int(h_out_n.max()),
               pairs_needing_the_wave_mem_pair=int(((h_npri[0::2] >= 1) & (h_npri[1::2] >= 1)
                                                    & (h_npri[0::2] + h_npri[1::2] > 2)).sum()),
               mark_primary_device_ms=spread(ms_mark),
               pair_select_device_ms=spread(ms_sel),
               pair_select_note="the whole entry between two events: the read-back of pes, the host's erfc tables "
                                "and their upload (each a stream wait) and the kernel",
               reads_by_mark_status={str(k): int((mstat == k).sum()) for k in range(3)},
               pairs_by_status={str(k): int((sel["status"] == k).sum()) for k in range(3)},
               pairs_paired=int(((sel["status"] == 0) & (sel["branch"] == 1)).sum()),
               pes=[dict(low=int(x["low"]), high=int(x["high"]), failed=int(x["failed"])) for x in pes])
    try:
        h_regs = rescued.cpu().numpy().view(abi.ALNREG_DTYPE)
        by_read = [h_regs[out_off[r]:out_off[r] + h_out_n[r]].copy() for r in range(nr)]
        want, res["reference_cpu"] = cpu_reference(opt, ref, by_read, pes, alt)
        done = sel["status"] == 0  # the others are left to the CPU path (rescue overflow, over the cap)
        res["reference_cpu"]["records_equal_on_done_pairs"] = bool(sel[done].tobytes() == want[done].tobytes())
    except Exception as e:  # no reference library beside the tree
        res["reference_cpu"] = {"error": repr(e)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
