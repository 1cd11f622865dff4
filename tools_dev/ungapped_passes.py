#!/usr/bin/env python3
"""The ungapped certificate's round-A sides on the C2 fixture's batches, restated
in numpy on the batches' own bases (no GPU): the sides that hold
the certificate, those settled at sort time and the late right sides, and the
sixteen-base passes the certificate kernel issues (every side's first pass, and
every later pass of a side its first pass leaves alive) against the passes a
serial scan needs (one that stops at the end of the pass in which the side
dies).  Round A extends each chain's first seed in processing order, so its
tasks follow from the batch alone; round B's depend on the selection.

    python tools_dev/ungapped_passes.py [batches]"""
import json
import os
import sys

import numpy as np

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bwa-flow_amd", "python"))
from bwagpu import workload  # noqa: E402


def cal_max_gap(opt, qlen):
    l = max(int((qlen * opt["a"] - opt["o_del"]) / opt["e_del"]) + 1, int((qlen * opt["a"] - opt["o_ins"]) / opt["e_ins"]) + 1, 1)
    return min(l, opt["w"] << 1)


def fetch(ref, x0, n):
    x = np.arange(x0, x0 + n, dtype=np.int64)
    rev = x >= ref.l_pac
    f = np.where(rev, 2 * ref.l_pac - 1 - x, x)
    bs = (ref.pac[f >> 2].astype(np.int64) >> ((~f & 3) << 1)) & 3
    return np.where(rev, 3 - bs, bs)


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    opt, ref, rbs = workload.load_fixture()
    mat = np.asarray(opt["mat"], np.int64).reshape(5, 5)
    max_mat = int(max(0, mat.max()))
    oe_min = min(opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"])
    opt_ok = (opt["zdrop"] <= 0 or opt["zdrop"] >= oe_min) and (opt["w"] >> 1) + (opt["w"] >> 2) > 0 and max_mat >= 1
    l_pac = int(ref.l_pac)
    out = {"fixture": "c2_refseed", "round": "A", "batches": []}
    for k, rb in enumerate(rbs[:nb]):
        b = rb.batch
        cert_l = cert_r = settled = late = late_q = sides = call_ok = issued = serial = 0
        for rd in range(b.n_reads):
            lq = int(b.seq_off[rd + 1] - b.seq_off[rd])
            seq = b.seq[b.seq_off[rd]:b.seq_off[rd + 1]]
            for c in range(int(b.read_chain_off[rd]), int(b.read_chain_off[rd + 1])):
                sd = b.seeds[int(b.chain_seed_off[c]):int(b.chain_seed_off[c + 1])]
                if len(sd) == 0:
                    continue
                qbs, lns, rbs_ = sd["qbeg"].astype(np.int64), sd["len"].astype(np.int64), sd["rbeg"].astype(np.int64)
                lo = min(int(r - (q + cal_max_gap(opt, int(q)))) for r, q in zip(rbs_, qbs))
                hi = max(int(r + n + (lq - q - n) + cal_max_gap(opt, int(lq - q - n))) for r, q, n in zip(rbs_, qbs, lns))
                lo, hi = max(lo, 0), min(hi, 2 * l_pac)
                if lo < l_pac < hi:
                    if int(rbs_[0]) < l_pac:
                        hi = l_pac
                    else:
                        lo = l_pac
                rid = int(b.chain_rid[c])
                a0, al = int(ref.ann_offset[rid]), int(ref.ann_len[rid])
                if int(rbs_[0]) >= l_pac:
                    a0 = 2 * l_pac - (a0 + al)
                lo, hi = max(lo, a0), min(hi, a0 + al)
                t = max(range(len(sd)), key=lambda i: (int(sd[i]["score"]), i))
                rbeg, qb, ln = int(rbs_[t]), int(qbs[t]), int(lns[t])
                qr = lq - qb - ln
                ok = [False, False]
                for side, (q, x0, n, tlen, flip) in enumerate(((seq[:qb][::-1], rbeg - qb, qb, rbeg - lo, True),
                                                               (seq[qb + ln:], rbeg + ln, qr, hi - (rbeg + ln), False))):
                    if n == 0:
                        continue
                    sides += 1
                    if not (opt_ok and ln * opt["a"] >= oe_min and tlen >= n):
                        continue
                    call_ok += 1
                    tg = fetch(ref, x0, n)
                    if flip:
                        tg = tg[::-1]
                    loss = np.cumsum(max_mat - mat[tg, np.minimum(q, 4)])
                    ends = loss[np.minimum(np.arange(16, n + 16, 16), n) - 1]  # P at each pass's end
                    passes = len(ends)
                    dead = np.nonzero(ends >= oe_min)[0]
                    serial += int(dead[0]) + 1 if len(dead) else passes
                    issued += 1 if ends[0] >= oe_min else passes
                    ok[side] = len(dead) == 0
                cert_l += ok[0]
                cert_r += ok[1]
                in_l = qb > 0 and not ok[0]
                settled += int(ok[0]) + int(ok[1] and not in_l)
                late += int(ok[1] and in_l)
                late_q += qr if ok[1] and in_l else 0
        out["batches"].append({"batch": k, "reads": b.n_reads, "chains": b.n_chains, "sides": sides, "sides_call_ok": call_ok,
                               "certificate_holds": cert_l + cert_r, "settled_at_sort_time": settled, "late_right": late,
                               "late_right_bases": late_q, "passes_issued_dense": issued, "passes_serial_needs": serial,
                               "issued_over_serial": round(issued / max(serial, 1), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
