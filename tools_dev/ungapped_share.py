#!/usr/bin/env python3
"""What the ungapped certificate settles on the C2 fixture's
batches (tests/golden/c2_refseed.npz), per round: the sides settled at sort
time and their query bases (the DP rows they would have run) beside the sides
left on the phased lists (bwagpu_debug_spec_ungapped, device entry), and the
right sides settled after the left launch (DESIGN.md §26;
bwagpu_debug_spec_ungapped_right, where the library has it).

    python tools_dev/ungapped_share.py [batches]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(REPO, "bwa-flow_amd", "python"))
from bwagpu import abi, workload  # noqa: E402
from bwagpu.engine import Engine  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 2
opt, ref, rbs = workload.load_fixture()
eng = Engine(0, opt, ref.l_pac, ref.ann_offset, ref.ann_len, pac=ref.pac)
dev = torch.device("cuda:0")
fields = ("seq_off", "seq", "read_chain_off", "chain_seed_off", "chain_rid", "chain_frac_rep", "seeds")
out = {"fixture": "c2_refseed", "ungapped_right": eng.ungapped_right() if hasattr(eng.lib, "bwagpu_ctx_ungapped_right") else None,
       "batches": []}
for k, rb in enumerate(rbs[:nb]):
    b = rb.batch
    t = {f: torch.from_numpy(np.ascontiguousarray(getattr(b, f)).view(np.uint8).copy()).to(dev) for f in fields}
    regs = torch.zeros(max(b.n_seeds, 1) * 88, dtype=torch.uint8, device=dev)
    nn = torch.zeros(max(b.n_reads, 1), dtype=torch.int32, device=dev)
    c = abi.BatchC()
    c.n_reads, c.n_chains, c.n_seeds = b.n_reads, b.n_chains, b.n_seeds
    c.seq_bytes = int(b.seq_off[-1])
    for f in fields:
        setattr(c, f, t[f].data_ptr())
    st = torch.cuda.current_stream()
    eng.chain2aln_device(c, regs.data_ptr(), nn.data_ptr(), None, st.cuda_stream)
    torch.cuda.synchronize()
    ctr = np.zeros(12, np.int64)
    assert eng.lib.bwagpu_debug_spec_ungapped(eng.ctx, C.c_void_p(st.cuda_stream), ctr.ctypes.data_as(C.c_void_p)) == 0
    late = eng.ungapped_right_counters(st.cuda_stream) if hasattr(eng.lib, "bwagpu_debug_spec_ungapped_right") else None
    sh = np.zeros(9, np.int64)
    assert eng.lib.bwagpu_debug_spec_short(eng.ctx, C.c_void_p(st.cuda_stream), sh.ctypes.data_as(C.c_void_p)) == 0
    ok = rb.check(regs.cpu().numpy().view(abi.ALNREG_DTYPE)[:b.n_seeds], nn.cpu().numpy()[:b.n_reads])
    rounds = {}
    for r, name in enumerate("AB"):
        settled, bases, left, right = (int(x) for x in ctr[4 * r:4 * r + 4])
        rounds[name] = {"settled_sides": settled, "settled_bases": bases, "listed_left": left, "listed_right": right,
                        "settled_share_of_sides": round(settled / max(settled + left + right, 1), 4)}
        # the first bin's lists: the short run (sides of up to the short threshold) of each launch; it runs sixteen
        # per wave if it fills short_fill percent of the launch's sixteen-per-wave slots (spec_side4_kernel)
        ll, llong, rl, rlong = (int(x) for x in sh[1 + 4 * r:5 + 4 * r])
        rounds[name].update({"left_short_run": ll - llong, "right_short_run": rl - rlong})
        if late is not None:
            ln, lb = int(late[r, 0]), int(late[r, 1])
            rounds[name].update({"late_settled_right": ln, "late_settled_bases": lb,
                                 "late_share_of_right_sides_needing_a_left_dp": round(ln / max(ln + right, 1), 4),
                                 "late_share_of_side_calls": round(ln / max(ln + left + right, 1), 4)})
    out["batches"].append({"batch": k, "reads": b.n_reads, "sides_run_sixteen_per_wave": int(sh[0]), "regions_match_reference": bool(ok), "rounds": rounds})
print(json.dumps(out))
