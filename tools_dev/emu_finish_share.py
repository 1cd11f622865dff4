#!/usr/bin/env python3
"""What the emulate selection pass finishes on the C2 fixture's
batches (tests/golden/c2_refseed.npz): the narrow and the wider light reads it
writes itself, the light reads it lists for the final pass and the batch's
light reads (bwagpu_debug_spec_finish, device entry), beside the round-B tasks.

    python tools_dev/emu_finish_share.py [batches]"""
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
out = {"fixture": "c2_refseed", "emu_finish": eng.emu_finish(), "batches": []}
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
    fc, sc = np.zeros(4, np.int64), np.zeros(8, np.int64)
    assert eng.lib.bwagpu_debug_spec_finish(eng.ctx, C.c_void_p(st.cuda_stream), fc.ctypes.data_as(C.c_void_p)) == 0
    assert eng.lib.bwagpu_debug_spec_counters(eng.ctx, C.c_void_p(st.cuda_stream), sc.ctypes.data_as(C.c_void_p)) == 0
    ok = rb.check(regs.cpu().numpy().view(abi.ALNREG_DTYPE)[:b.n_seeds], nn.cpu().numpy()[:b.n_reads])
    nar, wide, listed, light = (int(x) for x in fc)
    out["batches"].append({"batch": k, "reads": b.n_reads, "regions_match_reference": bool(ok),
                           "finished_narrow": nar, "finished_wide": wide, "listed": listed, "light_reads": light,
                           "finished_share_of_light": round((nar + wide) / max(light, 1), 4),
                           "round_B_tasks": int(sc[1]), "heavy_reads": int(sc[5])})
print(json.dumps(out))
