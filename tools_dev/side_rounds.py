#!/usr/bin/env python3
"""The phased extension's side launches per round from a rocprofv3 kernel trace
(tools_dev/gpu_trace.sh, one caller stream): the average launch time of the
left and the right spec_side4_kernel of round A and of round B over the timed
steps (a sequence's side launches in launch order: A left, A right, B left,
B right).

    python tools_dev/side_rounds.py <run_kernel_trace.csv> [warmup] [steps]"""
import json
import sys

from trace_busy import load, sequences

path = sys.argv[1]
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
seqs = sequences(load(path))[warmup:warmup + steps]
names = ("A_left", "A_right", "B_left", "B_right")
tot = dict.fromkeys(names, 0.0)
n = 0
for q in seqs:
    side = [r for r in q if r["name"].startswith("spec_side4_kernel<16, 10, true")]
    if len(side) != 4:
        continue
    assert [r["name"].endswith("true>") for r in side] == [False, True, False, True], [r["name"] for r in side]
    for k, r in zip(names, side):
        tot[k] += (r["e"] - r["s"]) / 1e6
    n += 1
out = {"trace": path, "steps": n, "avg_launch_ms": {k: round(v / max(n, 1), 4) for k, v in tot.items()}}
out["sum_ms_per_step"] = round(sum(tot.values()) / max(n, 1), 4)
t0 = min(r["s"] for q in seqs for r in q)
t1 = max(r["e"] for q in seqs for r in q)
out["window_ms_per_step"] = round((t1 - t0) / 1e6 / max(len(seqs), 1), 4)
print(json.dumps(out))
