"""bench.py --dump-outputs (bench.dump_outputs) on the CPU: the files hold the
step's per-read counts and its regions in read order, float64 and exact, the
same from call to call, and a batch past the size cap keeps a fixed sample."""
import os
import sys

import numpy as np
import pytest

import golden_io as G
from bwagpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step():
    """bench + a DevBatch in host memory whose output slot holds the golden
    regions of c1_default in the ABI's slot layout"""
    torch = pytest.importorskip("torch")
    keep = os.environ.get("BWAGPU_BENCH_KEEP_HWQ")
    os.environ["BWAGPU_BENCH_KEEP_HWQ"] = "1"  # importing bench must not change this process's HIP settings
    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
        if keep is None:
            del os.environ["BWAGPU_BENCH_KEEP_HWQ"]
        else:
            os.environ["BWAGPU_BENCH_KEEP_HWQ"] = keep
    _, b, want, want_n = G.load_chain_set("c1_default")
    d = bench.DevBatch(b, torch.device("cpu"))
    n = np.asarray(want_n, np.int64)
    where = np.repeat(b.read_seed_off().astype(np.int64), n) + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    regs = np.zeros(max(b.n_seeds, 1), abi.ALNREG_DTYPE)
    regs["rb"] = -1  # slots past a read's count are never dumped
    regs[where] = want
    out, cnt = d.outs[0]
    out.copy_(torch.from_numpy(regs.view(np.uint8).copy()))
    cnt.copy_(torch.from_numpy(np.asarray(want_n, np.int32)))
    return bench, d, want, want_n


def records(rows: np.ndarray) -> np.ndarray:
    """regions.npy's columns back into mem_alnreg_t records"""
    names = [f for f in abi.ALNREG_DTYPE.names if f != "hash"]
    assert rows.shape[1] == len(names) + 2
    r = np.zeros(len(rows), abi.ALNREG_DTYPE)
    for k, f in enumerate(names):
        r[f] = rows[:, k].astype(abi.ALNREG_DTYPE[f])
    r["hash"] = (rows[:, -2].astype(np.uint64) << np.uint64(32)) | rows[:, -1].astype(np.uint64)
    return r


def test_dump_is_exact_and_repeatable(step, tmp_path):
    bench, d, want, want_n = step
    for k in ("a", "b"):
        bench.dump_outputs(str(tmp_path / k), d, 0, 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["region_counts.npy", "regions.npy"]
    cnt, rows = np.load(tmp_path / "a" / "region_counts.npy"), np.load(tmp_path / "a" / "regions.npy")
    assert cnt.dtype == np.float64 and rows.dtype == np.float64
    assert np.array_equal(cnt, np.asarray(want_n, np.float64))
    assert len(want) > 0 and G.region_mismatch(records(rows), want) is None
    for f in ("region_counts.npy", "regions.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()


def test_dump_past_the_cap_keeps_a_fixed_sample(step, tmp_path, monkeypatch):
    bench, d, want, want_n = step
    keep = len(want) // 3
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", keep * 20 * 8)
    for k in ("a", "b"):
        bench.dump_outputs(str(tmp_path / k), d, 0, 0, 1)
    rows = np.load(tmp_path / "a" / "regions.npy")
    assert len(rows) == keep and rows.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(rows, np.load(tmp_path / "b" / "regions.npy"))
    # the sample is rows of the full dump, in order
    full = np.stack([want[f].astype(np.float64) for f in abi.ALNREG_DTYPE.names if f != "hash"], axis=1)
    j = 0
    for row in rows[:, :-2]:
        while not np.array_equal(full[j], row):
            j += 1
        j += 1
    assert np.array_equal(np.load(tmp_path / "a" / "region_counts.npy"), np.asarray(want_n, np.float64))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` in a process
    of its own: three timed steps, the headline's fields and none of --full's
    legs in the result line, and the last step's regions written"""
    import json
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "d")], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Mreads/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = reads of the three steps / their time
    reads = 3 * d["config"]["reads_per_batch"]
    assert d["value"] == pytest.approx(reads / (3 * d["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert d["parity_all_steps"] is None
    for leg in ("roofline", "roofline_hbm", "cpu_baseline", "two_batch_fixture", "hw_queues_4", "host_buffer_path",
                "end_to_end", "end_to_end_align", "cigar_stage", "seeding_stage", "chaining_stage", "regime_grch38",
                "c5_refseed"):
        assert leg not in d
    cnt, rows = np.load(tmp_path / "d" / "region_counts.npy"), np.load(tmp_path / "d" / "regions.npy")
    assert cnt.dtype == np.float64 and rows.dtype == np.float64 and rows.shape[1] == 20
    assert len(cnt) > 0 and int(cnt.sum()) == len(rows) > 0
    assert cnt.nbytes + rows.nbytes <= 64 << 20


def test_dump_names_of_later_ranks(step, tmp_path):
    bench, d, _, _ = step
    bench.dump_outputs(str(tmp_path), d, 0, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["region_counts_rank1.npy", "regions_rank1.npy"]
