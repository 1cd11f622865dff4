"""GPU parity of bwagpu_mark_primary / bwagpu_mark_primary_device: mem_mark_primary_se on
the device, byte for byte against the reference's own results: the flags-7 regions of
tests/golden/post_*.npz from their flags-3 regions, and the marked regions of
tests/golden/pair_*.npz, through the host and the device entry."""
import ctypes as C

import numpy as np
import pytest

import golden_io as G
import pair_io as P
import post_io as PO
from bwagpu import abi
from bwagpu.engine import BwaGpuError, Engine

pytestmark = pytest.mark.gpu

_engines = {}


def engine(opt, genome_key, g) -> Engine:
    key = (genome_key, tuple(int(opt[k]) for k in G.OPT_KEYS), bytes(np.asarray(opt["mat"], np.int8)))
    if key not in _engines:
        _engines[key] = Engine(0, opt, g["l_pac"], g["ann_offset"], g["ann_len"], pac=g["pac"])
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def to_dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).copy()
    if b.size == 0:  # a batch without regions still hands the entry a valid pointer
        b = np.zeros(88, np.uint8)
    return torch.from_numpy(b).to(torch.device("cuda", 0))


def mark_device(torch, eng, off, regs, n, id0, so):
    dev = torch.device("cuda", 0)
    d_off, d_regs, d_n = to_dev(torch, off), to_dev(torch, regs), to_dev(torch, n)
    d_npri = torch.full((max(len(n), 1),), -7, dtype=torch.int32, device=dev)
    d_status = torch.full((max(len(n), 1),), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    eng.mark_primary_device(len(n), d_off.data_ptr(), d_regs.data_ptr(), d_n.data_ptr(), d_npri.data_ptr(),
                            d_status.data_ptr(), id0, so, stream.cuda_stream)
    stream.synchronize()
    return (d_regs.cpu().numpy().view(abi.ALNREG_DTYPE)[:len(regs)], d_npri.cpu().numpy()[:len(n)],
            d_status.cpu().numpy()[:len(n)])


def check(eng, torch, what, off, regs, n, id0, so, want_regs, want_npri):
    """host entry twice on fresh copies and the device entry: all equal the reference"""
    before = regs.copy()
    runs = [eng.mark_primary(off, regs, n, id0, so), eng.mark_primary(off, regs.copy(), n, id0, so),
            mark_device(torch, eng, off, regs, n, id0, so)]
    assert regs.tobytes() == before.tobytes()
    for k, (got, n_pri, status) in enumerate(runs):
        w = f"{what} (run {k})"
        assert (status == abi.SEL_DONE).all(), f"{w}: status {np.unique(status).tolist()}"
        bad = G.region_mismatch(got, want_regs)
        assert bad is None, f"{w}: {bad}"
        assert got.tobytes() == want_regs.tobytes(), w
        if want_npri is not None:
            assert np.array_equal(n_pri, want_npri), f"{w}: n_pri differs at reads {np.nonzero(n_pri != want_npri)[0][:8].tolist()}"
    assert eng.last_stats()["kernel_ms"] >= 0


@pytest.mark.parametrize("name", PO.POST_SETS)
def test_post_sets_flags3_to_flags7(name):
    torch = pytest.importorskip("torch")
    s = PO.load(name)
    regs3, n3 = s.want[3]
    regs7, n7 = s.want[7]
    assert np.array_equal(n3, n7)
    eng = engine(s.opt, s.genome, PO.genome(s.genome))
    so = abi.default_selopt()
    so.mask_level = float(s.popt.mask_level)
    alt = (regs7["n_comp_is_alt"] >> np.uint32(30)) != 0
    off = G.offsets(n3)
    want_npri = np.array([int((~alt[o:o + k]).sum()) for o, k in zip(off, n3)], np.int32)
    assert n3.max() <= abi.SEL_MAX_REGS
    check(eng, torch, f"post_{name}", off, regs3, n3, s.id0, so, regs7, want_npri)


@pytest.mark.parametrize("name", P.PAIR_SETS)
def test_pair_sets(name):
    torch = pytest.importorskip("torch")
    d = P.load(name)
    eng = engine(d.opt, ("pair", d.genome_id, name if d.genome_id else ""), d.genome)
    check(eng, torch, f"pair_{name}", d.off, d.regs, d.n, 2 * d.pair_id0, d.selopt(), d.marked, d.n_pri)


@pytest.mark.parametrize("case", [c for c in P.CASES if c != "n_cap_plus_1"])
def test_hand_built_cases(case):
    torch = pytest.importorskip("torch")
    d = P.load_cases()[case]
    eng = engine(d.opt, ("pair", 0, ""), d.genome)
    check(eng, torch, case, d.off, d.regs, d.n, 2 * d.pair_id0, d.selopt(), d.marked, d.n_pri)


def test_a_read_over_the_cap_is_left_untouched():
    torch = pytest.importorskip("torch")
    d = P.load_cases()["n_cap_plus_1"]
    eng = engine(d.opt, ("pair", 0, ""), d.genome)
    assert d.n[0] == abi.SEL_MAX_REGS + 1
    for got, n_pri, status in (eng.mark_primary(d.off, d.regs, d.n, 2 * d.pair_id0, d.selopt()),
                               mark_device(torch, eng, d.off, d.regs, d.n, 2 * d.pair_id0, d.selopt())):
        assert status.tolist() == [abi.SEL_TOO_MANY, 0, 0, 0] and n_pri[0] == 0
        k = int(d.n[0])
        assert got[:k].tobytes() == d.regs[:k].tobytes()
        assert got[k:].tobytes() == d.marked[k:].tobytes() and np.array_equal(n_pri[1:], d.n_pri[1:])


def test_spans_with_gaps_and_empty_batch():
    d = P.load("ends")
    eng = engine(d.opt, ("pair", d.genome_id, ""), d.genome)
    nr = 200
    n = d.n[:nr]
    off = (np.cumsum(n.astype(np.int64) + 3) - n - 3 + 5).astype(np.int64)  # 3 records between spans, 5 in front
    regs = np.zeros(int(off[-1] + n[-1]) + 2, abi.ALNREG_DTYPE)
    regs["score"] = -12345
    for r in range(nr):
        regs[off[r]:off[r] + n[r]] = d.regs[d.off[r]:d.off[r] + n[r]]
    got, n_pri, status = eng.mark_primary(off, regs, n, 2 * d.pair_id0, d.selopt())
    assert (status == 0).all() and np.array_equal(n_pri, d.n_pri[:nr])
    used = np.zeros(len(regs), bool)
    for r in range(nr):
        used[off[r]:off[r] + n[r]] = True
        assert got[off[r]:off[r] + n[r]].tobytes() == d.marked[d.off[r]:d.off[r] + n[r]].tobytes(), f"read {r}"
    assert got[~used].tobytes() == regs[~used].tobytes()
    got, n_pri, status = eng.mark_primary(np.zeros(0, np.int64), np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32))
    assert len(got) == 0 and len(n_pri) == 0 and len(status) == 0


def test_errors_launch_nothing():
    d = P.load("fr")
    eng = engine(d.opt, ("pair", d.genome_id, ""), d.genome)
    nr = 40
    n, off = d.n[:nr], d.off[:nr]
    regs = d.regs[:int(n.sum())]
    eng.mark_primary(off, regs, n, 0, d.selopt())
    before = eng.last_stats()

    def code(off=off, regs=regs, n=n, so=d.selopt()):
        with pytest.raises(BwaGpuError) as e:
            eng.mark_primary(off, regs, n, 0, so)
        return e.value.code

    bad_n = n.copy()
    bad_n[3] = -1
    assert code(n=bad_n) == abi.E_INVAL
    over = off.copy()
    over[5] = off[4]
    assert code(off=over) == abi.E_INVAL  # spans overlap
    so = d.selopt()
    so.mask_level = float("nan")
    assert code(so=so) == abi.E_INVAL
    lib = eng.lib
    so = d.selopt()
    assert lib.bwagpu_mark_primary(eng.ctx, C.byref(so), 0, nr, None, None, None, None, None) == abi.E_INVAL
    assert lib.bwagpu_mark_primary(eng.ctx, None, 0, 0, None, None, None, None, None) == abi.E_INVAL
    assert lib.bwagpu_mark_primary_device(eng.ctx, C.byref(so), 0, nr, None, None, None, None, None, None) == abi.E_INVAL
    assert eng.last_stats() == before
    # the flag bwagpu_regs_post reserves for this pass stays refused there
    with pytest.raises(BwaGpuError) as e:
        eng.regs_post(np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, abi.ALNREG_DTYPE),
                      np.zeros(0, np.int32), abi.POST_PRIMARY)
    assert e.value.code == abi.E_UNSUPPORTED
