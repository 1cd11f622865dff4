"""The segment form of the ungapped certificate's diagonal scan (UngSeg and
ungseg_combine in bwa-flow_amd/csrc/ungapped.h): a side's bases
summarised in pieces {c, P, M, am} and folded in order must give what the
serial UngappedScan gives, whatever the pieces and the nesting of the fold.  On
the CPU: the header behind a small shim (tests/cpp/ungapped_seg_shim.cpp, built
here with g++), against

* the serial scan on random score sequences of 1 .. 160 bases, cut at every
  multiple of 16 and at random places, folded left- and right-nested;
* hand-made sequences: c comes back to M in a later segment (am stays the first
  index), M = 0, and P reaching oe_min only as the sum of two segments;
* the reference's recorded results of every golden ksw_extend2 set, wherever
  the certificate holds, and the serial form's certified mask on them.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_io as G
from bwagpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp, src, name):
    so = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fPIC", "-shared",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", src), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ungapped_seg")
    lib = build(tmp, "ungapped_seg_shim.cpp", "libungapped_seg_shim.so")
    lib.ungseg_serial.restype = None
    lib.ungseg_serial.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.ungseg_fold.restype = None
    lib.ungseg_fold.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.ungseg_batch.restype = C.c_int32
    lib.ungseg_batch.argtypes = [C.POINTER(abi.Opt), C.c_int32] + [C.c_void_p] * 5
    serial = build(tmp, "ungapped_shim.cpp", "libungapped_shim.so")
    serial.ungapped_batch.restype = C.c_int32
    serial.ungapped_batch.argtypes = lib.ungseg_batch.argtypes
    return lib, serial


def serial(lib, s, max_mat):
    s = np.ascontiguousarray(s, np.int32)
    out = np.zeros(4, np.int32)
    lib.ungseg_serial(s.ctypes.data, len(s), max_mat, out.ctypes.data)
    return tuple(int(x) for x in out)  # c, P, M, am


def fold(lib, s, max_mat, cuts, order):
    s = np.ascontiguousarray(s, np.int32)
    cuts = np.ascontiguousarray(cuts, np.int32)
    out = np.zeros(5, np.int32)
    lib.ungseg_fold(s.ctypes.data, len(s), max_mat, cuts.ctypes.data, len(cuts), order, out.ctypes.data)
    assert out[0] == len(s)
    return tuple(int(x) for x in out[1:])


def numpy_scan(s, max_mat):
    """the scan restated: c, P, M = max(0, max prefix sum), am = its first index + 1 (0 if M = 0)"""
    c = np.cumsum(np.asarray(s, np.int64))
    m = int(max(0, c.max()))
    return int(c[-1]), int(len(s) * max_mat - c[-1]), m, (int(np.argmax(c == m)) + 1 if m > 0 else 0)


def check_all_folds(lib, s, max_mat, cut_sets):
    want = serial(lib, s, max_mat)
    assert want == numpy_scan(s, max_mat), (list(s), want)
    for cuts in cut_sets:
        for order in (0, 1):
            got = fold(lib, s, max_mat, cuts, order)
            assert got == want, f"scores {list(s)}, cuts {list(cuts)}, order {order}: {got}, the serial scan has {want}"


def test_random_sequences(shim):
    lib, _ = shim
    rng = np.random.default_rng(26)
    for it in range(1500):
        n = int(rng.integers(1, 161))
        kind = it % 3
        if kind == 0:    # a read's diagonal: matches with a few mismatches and Ns
            s = np.where(rng.random(n) < 0.9, 1, np.where(rng.random(n) < 0.5, -4, -1))
            max_mat = 1
        elif kind == 1:  # a general matrix's scores
            s = rng.integers(-6, 5, n)
            max_mat = 4
        else:            # small steps: many ties of c with M
            s = rng.integers(-1, 2, n)
            max_mat = 1
        every16 = np.arange(16, n, 16)
        rnd = np.sort(rng.choice(np.arange(1, n), size=int(rng.integers(0, min(n - 1, 12) + 1)), replace=False)) if n > 1 else []
        every = np.arange(1, n)  # one base per segment
        check_all_folds(lib, s, max_mat, [every16, rnd, every, []])


def test_hand_made_sequences(shim):
    lib, _ = shim
    # c returns to M in later segments: M = 10 first at index 9 (am = 10), again at index 14 and, past the cut
    # at 16, at index 20
    tie = [1] * 10 + [-4] + [1] * 4 + [-1] * 3 + [1] * 3 + [-1] * 2
    assert numpy_scan(tie, 1)[2:] == (10, 10) and sum(tie[:15]) == 10 and sum(tie[:21]) == 10
    check_all_folds(lib, tie, 1, [[16], [10], [11], [15], [16, 20], [16, 21], list(range(1, len(tie)))])
    # ... and a tie exactly at a segment's first base
    tie2 = [1] * 16 + [-1, 1, -1, 1]
    assert numpy_scan(tie2, 1)[2:] == (16, 16)
    check_all_folds(lib, tie2, 1, [[16], [17], [16, 18], [8, 16]])
    # M = 0: the side never rises above its start (am = 0), with zero sums in later segments
    for s in ([-4] + [1] * 3, [-1] * 20, [0] * 33, [-4, 1, 1, 1, 1] + [0] * 20, [-1, 1] * 16):
        assert numpy_scan(s, 1)[2:] == (0, 0)
        check_all_folds(lib, s, 1, [np.arange(16, len(s), 16), [1], [2], list(range(1, len(s)))])
    # P reaches oe_min = 7 only as the sum of two segments: one mismatch (5) in pass k, one in pass k + 1
    two = [1] * 40
    two[12], two[20] = -4, -4
    got = fold(lib, two, 1, [16, 32], 1)
    assert got[1] == 10 and got == serial(lib, two, 1)
    halves = [fold(lib, two[:16], 1, [], 0)[1], fold(lib, two[16:32], 1, [], 0)[1], fold(lib, two[32:], 1, [], 0)[1]]
    assert halves == [5, 5, 0], "each segment alone stays below oe_min"
    check_all_folds(lib, two, 1, [[16, 32], [16], [32], [13, 21]])


@pytest.mark.parametrize("name", G.CHAIN_SETS + G.KSW_SETS)
def test_golden_sets(shim, name):
    lib, ser = shim
    opt, tasks, want, qp, tp = G.load_tasks(name)
    o = abi.opt_from_dict(opt)
    tasks = np.ascontiguousarray(tasks, abi.EXT_TASK_DTYPE)
    qp, tp = np.ascontiguousarray(qp, np.uint8), np.ascontiguousarray(tp, np.uint8)
    out = {}
    for key, fn in (("seg", lib.ungseg_batch), ("serial", ser.ungapped_batch)):
        res = np.zeros(max(len(tasks), 1), abi.EXT_RES_DTYPE)
        cert = np.zeros(max(len(tasks), 1), np.uint8)
        n = fn(C.byref(o), len(tasks), tasks.ctypes.data, qp.ctypes.data, tp.ctypes.data, res.ctypes.data, cert.ctypes.data)
        out[key] = (cert[:len(tasks)].astype(bool), res[:len(tasks)])
        assert n == int(out[key][0].sum())
    cert, got = out["seg"]
    print(f"{name}: {int(cert.sum())} of {len(tasks)} calls certified")
    assert np.array_equal(cert, out["serial"][0]), "the folded scan certifies other calls than the serial one"
    g, w = got.view(np.int32).reshape(-1, 6)[cert], want.view(np.int32).reshape(-1, 6)[cert]
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} certified calls differ; first {tasks[cert][bad[0]]}: {g[bad[0]]} want {w[bad[0]]}"
    if name == "c1_default":
        assert cert.sum() >= 400
