"""The region post-processing fixtures (tests/golden/post_*.npz): they load,
their coverage meets the generator's floors, the reference's outputs obey the
invariants of mem_sort_dedup_patch / mem_mark_primary_se, and abi.PostOpt is
the header's bwagpu_postopt_t."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import golden_io as G
import post_io as P
from bwagpu import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = np.uint32(0x3fffffff)


@pytest.mark.parametrize("name", P.POST_SETS)
def test_fixture_loads_and_is_consistent(name):
    s = P.load(name)
    nr = len(s.seq_off) - 1
    assert len(s.n) == nr and int(s.n.sum()) == len(s.regs)
    assert int(np.diff(s.seq_off).max()) <= abi.MAX_READ_LEN
    for flags in (3, 7):
        regs, n = s.want[flags]
        assert len(n) == nr and int(n.sum()) == len(regs)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", f"post_{name}.npz")) <= 1 << 20


def test_coverage_floors():
    total = dict.fromkeys(P.COVERAGE_KEYS, 0)
    for name in P.POST_SETS:
        for k, v in P.load(name).coverage.items():
            total[k] += v
    short = {k: (total[k], P.FLOORS[k]) for k in P.COVERAGE_KEYS if total[k] < P.FLOORS[k]}
    assert not short, f"coverage below the floors (have, need): {short}"


@pytest.mark.parametrize("name", P.POST_SETS)
def test_expected_outputs_obey_the_invariants(name):
    s = P.load(name)
    r3, n3 = s.want[3]
    r7, n7 = s.want[7]
    assert np.array_equal(n3, n7)
    assert (n3 <= s.n).all()
    assert (r3["qe"] > r3["qb"]).all() and (r7["qe"] > r7["qb"]).all()
    o3 = G.offsets(n3)
    # a read with n <= 1 is unchanged apart from the flags (is_alt; with flag 4 also
    # sub / alt_sc / secondary / secondary_all / hash)
    one = np.nonzero(s.n == 1)[0]
    assert (n3[one] == 1).all() and (n3[s.n == 0] == 0).all()
    assert len(one) or name in ("rep_redun1", "c5_refseed")  # these two hold heavy reads only
    a, b, c = s.regs[s.off[one]].copy(), r3[o3[one]].copy(), r7[o3[one]].copy()
    assert ((a["n_comp_is_alt"] & COMP) == (b["n_comp_is_alt"] & COMP)).all()  # n_comp stays 0 (bwamem.c:449)
    for x in (a, b, c):
        x["n_comp_is_alt"] = 0
    assert a.tobytes() == b.tobytes()
    assert (c["secondary"] == -1).all() and (c["secondary_all"] == -1).all() and (c["sub"] == 0).all()
    for f in ("sub", "alt_sc", "secondary", "secondary_all", "hash"):
        a[f] = 0
        c[f] = 0
    assert a.tobytes() == c.tobytes()
    # the ALT bit follows the table
    rid = r3["rid"]
    assert np.array_equal((r3["n_comp_is_alt"] >> np.uint32(30)) != 0, s.alt[rid] != 0)


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "bwagpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d %d %d\n", sizeof(bwagpu_postopt_t), offsetof(bwagpu_postopt_t, max_chain_gap),
         offsetof(bwagpu_postopt_t, mask_level_redun), offsetof(bwagpu_postopt_t, mask_level),
         offsetof(bwagpu_postopt_t, pad_), BWAGPU_POST_DEDUP_PATCH, BWAGPU_POST_MARK_ALT, BWAGPU_POST_PRIMARY);
  return 0;
}
"""


def test_postopt_matches_the_header():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(LAYOUT_C)
        subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), src, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    T = abi.PostOpt
    assert got == [C.sizeof(T), T.max_chain_gap.offset, T.mask_level_redun.offset, T.mask_level.offset,
                   T.pad_.offset, abi.POST_DEDUP_PATCH, abi.POST_MARK_ALT, abi.POST_PRIMARY]
    assert got[0] == 16
    d = abi.default_postopt()
    assert (d.max_chain_gap, d.mask_level_redun, d.mask_level) == (10000, np.float32(0.95), 0.5)
    for f in ("bwagpu_regs_post", "bwagpu_regs_post_device", "bwagpu_set_regs_post"):
        assert f in abi.PROTOS and hasattr(abi.load(), f)
