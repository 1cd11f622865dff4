"""The XA selection fixture (tests/golden/xa_select.npz, tools_dev/gen_xa_fixture.py)
loads, is consistent with the pair fixtures it extends and with the numpy
restatement the generator pinned, covers what the generator's floors promise,
and the hand-built cases say what they were built to say; the Python mirror of
bwagpu_samopt_t has the header's layout.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_io as G
import xa_io as X
from bwagpu import abi

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwagpu.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(bwagpu_samopt_t), offsetof(bwagpu_samopt_t, flags),
         offsetof(bwagpu_samopt_t, XA_drop_ratio), offsetof(bwagpu_samopt_t, max_XA_hits),
         offsetof(bwagpu_samopt_t, max_XA_hits_alt));
  return 0;
}
"""


def test_samopt_layout_equals_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = abi.SamOpt
    assert got == [C.sizeof(S), S.flags.offset, S.XA_drop_ratio.offset, S.max_XA_hits.offset,
                   S.max_XA_hits_alt.offset] == [16, 0, 4, 8, 12]
    d = abi.default_samopt()
    assert (d.flags, d.max_XA_hits, d.max_XA_hits_alt) == (0, 5, 200)
    assert float(d.XA_drop_ratio) == float(np.float32(0.8)) > 0.8  # why 80 under 100 is dropped


def test_file_size_and_floors():
    assert os.path.getsize(os.path.join(G.GOLD, "xa_select.npz")) <= 1 << 20
    cov = X.coverage()
    for k, floor in X.FLOORS.items():
        assert cov[k] >= floor, (k, cov[k], floor)


def counts_from(xa_of, d, mode):
    """hits per record from a selection: parallel to the regions, -1 where there is no record"""
    cnt = np.where(d.out_mapq[mode] >= 0, 0, -1).astype(np.int32)
    for r in range(d.n_reads):
        lo, n = int(d.off[r]), int(d.n[r])
        x = xa_of[lo:lo + n]
        np.add.at(cnt, lo + x[x >= 0], 1)
    return cnt


@pytest.mark.parametrize("mode", [0, 1], ids=["pairing", "nopairing"])
@pytest.mark.parametrize("name", X.SETS + ["cases"])
def test_restatement_gives_the_reference_counts(name, mode):
    d = X.load_cases() if name == "cases" else X.load(name)
    assert len(d.xa_cnt[mode]) == len(d.regs[mode]) == len(d.out_mapq[mode]) == int(d.n.sum())
    assert np.array_equal(d.xa_cnt[mode] < 0, d.out_mapq[mode] < 0)
    xa_of, job, ev = X.xa_model(d.off, d.regs[mode], d.n, d.sel[mode], d.out_mapq[mode])
    assert np.array_equal(counts_from(xa_of, d, mode), d.xa_cnt[mode])
    assert ev["hits"] == int(d.xa_cnt[mode][d.xa_cnt[mode] > 0].sum())
    # every record and every hit needs a CIGAR (an ALT record can be a hit of the primary's string too)
    assert ((job >= 0) >= ((xa_of >= 0) | (d.out_mapq[mode] >= 0))).all()


def test_cases_say_what_they_were_built_for():
    d = X.load_cases()
    first = {name: int(d.off[2 * p]) for p, name in enumerate(X.CASES)}
    for mode in (0, 1):
        c = d.xa_cnt[mode]
        assert c[first["at_cap"]] == 5 and c[first["over_cap"]] == 0 and c[first["alt_lifts_cap"]] == 6
        assert c[first["ratio_80_81"]] == 1  # 81 of 100 stays, 80 of 100 does not
        lo = first["two_strings"]
        assert c[lo:lo + 2].tolist() == [2, 1]
    # the primary under T: the paired branch prints it with its string, mem_reg2sam prints neither
    lo = first["primary_below_T"]
    assert d.xa_cnt[0][lo] == 2 and int(d.sel[0][X.CASES.index("primary_below_T")]["branch"]) == abi.SEL_PAIRED
    assert (d.xa_cnt[1][lo:lo + 3] == -1).all()
    _, _, ev = X.xa_model(d.off, d.regs[1], d.n, d.sel[1], d.out_mapq[1])
    assert ev["strings_unprinted"] == 1
    sc = d.regs[0]["score"][first["ratio_80_81"]:][:3]
    assert sorted(sc.tolist()) == [80, 81, 100]
