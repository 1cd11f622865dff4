"""The pair-selection fixtures (tests/golden/pair_*.npz, tools_dev/gen_pair_fixture.py)
load, are consistent, and cover what the generator's floors promise; the Python
mirrors of the new structs have the header's sizes and offsets.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.lib.recfunctions import repack_fields

import golden_io as G
import pair_io as P
from bwagpu import abi

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "bwagpu.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("bwagpu_selopt_t %zu\n", sizeof(bwagpu_selopt_t));
  F(bwagpu_selopt_t, T); F(bwagpu_selopt_t, pen_unpaired); F(bwagpu_selopt_t, min_seed_len);
  F(bwagpu_selopt_t, mapQ_coef_len); F(bwagpu_selopt_t, mapQ_coef_fac); F(bwagpu_selopt_t, mask_level);
  F(bwagpu_selopt_t, drop_ratio); F(bwagpu_selopt_t, flags);
  printf("bwagpu_pairsel_t %zu\n", sizeof(bwagpu_pairsel_t));
  F(bwagpu_pairsel_t, status); F(bwagpu_pairsel_t, branch); F(bwagpu_pairsel_t, n_pri); F(bwagpu_pairsel_t, z);
  F(bwagpu_pairsel_t, mapq); F(bwagpu_pairsel_t, alt); F(bwagpu_pairsel_t, extra_flag); F(bwagpu_pairsel_t, o);
  F(bwagpu_pairsel_t, subo); F(bwagpu_pairsel_t, n_sub);
  printf("consts %d %d %d %d %d %d %d %d %d %d %d\n", BWAGPU_SEL_DONE, BWAGPU_SEL_TOO_MANY, BWAGPU_SEL_SKIPPED,
         BWAGPU_SEL_NO_PAIRING, BWAGPU_SEL_PAIRED, BWAGPU_SEL_MAX_REGS, BWAGPU_MEM_F_NOPAIRING, BWAGPU_MEM_F_ALL,
         BWAGPU_MEM_F_NO_MULTI, BWAGPU_MEM_F_PRIMARY5, BWAGPU_MEM_F_KEEP_SUPP_MAPQ);
  return 0;
}
"""


def test_struct_layouts_equal_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line and not line.startswith("consts"))
    assert int(got.pop("bwagpu_selopt_t")) == C.sizeof(abi.SelOpt) == 32
    assert int(got.pop("bwagpu_pairsel_t")) == abi.PAIRSEL_DTYPE.itemsize == 64
    for key, off in got.items():
        struct, field = key.split(".")
        if struct == "bwagpu_selopt_t":
            assert getattr(abi.SelOpt, field).offset == int(off), key
        else:
            assert abi.PAIRSEL_DTYPE.fields[field][1] == int(off), key
    assert len(got) == 8 + 10
    consts = [int(x) for x in next(line for line in out if line.startswith("consts")).split()[1:]]
    assert consts == [abi.SEL_DONE, abi.SEL_TOO_MANY, abi.SEL_SKIPPED, abi.SEL_NO_PAIRING, abi.SEL_PAIRED,
                      abi.SEL_MAX_REGS, abi.MEM_F_NOPAIRING, abi.MEM_F_ALL, abi.MEM_F_NO_MULTI, abi.MEM_F_PRIMARY5,
                      abi.MEM_F_KEEP_SUPP_MAPQ]
    d = abi.default_selopt()
    assert (d.T, d.pen_unpaired, d.min_seed_len, d.mapQ_coef_fac, d.flags) == (30, 17, 19, 3, 0)
    assert (d.mapQ_coef_len, d.mask_level, d.drop_ratio) == (50.0, 0.5, 0.5)


def check(d):
    nr = d.n_reads
    assert nr % 2 == 0
    total = int(d.n.sum())
    assert len(d.regs) == len(d.marked) == len(d.final) == total
    assert len(d.n_pri) == nr and (d.n_pri >= 0).all() and (d.n_pri <= d.n).all()
    alt = (d.marked["n_comp_is_alt"] >> np.uint32(30)) != 0
    for r in range(nr):
        o, k = int(d.off[r]), int(d.n[r])
        a = alt[o:o + k]
        assert int((~a).sum()) == d.n_pri[r]
        if 0 < d.n_pri[r] < k:
            assert not a[:d.n_pri[r]].any() and a[d.n_pri[r]:].all()  # mem_ars_hash2 puts the ALT hits last
    # marking reorders and rewrites six fields; the selection rewrites three
    keep = [f for f in abi.ALNREG_DTYPE.names if f not in ("sub", "sub_n", "alt_sc", "secondary", "secondary_all", "hash")]
    for r in range(nr):
        o, k = int(d.off[r]), int(d.n[r])
        x, y = (np.sort(repack_fields(v[o:o + k][keep]), order=keep) for v in (d.regs, d.marked))
        assert x.tobytes() == y.tobytes()
    same = [f for f in abi.ALNREG_DTYPE.names if f not in ("sub", "secondary", "secondary_all")]
    assert repack_fields(d.final[same]).tobytes() == repack_fields(d.marked[same]).tobytes()
    for mode in (0, 1):
        sel, om = d.sel[mode], d.out_mapq[mode]
        assert len(sel) == nr // 2 and len(om) == total
        assert (sel["status"] == 0).all() and np.array_equal(sel["n_pri"].reshape(-1), d.n_pri)
        assert ((om >= -1) & (om <= 255)).all()
        assert set(np.unique(sel["extra_flag"]).tolist()) <= {1, 3}
    assert (d.sel[1]["branch"] == abi.SEL_NO_PAIRING).all() and (d.sel[1]["o"] == 0).all()
    assert (d.sel[1]["extra_flag"] == 1).all()
    s = d.sel[0]
    paired = s["branch"] == abi.SEL_PAIRED
    assert (s["extra_flag"][paired & (s["z"] != 0).any(axis=1)] == 3).all()
    for p in np.nonzero(paired)[0][:300]:
        for i in range(2):
            r = 2 * p + i
            z = int(s["z"][p][i])
            assert 0 <= z < d.n_pri[r]
            q = d.out_mapq[0][d.off[r]:d.off[r] + d.n[r]]
            assert q[z] == s["mapq"][p][i]
            emitted = set(np.nonzero(q >= 0)[0].tolist())
            assert emitted == {z} | ({int(s["alt"][p][i])} if s["alt"][p][i] >= 0 else set())


@pytest.mark.parametrize("name", P.PAIR_SETS)
def test_set_loads_and_is_consistent(name):
    assert os.path.getsize(os.path.join(G.GOLD, f"pair_{name}.npz")) <= 1 << 20
    d = P.load(name)
    assert d.n_reads >= 800
    check(d)


def test_pair_ids_cross_2_to_the_23():
    crossing = [n for n in P.PAIR_SETS
                if P.load(n).pair_id0 < (1 << 23) <= P.load(n).pair_id0 + P.load(n).n_reads // 2]
    assert len(crossing) >= 2


def test_floors_are_met():
    total = dict.fromkeys(P.COVERAGE_KEYS, 0)
    for name in P.PAIR_SETS:
        for k, v in P.load(name).coverage.items():
            total[k] += v
    short = {k: (total[k], f) for k, f in P.FLOORS.items() if total[k] < f}
    assert not short, f"coverage floors not met (have, need): {short}"
    assert (P.load("mixed").pes["failed"] == 0).sum() >= 2


def test_cases_load():
    assert os.path.getsize(os.path.join(G.GOLD, "pair_cases.npz")) <= 1 << 20
    cases = P.load_cases()
    for d in cases.values():
        check(d)
    cap = abi.SEL_MAX_REGS
    assert cases["n_cap"].n.max() == cap and cases["n_cap_plus_1"].n.max() == cap + 1
    assert cases["pri_cap_plus_1"].n_pri[:2].sum() == cap + 1
    assert cases["all_failed"].pes["failed"].tolist() == [1, 1, 1, 1]
    assert cases["dist_at_low_high"].sel[0]["branch"].tolist() == [1, 1, 0, 0]
    assert cases["only_alt"].n_pri[:2].tolist() == [0, 0]
    assert {int(cases[f"n{k}"].n.max()) for k in (16, 17, 64, 65)} == {16, 17, 64, 65}
