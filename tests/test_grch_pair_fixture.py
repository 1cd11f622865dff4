"""The GRCh38-regime fixtures of the post / rescue / pair stages (tests/golden/grch_*.npz,
tools_dev/gen_grch_pair_fixture.py) load against the regenerated composite genome and the
translated inputs, are consistent, and reach the coverage floors: coordinates past 2^31 and
2^32 in the inputs, in what the rescue adds, in what mem_patch_reg patches, in clamped
windows and in proper pairs of both copies.  Where oracle/_ref is built, the reference is
run again on the first 50 pairs of one set.  CPU only."""
import os
import sys

import numpy as np
import pytest

import golden_io as G
import grch_io as GI
import oracle
from bwagpu import abi
from test_pair_fixture import check

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_files_are_small():
    for f in GI.all_files():
        assert os.path.getsize(os.path.join(G.GOLD, f)) <= 1 << 20, f


def test_composite_genome_and_translation():
    c = GI.composite()
    assert c.l_small == 1_000_000 and c.rid_b == 198 and len(c.genome["ann_len"]) == 201
    assert len(c.genome["pac"]) == c.l_pac // 4 + 1  # a .pac file's length, which bwagpu_create asks for
    assert c.off_b > 1 << 31 and c.off_b + 2 * c.l_small < 1 << 32 and 2 * (c.l_pac - c.l_small) > 1 << 32
    a = np.zeros(4, abi.ALNREG_DTYPE)
    a["rb"] = [10, c.l_small - 100, c.l_small, 2 * c.l_small - 150]
    a["re"] = [160, c.l_small, c.l_small + 150, 2 * c.l_small]  # a forward region ending at l_small, a reverse one at 2 l_small
    a["rid"] = [0, 2, 2, 0]
    ta, tb = c.translate(a, False), c.translate(a, True)
    assert ta["rb"].tolist() == [10, c.l_small - 100, 2 * c.l_pac - c.l_small, 2 * c.l_pac - 150]
    assert ta["re"].tolist() == [160, c.l_small, 2 * c.l_pac - c.l_small + 150, 2 * c.l_pac]
    assert ta["rid"].tolist() == [0, 2, 2, 0] and tb["rid"].tolist() == [198, 200, 200, 198]
    assert (tb["rb"] - a["rb"] == c.off_b).all() and (tb["re"] - a["re"] == c.off_b).all()
    # the same bases lie under a translated region: copy B's last forward window and its reverse-strand twin
    pac, L = c.genome["pac"], c.l_pac
    base = lambda x: (int(pac[x >> 2]) >> ((~x & 3) << 1)) & 3  # noqa: E731
    small = G.load_ref()["pac"]
    sbase = lambda x: (int(small[x >> 2]) >> ((~x & 3) << 1)) & 3  # noqa: E731
    for x in (0, 1, 999_999, 123_457):
        assert base(x) == sbase(x) == base(x + c.off_b)
    assert int(c.genome["ann_offset"][198]) == c.off_b and int(c.genome["ann_offset"][-1] + c.genome["ann_len"][-1]) == L


@pytest.mark.parametrize("name", GI.POST_SETS)
def test_post_set(name):
    s = GI.load_post(name)
    for f in (3, 7):
        regs, n = s.want[f]
        assert len(n) == len(s.n) and n.sum() == len(regs) and (n <= s.n).all()
    assert np.array_equal(s.want[3][1], s.want[7][1])
    o3 = s.want[3][0]
    in_b = GI.composite().copy_b(s.want[3][1])
    assert (o3["rid"][in_b] >= 198).all() and (o3["rid"][~in_b] <= 2).all()
    assert (o3["rb"][in_b] >= 1 << 31).all() and (o3["re"][in_b] < 1 << 32).all()
    a_rev = ~in_b & (o3["rb"] >= GI.composite().l_pac)
    assert (o3["rb"][a_rev] >= 1 << 32).all() and (o3["rb"][~in_b & ~a_rev] < 1_000_000).all()


@pytest.mark.parametrize("name", GI.RESCUE_SETS + [GI.CROSS])
def test_rescue_set(name):
    s = GI.load_rescue(name)
    nr = s.n_reads
    assert nr % 2 == 0 and s.n.sum() == len(s.regs) and s.out_n.sum() == len(s.out_regs)
    assert len(s.out_n) == nr and len(s.peak_n) == nr and len(s.n_sw) == nr // 2
    assert (s.peak_n >= s.n).all() and (s.peak_n >= s.out_n).all() and (s.n_sw >= 0).all() and (s.peak_n - s.n <= 8).all()
    if name == GI.CROSS:
        assert nr == 2 * GI.N_CROSS and (s.pes_own["failed"] == 1).all() and s.pes.tobytes() == GI.load_rescue("fr").pes.tobytes()
        r1, r2 = s.regs[s.off[0::2]], s.regs[s.off[1::2]]
        assert (r1["rid"] <= 2).all() and (r2["rid"] >= 198).all()
        assert (np.abs(r2["rb"] - r1["rb"]) > 1 << 31).all()
        assert (s.n_sw > 0).all() and np.array_equal(s.out_n, s.n)  # windows were tried beside both reads; nothing was found
    else:
        assert s.pes.tobytes() == s.pes_own.tobytes() == s.small.pes.tobytes()


@pytest.mark.parametrize("name", GI.PAIR_SETS + [GI.CROSS])
def test_pair_set(name):
    d = GI.load_pair(name)
    check(d)
    if name == GI.CROSS:
        s = d.sel[0]
        assert (s["branch"] == abi.SEL_NO_PAIRING).all() and (s["o"] == 0).all() and (s["extra_flag"] == 1).all()
        assert (d.n_pri.reshape(-1, 2) > 0).all()  # unpaired although both reads have primary hits


def test_alignment_records():
    jobs, exp, ops, mds = GI.load_aln()
    c = GI.composite()
    assert len(jobs) == len(exp) == int((GI.load_pair(GI.ALN_SET).out_mapq[0] >= 0).sum()) > 1000
    ok = exp["status"] == abi.ALN_OK
    assert ok.sum() > len(jobs) // 2 and (exp["n_cigar"][ok] > 0).all()
    rid = exp["rid"][ok]
    assert rid.min() <= 2 and rid.max() >= 198
    g = c.genome
    assert (exp["pos"][ok] >= 0).all() and (exp["pos"][ok] < np.asarray(g["ann_len"])[rid]).all()


def test_floors_are_met():
    c = GI.composite()
    stored = dict.fromkeys(GI.COVERAGE_KEYS, 0)
    for f in GI.all_files():
        z = np.load(os.path.join(G.GOLD, f), allow_pickle=False)
        for k, v in GI.coverage_of(z).items():
            stored[k] += v
    # what the records themselves show must be what the generator counted
    seen = dict.fromkeys(GI.COVERAGE_KEYS, 0)
    inputs = [GI.load_post(n).regs for n in GI.POST_SETS] + [GI.load_rescue(n).regs for n in GI.RESCUE_SETS + [GI.CROSS]] + \
        [GI.split_input()[0]]
    for regs in inputs:
        seen["in_rb_ge_2^32"] += int((regs["rb"] >= 1 << 32).sum())
        seen["in_rb_2^31_to_2^32"] += int(((regs["rb"] >= 1 << 31) & (regs["rb"] < 1 << 32)).sum())
    for n in GI.POST_SETS:
        o3, n3 = GI.load_post(n).want[3]
        patched = (o3["n_comp_is_alt"] & np.uint32(0x3fffffff)) > 1
        in_b = c.copy_b(n3)
        seen["patched_copy_a"] += int((patched & ~in_b).sum())
        seen["patched_copy_b"] += int((patched & in_b).sum())
        seen["patched_rev"] += int((patched & (o3["rb"] >= c.l_pac)).sum())
    for n in GI.PAIR_SETS:
        proper = GI.load_pair(n).sel[0]["branch"] == abi.SEL_PAIRED
        seen["proper_copy_a"] += int(proper[0::2].sum())
        seen["proper_copy_b"] += int(proper[1::2].sum())
    for k in ("in_rb_ge_2^32", "in_rb_2^31_to_2^32", "patched_copy_a", "patched_copy_b", "patched_rev", "proper_copy_a",
              "proper_copy_b"):
        assert seen[k] == stored[k], k
    # regions the rescue added: at least the growth of the reads, by copy and strand
    grown = {"added_rb_ge_2^32": 0, "added_rb_2^31_to_2^32": 0}
    for n in GI.RESCUE_SETS:
        s = GI.load_rescue(n)
        for key, cnt in (("added_rb_ge_2^32", lambda a: int((a["rb"] >= 1 << 32).sum())),
                         ("added_rb_2^31_to_2^32", lambda a: int(((a["rb"] >= 1 << 31) & (a["rb"] < 1 << 32)).sum()))):
            grown[key] += cnt(s.out_regs) - cnt(s.regs)
    for k, v in grown.items():
        assert stored[k] >= v >= GI.FLOORS[k], (k, stored[k], v)
    short = {k: (stored[k], f) for k, f in GI.FLOORS.items() if stored[k] < f}
    assert not short, f"coverage floors not met (have, need): {short}"
    rids = GI.all_rids()
    assert GI.contigs_ok(rids) and {0, 1, 2, 198, 199, 200} <= rids
    assert (GI.load_rescue("mixed").pes["failed"] == 0).sum() >= 2


def test_a_changed_input_is_refused():
    s = GI.rescue_input("shift")
    z = np.load(os.path.join(G.GOLD, "grch_rescue_shift.npz"), allow_pickle=False)
    GI._check_input(z, "rescue", "shift", s.in_sha256)
    regs = s.regs.copy()
    regs["rb"][0] ^= 1 << 32  # one high bit of one coordinate
    with pytest.raises(RuntimeError):
        GI._check_input(z, "rescue", "shift", GI.digest(s.seq_off, s.seq, s.n, regs, s.alt))


def test_reference_again_on_the_first_pairs():
    """only this part needs oracle/_ref: mem_pestat on the whole set and the rescue loop on its first 50 pairs"""
    if oracle.ref_lib() is None:
        pytest.skip("oracle/_ref not built")
    sys.path.insert(0, os.path.join(REPO, "tools_dev"))
    import gen_grch_pair_fixture as gen
    s = GI.load_rescue("ends")
    rs = gen.GrchSel(s.opt, gen.pairopt_dict(s), s.genome, s.alt)
    assert rs.pestat(gen.per_read(s.regs, s.n)).tobytes() == s.pes.tobytes()
    out, out_n, n_sw, peak_n = gen.rescue_expected(s, s.pes, n_pairs=50)
    assert np.array_equal(out_n, s.out_n[:100]) and np.array_equal(n_sw, s.n_sw[:50]) and np.array_equal(peak_n, s.peak_n[:100])
    assert G.region_mismatch(out, s.out_regs[:int(s.out_n[:100].sum())]) is None
    p = gen.post_expected(GI.load_post("sv"), reads=range(100))
    want, n = GI.load_post("sv").want[3]
    assert np.array_equal(p[3][1], n[:100]) and G.region_mismatch(p[3][0], want[:int(n[:100].sum())]) is None
