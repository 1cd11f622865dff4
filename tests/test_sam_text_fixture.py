"""The SAM text fixtures (tests/golden/sam_text_<set>.npz, tools_dev/gen_sam_fixture.py)
load, are consistent with the pair fixtures they extend, cover what the generator's
floors promise, and the hand-built pairs say what they were built to say; the
Python mirror of bwagpu_samtext_t has the header's layout.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import golden_io as G
import sam_io as S
from bwagpu import abi

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIELDS = [k for k, _ in abi.SamText._fields_]
LAYOUT_C = ("#include <stddef.h>\n#include <stdio.h>\n#include \"bwagpu.h\"\nint main(void) {\n"
            "  printf(\"%zu\\n\", sizeof(bwagpu_samtext_t));\n" +
            "".join(f"  printf(\"%zu\\n\", offsetof(bwagpu_samtext_t, {k}));\n" for k in FIELDS) +
            "  printf(\"%d %d %d %d %d %d %d %d\\n\", BWAGPU_SAM_DONE, BWAGPU_SAM_SKIPPED, BWAGPU_SAM_NEEDS_HOST,\n"
            "         BWAGPU_SAM_NO_ROOM, BWAGPU_SAM_MAX_RG, BWAGPU_MEM_F_REF_HDR, BWAGPU_MEM_F_SOFTCLIP, BWAGPU_MEM_F_XB);\n"
            "  printf(\"%d\\n\", BWAGPU_ABI_VERSION);\n  return 0;\n}\n")


def test_samtext_layout_equals_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = abi.SamText
    assert got[:1 + len(FIELDS)] == [C.sizeof(T)] + [getattr(T, k).offset for k in FIELDS]
    assert C.sizeof(T) == 224 and T.rg_id.offset == 152 and T.text_cap.offset == 184 and T.dev_text_n.offset == 216
    assert got[1 + len(FIELDS):] == [abi.SAM_DONE, abi.SAM_SKIPPED, abi.SAM_NEEDS_HOST, abi.SAM_NO_ROOM, abi.SAM_MAX_RG,
                                     abi.MEM_F_REF_HDR, abi.MEM_F_SOFTCLIP, abi.MEM_F_XB, 1]
    assert "bwagpu_sam_text_device" in abi.PROTOS


def test_file_sizes_and_floors():
    for name in S.SETS + ["cases", "aln"]:
        assert os.path.getsize(os.path.join(G.GOLD, f"sam_text_{name}.npz")) <= S.MAX_BYTES, name
    cov = S.coverage()
    for k, floor in S.FLOORS.items():
        assert cov[k] >= floor >= 1, (k, cov[k], floor)
    assert set(S.FLOORS) == set(S.COVERAGE_KEYS)


@pytest.mark.parametrize("name", S.SETS + ["cases"])
def test_spans_and_line_counts(name):
    d, seq_off, seq, runs = S.load(name)
    assert len(seq_off) == d.n_reads + 1 and seq_off[-1] == len(seq)
    assert sorted(runs) == sorted(S.keys_of(name) if name != "cases" else S.KEYS)
    for key, t in runs.items():
        mode, _ = S.KEYS[key]
        om = d.out_mapq[mode]
        assert t.n_reads == d.n_reads and t.off[0] == 0 and t.off[-1] == len(t.text) and b"\0" not in t.text
        for r in range(d.n_reads):
            n_rec = int((om[d.off[r]:d.off[r] + d.n[r]] >= 0).sum())
            assert t.n_lines[r] == max(1, n_rec), (key, r)
            if r < t.n_full:
                b = t.span(r)
                assert b.endswith(b"\n") and b.count(b"\n") == t.n_lines[r], (key, r)
                for line in b.split(b"\n")[:-1]:
                    assert line.split(b"\t")[0] == S.pair_name("cases" if name == "cases" else name, r >> 1)
                    assert b"\tRG:Z:" + S.RG_ID in line


def test_stored_digests_are_of_the_text():
    """the digest path of SamText.mismatch, on a file cut by hand: whole text for two reads, digests after"""
    _, _, _, runs = S.load("cases")
    t = runs["pair"]
    whole = {r: t.span(r) for r in range(t.n_reads)}
    cut = S.SamText.__new__(S.SamText)
    cut.off, cut.text, cut.n_full, cut.n_reads = t.off[:3], t.text[:t.off[2]], 2, t.n_reads
    cut.digests = np.frombuffer(b"".join(S.digest(whole[r]) for r in range(2, t.n_reads)), np.uint8).reshape(-1, 16)
    assert cut.mismatch(t.off, t.text) is None
    bad = bytearray(t.text)
    bad[t.off[5]] ^= 1
    assert cut.mismatch(t.off, bytes(bad)).startswith("read 5:")
    bad = bytearray(t.text)
    bad[t.off[1]] ^= 1
    assert cut.mismatch(t.off, bytes(bad)).startswith("read 1:")


def lines_of(t, r):
    return [x.split("\t") for x in t.span(r).decode().split("\n")[:-1]]


def test_cases_say_what_they_were_built_for():
    d, _, _, runs = S.load("cases")
    pair = {name: p for p, name in enumerate(S.CASES)}
    t, tn, to = runs["pair"], runs["nopair"], runs["other"]
    # a primary of 65 under an ALT hit of 80, and the {h, g} list with SA:Z on both lines
    h, g = lines_of(t, 2 * pair["pa_65_80"])
    assert "pa:f:0.812" in h and "AS:i:65" in h and int(g[1]) & 0x800 and "AS:i:80" in g
    assert any(f.startswith("SA:Z:") for f in h) and any(f.startswith("SA:Z:") for f in g)
    assert "S" not in g[5] or "H" not in g[5]
    assert int(d.sel[0][pair["h_g"]]["alt"][0]) >= 0 and len(lines_of(t, 2 * pair["h_g"])) == 2
    # the supplementary line hard-clips, and shows its clipped mate's CIGAR with H; the mate's own line has S
    prim, supp = lines_of(tn, 2 * pair["supp_mate_clipped"])
    (mate,) = lines_of(tn, 2 * pair["supp_mate_clipped"] + 1)
    assert "H" in supp[5] and "S" in prim[5] and len(supp[9]) == 75 and len(prim[9]) == 150
    mc = [f for f in supp if f.startswith("MC:Z:")][0]
    assert "S" in mate[5] and mc == "MC:Z:" + mate[5].replace("S", "H")
    assert [f for f in prim if f.startswith("MC:Z:")][0] == "MC:Z:" + mate[5]
    (soft,) = [x for x in lines_of(to, 2 * pair["supp_mate_clipped"]) if int(x[1]) & 0x800] or [None]
    assert soft is None or "H" not in soft[5]
    # unaligned beside a reverse-strand mate: the mate's coordinates, the reverse complement, TLEN 0, AS and XS 0
    (u,) = lines_of(t, 2 * pair["unaligned_rev_mate"])
    (m,) = lines_of(t, 2 * pair["unaligned_rev_mate"] + 1)
    assert int(u[1]) & 0x14 == 0x14 and u[2:6] == [m[2], m[3], "0", "*"] and u[8] == "0"
    assert "AS:i:0" in u and "XS:i:0" in u and not any(f.startswith("MC:Z:") for f in m)
    (u2,) = lines_of(t, 2 * pair["unaligned_fwd_mate"] + 1)
    assert int(u2[1]) & 0x14 == 0x4
    (b0,) = lines_of(t, 2 * pair["both_unaligned"])
    assert int(b0[1]) & 0xc == 0xc and b0[2:9] == ["*", "0", "0", "*", "*", "0", "0"]
    # XB carries the score
    xa = [f for f in lines_of(t, 2 * pair["two_strings"])[0] if f.startswith("XA:Z:")][0]
    xb = [f for f in lines_of(to, 2 * pair["two_strings"])[0] if f.startswith("XB:Z:")][0]
    assert len(xa.split(";")[0].split(",")) == 4 and len(xb.split(";")[0].split(",")) == 5


def test_aln_cases_reach_what_reads_do_not():
    a = S.load_aln()
    n_ops = sorted(set(a["aln"]["n_cigar"].tolist()))
    assert {1, 63, 64, 65, 200} <= set(n_ops) and max(n_ops) <= S.ALN_MAX_OPS
    lens = set((a["seq_off"][1:] - a["seq_off"][:-1]).tolist())
    assert {1, 63, 64, 65, 250} <= lens
    assert {1, S.ALN_MAX_MD - 1} <= set(a["aln"]["md_len"].tolist())
    assert a["aln"]["pos"].max() > 1 << 32 and a["aln"]["pos"].min() == 0
    assert set(a["aln"]["is_rev"].tolist()) == {0, 1}
    q, nq = a["with_qual"], a["no_qual"]
    assert q.n_reads == nq.n_reads == len(a["n"]) and q.n_full == q.n_reads
    for r in range(q.n_reads):
        for lq, ln in zip(lines_of(q, r), lines_of(nq, r)):
            assert ln[10] == "*" and lq[:10] == ln[:10] and lq[11:] == ln[11:] and len(lq[10]) == len(lq[9])
