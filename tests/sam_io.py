"""Loader of tests/golden/sam_text_<set>.npz (tools_dev/gen_sam_fixture.py: the text
the reference's own mem_sam_pe leaves in bseq1_t.sam on the pair sets and on
hand-built pairs, and what its mem_aln2sam prints for hand-built mem_aln_t lists),
and the inputs the text was made with that need no storing: read names, qualities,
comments, contig names and the read group come from the small formulas below."""
from __future__ import annotations

import functools
import hashlib
import os

import numpy as np

import golden_io as G
import xa_io as X
from bwagpu import abi

SETS = X.SETS
RG_ID = b"grp1.lane-7"
MAX_OPS, MAX_MD = 128, 512          # the slots of the sets' records
ALN_MAX_OPS, ALN_MAX_MD = 256, 64   # the slots of the mem_aln2sam cases
# key -> (mode of the pair fixtures: 0 pairing, 1 MEM_F_NOPAIRING; further mem_opt_t.flag bits)
KEYS = {"pair": (0, 0), "nopair": (1, 0), "other": (0, abi.MEM_F_SOFTCLIP | abi.MEM_F_XB)}
OTHER_SET = "ends"  # the one set that also runs under MEM_F_SOFTCLIP | MEM_F_XB
CASES = ["pa_65_80", "h_g", "supp_mate_clipped", "unaligned_rev_mate", "unaligned_fwd_mate", "both_unaligned",
         "two_strings"]
COVERAGE_KEYS = ("lines", "xa", "sa", "mc", "pa", "hard_clipped", "reverse", "unmapped_mate_fwd", "unmapped_mate_rev",
                 "both_unmapped", "hg_lists", "nopair_multi_lines")
# half of what the reference yields on these inputs (gen_sam_fixture.py prints the counts), at least 1
FLOORS = dict(lines=9159, xa=1762, sa=93, mc=8429, pa=43, hard_clipped=2, reverse=4082, unmapped_mate_fwd=608,
              unmapped_mate_rev=116, both_unmapped=3, hg_lists=25, nopair_multi_lines=43)
MAX_BYTES = 1 << 20

_ALNUM = "abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def pair_name(tag: str, p: int) -> bytes:
    """the name both reads of pair p carry: 1 to 70 bytes"""
    s = f"{p:x}.{tag}:" + _ALNUM * 2
    return s[:1 + (p * 7) % 70].encode()


def read_qual(r: int, l_seq: int) -> np.ndarray:
    j = np.arange(l_seq, dtype=np.int64)
    return (33 + (7 * r + 3 * j + (j * j) % 11) % 41).astype(np.uint8)


def read_comment(r: int) -> bytes:
    return b"" if r % 3 else b"BC:Z:" + _ALNUM[r % 50:r % 50 + 1 + r % 17].encode()


def contig_name(i: int) -> bytes:
    return f"c{i}".encode() + b"_alt" * (i % 3) + b"Z" * (i % 5)


def blob(parts):
    """byte strings -> (int64 offsets[n + 1], uint8 blob)"""
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in parts])
    return off, np.frombuffer(b"".join(parts), np.uint8).copy()


def read_inputs(tag: str, seq_off) -> dict:
    """names, qualities and comments of the reads whose bases are at seq_off"""
    n = len(seq_off) - 1
    name_off, names = blob([pair_name(tag, r >> 1) for r in range(n)])
    com_off, comments = blob([read_comment(r) for r in range(n)])
    qual = np.zeros(int(seq_off[-1]), np.uint8)
    for r in range(n):
        qual[seq_off[r]:seq_off[r + 1]] = read_qual(r, int(seq_off[r + 1] - seq_off[r]))
    return dict(name_off=name_off, names=names, comment_off=com_off, comments=comments, qual=qual)


def contigs(n: int):
    return blob([contig_name(i) for i in range(n)])


def digest(b: bytes) -> bytes:
    return hashlib.blake2b(b, digest_size=16).digest()


def line_events(text: str, ev: dict):
    """counts of COVERAGE_KEYS that one read's text shows"""
    for line in text.split("\n")[:-1]:
        f = line.split("\t")
        flag = int(f[1])
        ev["lines"] += 1
        ev["xa"] += "\tXA:Z:" in line or "\tXB:Z:" in line
        ev["sa"] += "\tSA:Z:" in line
        ev["mc"] += "\tMC:Z:" in line
        ev["pa"] += "\tpa:f:" in line
        ev["hard_clipped"] += "H" in f[5]
        ev["reverse"] += bool(flag & 0x10)
        if flag & 4:
            ev["both_unmapped" if flag & 8 else "unmapped_mate_rev" if flag & 0x10 else "unmapped_mate_fwd"] += 1


class SamText:
    """one run's expected text: whole for the first n_full reads (off, text), a blake2b-16 digest for each
    later read; n_lines per read"""

    def __init__(self, z, pre):
        self.off = z[pre + "off"].astype(np.int64)
        self.text = z[pre + "text"].tobytes()
        self.digests = z[pre + "digest"]
        self.n_lines = z[pre + "n_lines"].astype(np.int64)
        self.n_full = len(self.off) - 1
        self.n_reads = self.n_full + len(self.digests)

    def span(self, r):
        return self.text[self.off[r]:self.off[r + 1]]

    def mismatch(self, got_off, got: bytes):
        """the first read whose device text differs -> message, or None"""
        for r in range(self.n_reads):
            b = got[got_off[r]:got_off[r + 1]]
            if r < self.n_full:
                if b != self.span(r):
                    return f"read {r}: {b!r} != {self.span(r)!r}"
            elif digest(b) != self.digests[r - self.n_full].tobytes():
                return f"read {r}: digest differs; device text {b!r}"
        return None


def _file(name):
    return np.load(os.path.join(G.GOLD, f"sam_text_{name}.npz"), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def coverage() -> dict:
    tot = dict.fromkeys(COVERAGE_KEYS, 0)
    for name in SETS + ["cases"]:
        for k, v in zip(COVERAGE_KEYS, _file(name)["coverage"].tolist()):
            tot[k] += int(v)
    return tot


def keys_of(name):
    return ["pair", "nopair"] + (["other"] if name == OTHER_SET else [])


@functools.lru_cache(maxsize=None)
def load(name):
    """-> (XaData of the set or of the hand-built pairs, seq_off, seq, {key: SamText})"""
    z = _file(name)
    if name == "cases":
        pre = "cases_"
        d = X.XaData("sam_cases", z[pre + "n"].astype(np.int32),
                     {0: z[pre + "final"].astype(abi.ALNREG_DTYPE), 1: z[pre + "marked"].astype(abi.ALNREG_DTYPE)},
                     {0: z[pre + "sel"].astype(abi.PAIRSEL_DTYPE), 1: z[pre + "sel_nopair"].astype(abi.PAIRSEL_DTYPE)},
                     {0: z[pre + "out_mapq"].astype(np.int32), 1: z[pre + "out_mapq_nopair"].astype(np.int32)},
                     None, G.load_ref(), G.opt_of(z), z["alt"])
        seq_off, seq = z["seq_off"].astype(np.int64), z["seq"].astype(np.uint8)
        keys = ["pair", "nopair", "other"]
    else:
        import rescue_io as R
        d, s = X.load(name), R.load(name)
        seq_off, seq = s.seq_off.astype(np.int64), s.seq.astype(np.uint8)
        keys = keys_of(name)
    return d, seq_off, seq, {k: SamText(z, k + "_") for k in keys}


@functools.lru_cache(maxsize=None)
def load_aln() -> dict:
    """the mem_aln2sam cases: every array bwagpu_sam_text_device takes, as the generator built them, and the
    reference's text with and without qualities"""
    z = _file("aln")
    d = {k: z[k] for k in z.files}
    d["with_qual"], d["no_qual"] = SamText(z, "q_"), SamText(z, "nq_")
    return d
