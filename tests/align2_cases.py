"""ksw_align2 task families at the limits of the batched local Smith-Waterman
(bwa-flow_amd/csrc/align2.hip).  Plain numpy, seeded, no GPU.  Every boundary
number below comes from the gate or the reference line it names, never from a
kernel's output:

  align2_opt_unsupported(o)  pure.h   o_del + e_del <= 65535, o_ins + e_ins <= 65535: ksw_i16 keeps
                                      16 bits of them (_mm_set1_epi16, ksw.c:252-255); every task
  align2_byte_ok(o)          pure.h   e_del, e_ins, o_del + e_del, o_ins + e_ins <= 255: ksw_u8
                                      keeps 8 bits (_mm_set1_epi8, ksw.c:132-135); XBYTE tasks only
  align2_word_fits(qlen, mm) pure.h   qlen * max(mat) <= 32767 (adds_epi16 clamps there); word tasks
  gmax + shift >= 255                 ksw_u8's saturation (ksw.c:201): no gate, both sides admitted
  BIG = 2^26                          align2.hip's segmented scan, see WORD_BIG_DERIVATION

A family is {side: Family}.  A side named "in..." is one option set whose every
task the entries admit, a side named "out..." holds the first refused value:
Family.refused marks the tasks a per-task gate refuses (bwagpu_align2_device
answers those with seven -1 and runs the others; bwagpu_align2_batch refuses
the batch), Family.opt_refused says that the options themselves are refused
(every entry then returns E_UNSUPPORTED).  tests/golden/align2_range.npz holds
the reference's kswr_t for every task of every side (oracle/gen_golden.py
--only-align2-range), the truncated results of the refused ones included.

Tasks (20..40 a side, qlen <= 255 but where a family says otherwise, targets
of qlen + 0..300 bases):
  * planted: the target holds a copy of the query with 1..3 extra bases at one
    third (a deletion: E, o_del / e_del) and 1..3 query bases missing at two
    thirds (an insertion: F, o_ins / e_ins), lengths cycling 1, 2, 3 so that
    one-base gaps (free once o + e wraps to 0) are always there;
  * planted + a second partial copy, so that score2 / te2 are live;
  * synth.mate_rescue_tasks in "mix" mode for the rest;
  * exact: query bases 0..2 and target filler 3, so that nothing matches
    outside the planted copies and scores are known in closed form
    (Family.expect: task index -> the fields the reference must report).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from bwagpu import abi, synth

XB, XSTOP, XSUBO, XSTART = abi.KSW_XBYTE, abi.KSW_XSTOP, abi.KSW_XSUBO, abi.KSW_XSTART

# align2.hip adds BIG * segment to X = T + j * e_ins and needs X < BIG = 2^26 = 67108864:
#   j <= 1023       (qlen <= BWAGPU_MAX_READ_LEN = 1023 -> at most 8 * 128 = 1024 columns)
#   e_ins <= 65534  (o_ins >= 1 and o_ins + e_ins <= 65535: align2_opt_unsupported)
#   T <= 32767      (word tasks: align2_word_fits; byte tasks: T <= 255)
#   X <= 32767 + 1023 * 65534 = 67074049 = 2^26 - 34815
# word-BIG runs qlen 1023 with e_ins = 65534 and a live T in its last column (j = 1022).
WORD_BIG_DERIVATION = 32767 + 1023 * 65534
assert WORD_BIG_DERIVATION == (1 << 26) - 34815


@dataclass
class Family:
    opt: dict
    tasks: np.ndarray
    qpool: np.ndarray
    tpool: np.ndarray
    gate: str                 # the clause this side sits at
    side: str
    refused: np.ndarray       # bool per task: a per-task gate refuses it under these options
    opt_refused: bool = False  # align2_opt_unsupported refuses the options
    expect: dict = field(default_factory=dict)   # task index -> {kswr field: value} the reference must report
    names: dict = field(default_factory=dict)    # task index -> the variant's name (flag equalities)


def _opt(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, mat=None):
    return dict(a=a, b=b, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, pen_clip5=5, pen_clip3=5, w=100,
                zdrop=100, mat=abi.fill_scmat(a, b) if mat is None else np.asarray(mat, np.int8))


def max_mat(opt):
    return max(0, int(np.asarray(opt["mat"], np.int8).max()))


def shift_of(opt):
    """ksw_qinit's shift (ksw.c:78-86): minus the matrix minimum as a byte"""
    return (256 - (int(np.asarray(opt["mat"], np.int8)[:25].min()) & 0xff)) & 0xff


def byte_ok(opt):
    """align2_byte_ok, pure.h"""
    return max(opt["e_del"], opt["e_ins"], opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"]) <= 255


def word_ok(opt):
    """align2_opt_unsupported's word limit, pure.h"""
    return max(opt["o_del"] + opt["e_del"], opt["o_ins"] + opt["e_ins"]) <= 65535


class _Build:
    def __init__(self, rng):
        self.rng = rng
        self.tasks, self.qs, self.ts, self.qo, self.to = [], [], [], 0, 0
        self.expect, self.names = {}, {}

    def add(self, q, t, xtra, expect=None, name=None):
        q, t = np.asarray(q, np.uint8), np.asarray(t, np.uint8)
        k = len(self.tasks)
        self.tasks.append((self.qo, self.to, len(q), len(t), int(xtra), 0))
        self.qs.append(q)
        self.ts.append(t)
        self.qo += len(q)
        self.to += len(t)
        if expect is not None:
            self.expect[k] = expect
        if name is not None:
            self.names[k] = name
        return k

    def extend(self, tasks, qp, tp, clear=0, force=0):
        """a synth batch; clear / force: xtra bits taken off / put on every task"""
        for t in tasks:
            self.add(qp[t["qoff"]:t["qoff"] + t["qlen"]], tp[t["toff"]:t["toff"] + t["tlen"]],
                     (int(t["xtra"]) & ~clear) | force)

    def planted(self, ql, k, xtra, second=False):
        """the module docstring's planted task: gap lengths 1 + k % 3 and 1 + (k + 1) % 3"""
        rng = self.rng
        q = rng.integers(0, 4, ql).astype(np.uint8)
        kd, ki = 1 + k % 3, 1 + (k + 1) % 3
        i, j = ql // 3, 2 * ql // 3
        copy = np.concatenate([q[:i], rng.integers(0, 4, kd), q[i:j], q[j + ki:]]).astype(np.uint8)
        flank = max(0, int(rng.integers(0, 301)) - (kd - ki))
        pre = int(rng.integers(0, flank + 1))
        t = np.concatenate([rng.integers(0, 4, pre), copy, rng.integers(0, 4, flank - pre)]).astype(np.uint8)
        if second and flank - pre >= ql // 2:  # a partial copy in the tail
            p2 = pre + len(copy) + int(rng.integers(0, flank - pre - ql // 2 + 1))
            t[p2:p2 + ql // 2] = q[:ql // 2]
        return self.add(q, t, xtra)

    def done(self, opt, gate, side):
        tasks = np.array(self.tasks, abi.ALIGN2_TASK_DTYPE)
        u8 = (tasks["xtra"] & XB) != 0
        refused = np.where(u8, not byte_ok(opt), tasks["qlen"].astype(np.int64) * max_mat(opt) > 32767)
        return Family(opt, tasks, np.concatenate(self.qs).astype(np.uint8), np.concatenate(self.ts).astype(np.uint8),
                      gate, side, refused.astype(bool), not word_ok(opt), self.expect, self.names)


MATESW = XSUBO | XSTART | 19  # what mem_matesw passes (bwamem_pair.c:150) but XBYTE, which the families set


def _gate_family(rng, opt, gate, side, with_bytes):
    """planted and synth tasks under one option set: byte and word tasks (with_bytes), or word tasks only"""
    b = _Build(rng)
    qlens = (33, 64, 100, 150, 200, 249)
    for k in range(12):
        u8 = XB if (with_bytes and k % 2 == 0) else 0
        flags = (MATESW, XSTART, MATESW, 0)[k % 4] if k < 8 else MATESW
        b.planted(int(qlens[k % len(qlens)]), k, flags | u8, second=k >= 8)
    s = synth.mate_rescue_tasks(rng, 10, a=opt["a"], qlens=(50, 100, 150), win=(0, 300), xtra_mode="mix")
    if with_bytes:
        b.extend(s[0][:5], s[1], s[2], force=XB)
        b.extend(s[0][5:], s[1], s[2], clear=XB)
    else:
        b.extend(*s, clear=XB)
    return b.done(opt, gate, side)


def _exact_q(rng, n):
    return rng.integers(0, 3, n).astype(np.uint8)


def _fill(n):
    return np.full(n, 3, np.uint8)


def _sat_family(rng, opt, qlens, gate):
    """perfect copies around gmax + shift == 254 / 255: score qlen while qlen + shift <= 254, else 255 with qe -1"""
    b = _Build(rng)
    sh = shift_of(opt)
    for ql in qlens:
        sat = ql + sh >= 255
        for v in range(4):
            q = _exact_q(rng, ql)
            pre, post = ((0, 0), (17, 40), (5, 0), (0, 120))[v]
            te = pre + ql - 1
            if sat:  # the first row whose maximum + shift reaches 255 ends the pass (ksw.c:201)
                exp = dict(score=255, te=pre + (255 - sh) - 1, qe=-1, tb=-1, qb=-1, score2=-1, te2=-1)
            else:
                exp = dict(score=ql, te=te, qe=ql - 1, score2=-1, te2=-1)
                if v != 3:
                    exp.update(tb=pre, qb=0)
            b.add(q, np.concatenate([_fill(pre), q, _fill(post)]), XB | (XSTART if v != 3 else 0), expect=exp)
    b.extend(*synth.mate_rescue_tasks(rng, 4, a=max_mat(opt), qlens=(60, 120), win=(0, 300), xtra_mode="mix"), force=XB)
    return b.done(opt, gate, "in")


def _flag_family(rng):
    """equality cases of XSTOP and XSUBO and the [te - k, te + k] window of the second-best score, under the
    defaults, on perfect copies of score S = 64 (a multiple of 16: no padding columns in either width, whose
    score-0 diagonal would carry S one row on).  k = ceil(S / max) = 64; the second copy is the query's last
    M = 24 bases with minsc = M, so that its only row maximum >= minsc is its last row."""
    b = _Build(rng)
    S, M = 64, 24
    for u8 in (XB, 0):
        w = "byte" if u8 else "word"
        q = _exact_q(rng, S)
        p = 30
        t = np.concatenate([_fill(p), q, _fill(100)])
        te = p + S - 1
        full = dict(score=S, te=te, qe=S - 1)
        b.add(q, t, u8 | XSTOP | (S - 1), name=f"{w}:xstop=S-1 stops a row early",
              expect=dict(score=S - 1, te=te - 1, qe=S - 2, tb=-1, qb=-1))
        b.add(q, t, u8 | XSTOP | S, name=f"{w}:xstop=S stops at te", expect=dict(full, tb=-1, qb=-1))
        b.add(q, t, u8 | XSTOP | (S + 1), name=f"{w}:xstop=S+1 never stops", expect=dict(full, tb=-1, qb=-1))
        b.add(q, t, u8 | XSUBO | XSTART | S, name=f"{w}:xsubo minsc=S runs the reverse pass",
              expect=dict(full, tb=p, qb=0, score2=-1, te2=-1))
        b.add(q, t, u8 | XSUBO | XSTART | (S + 1), name=f"{w}:xsubo minsc=S+1 skips the reverse pass (ksw.c:356)",
              expect=dict(full, tb=-1, qb=-1, score2=-1, te2=-1))
        b.add(q, t, u8 | XSUBO | XSTART | 0xffff, name=f"{w}:minsc=0xffff", expect=dict(full, tb=-1, qb=-1, score2=-1,
                                                                                       te2=-1))
        k = S
        for d, inside in ((-k - 1, False), (-k, True), (k, True), (k + 1, False)):
            # main copy at rows p .. te, the second copy's last row at te + d
            p = M + 12
            te = p + S - 1
            r2 = te + d
            t = _fill(te + k + 1 + 40)
            t[p:p + S] = q
            t[r2 - M + 1:r2 + 1] = q[S - M:]
            exp = dict(score=S, te=te, qe=S - 1, tb=p, qb=0)
            exp.update(dict(score2=-1, te2=-1) if inside else dict(score2=M, te2=r2))
            b.add(q, t, u8 | XSUBO | XSTART | M, expect=exp,
                  name=f"{w}:second copy at te{d:+d} is {'inside' if inside else 'outside'} the window")
    b.extend(*synth.mate_rescue_tasks(rng, 4, qlens=(64, 100), win=(0, 300), xtra_mode="mix"))
    return b.done(_opt(), "ksw.c:199-204 (XSTOP), 343-344 / 356 (XSUBO, XSTART), 215-225 (the second best's window)", "in")


def gapless_best(opt, q, t):
    """the best local score with no gap at all: every diagonal's best run (plain numpy)"""
    mat = np.asarray(opt["mat"], np.int64).reshape(5, 5)
    best, h = 0, np.zeros(len(q) + 1, np.int64)
    for tb in t:
        h[1:] = np.maximum(h[:-1] + mat[tb][q], 0)
        h[0] = 0
        best = max(best, int(h.max()))
    return best


def _big_family(rng):
    """e_ins = 65534, o_ins = 1, a = 1, qlen 1000 / 1023: the target is the query without two bases, so the
    insertion is there to take and costs 131069.  No alignment with a gap can pay for it, so the score is the best
    gapless one (Family.expect, from gapless_best), and where the half after the insertion is the longer one the
    last column holds it: X = T + 1022 * 65534, the largest value the scan sees (WORD_BIG_DERIVATION)."""
    opt = _opt(o_ins=1, e_ins=65534)
    b = _Build(rng)
    for ql in (1000, 1023):
        for v in range(10):
            q = _exact_q(rng, ql)
            cut = (ql // 4, ql // 3, ql // 2 - 1, 40, ql - 40)[v % 5]
            tq = np.concatenate([q[:cut], q[cut + 2:]])
            pre = (0, 13, 150)[v % 3]
            t = np.concatenate([_fill(pre), tq, _fill((2, 148, 20)[v % 3])])
            exp = dict(score=gapless_best(opt, q, t))
            if ql - cut - 2 > cut + 2:
                exp.update(qe=ql - 1, te=pre + len(tq) - 1)
            b.add(q, t, (XSTART, MATESW, 0)[v % 3], expect=exp)
    return b.done(opt, "align2.hip: T + j * e_ins < BIG = 2^26", "in")


def _ceiling_family(rng, side):
    """a = b = 127, perfect copies: qlen 257 -> 32639, 258 -> 32766 (the last admitted, and one column bucket
    further than 256 columns); "out": 259 -> 32893 > 32767 beside them"""
    opt = _opt(a=127, b=127)
    b = _Build(rng)
    for ql in (257, 258) + ((259,) if side == "out" else ()):
        for v in range(8 if side == "in" else 6):
            q = _exact_q(rng, ql)
            pre, post = ((0, 0), (9, 30), (0, 200), (100, 0))[v % 4]
            exp = dict(score=127 * ql, te=pre + ql - 1, qe=ql - 1) if ql <= 258 else None
            if exp and v % 2 == 0:
                exp.update(tb=pre, qb=0)
            b.add(q, np.concatenate([_fill(pre), q, _fill(post)]), XSTART if v % 2 == 0 else 0, expect=exp)
    s = synth.mate_rescue_tasks(rng, 6, a=127, qlens=(100, 257, 258), win=(0, 300), xtra_mode="mix")
    b.extend(*s, clear=XB)
    return b.done(opt, "align2_word_fits: qlen * max(mat) <= 32767", side)


def families(seed: int = 20261) -> dict:
    """-> {name: {side: Family}}"""
    rng = np.random.default_rng(seed)
    fams: dict = {}
    BYTE = "align2_byte_ok: e_del, e_ins, o_del + e_del, o_ins + e_ins <= 255 (XBYTE tasks)"
    WORD = "align2_opt_unsupported: o_del + e_del, o_ins + e_ins <= 65535"

    def sides(name, gate, with_bytes, **opts):
        fams[name] = {s: _gate_family(rng, _opt(**kw), gate, s, with_bytes) for s, kw in opts.items()}

    sides("byte-oe_del", BYTE, True, **{"in": dict(o_del=254, e_del=1), "out": dict(o_del=255, e_del=1)})
    sides("byte-oe_ins", BYTE, True, **{"in": dict(o_ins=254, e_ins=1), "out": dict(o_ins=255, e_ins=1)})
    sides("byte-e_del", BYTE, True, **{"in": dict(e_del=254, o_del=1), "out": dict(e_del=255, o_del=1),
                                       "out2": dict(e_del=256, o_del=0)})
    sides("byte-e_ins", BYTE, True, **{"in": dict(e_ins=254, o_ins=1), "out": dict(e_ins=255, o_ins=1)})
    sides("byte-mixed", BYTE, True, **{"out": dict(o_del=300)})
    sides("word-oe_del", WORD, False, **{"in": dict(o_del=65534, e_del=1), "out": dict(o_del=65535, e_del=1)})
    sides("word-oe_ins", WORD, False, **{"in": dict(o_ins=65534, e_ins=1), "in2": dict(e_ins=65534, o_ins=1),
                                         "out": dict(o_ins=65535, e_ins=1), "out2": dict(e_ins=65535, o_ins=1)})
    fams["word-BIG"] = {"in": _big_family(rng)}
    fams["word-ceiling"] = {"in": _ceiling_family(rng, "in"), "out": _ceiling_family(rng, "out")}

    SAT = "ksw_u8: gmax + shift >= 255 (ksw.c:201), shift = %d"
    fams["byte-sat-shift4"] = {"in": _sat_family(rng, _opt(), (249, 250, 251, 252), SAT % 4)}
    fams["byte-sat-shift127"] = {"in": _sat_family(rng, _opt(b=127), (126, 127, 128, 129, 130), SAT % 127)}
    m128 = abi.fill_scmat(1, 127).copy()
    m128[1] = -128
    fams["byte-sat-shift128"] = {"in": _sat_family(rng, _opt(b=127, mat=m128), (125, 126, 127, 128), SAT % 128)}
    m0 = np.zeros(25, np.int8)
    m0[[0, 6, 12, 18]] = 1  # match 1, mismatch and N 0
    fams["byte-sat-shift0"] = {"in": _sat_family(rng, _opt(b=0, mat=m0), (253, 254, 255, 256), SAT % 0)}
    fams["flags"] = {"in": _flag_family(rng)}
    return fams


def is_in(side):
    return side.startswith("in")


def flat(fams=None):
    """-> [(name, side, Family)] in a fixed order"""
    fams = families() if fams is None else fams
    return [(n, s, f) for n, d in fams.items() for s, f in d.items()]
